"""Measures the CSV decoder on an MI355X -> profiles/csv_bench.json.

    python tools/csv_bench.py [--n 1048576] [--out profiles/csv_bench.json]

* the corpus: 1 Mi values of exactly 512 bytes, 12 fields each (2048 distinct values, tiled), resident in device memory, in two forms:
  all fields unquoted, and with 20 % of the fields quoted, one `""` in every quoted field.  The three-byte-separator row reads the same
  fields joined by U+FF0C (the last field shortened so that the value keeps its 512 bytes).
* kernels: HIP events, 3 warm-up launches, 5 timed launches, min / median / max; everything that is compared is timed in the SAME run,
  alternating:
    - csv_split_kernel (W = 16): TrimLeadingSpace off, on, and the three-byte separator,
    - delim_split_kernel on the bytes of the first two rows, separator `,`, quote `"`, 16 columns kept: the figure to beat is its time
      per byte, the margin the spread (max - min) of its five runs,
    - a device-to-device copy of the corpus.
* the first 2048 values of every csv_split_kernel row are compared with tests/helpers/csv_model.py before anything is written.
Not measured here: the host entry (the trip), the processor, values longer than 512 bytes, hardware counters.
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VALUE_BYTES, FIELDS, UNIQUE = 512, 12, 2048
WIDE = "，"


def corpus_values(quoted_share, sep, seed=11):
    """UNIQUE values of exactly VALUE_BYTES bytes and FIELDS fields joined by sep; quoted_share of the fields are quoted and hold one `""`"""
    rng, out = random.Random(seed), []
    letters = "abcdefghijklmnopqrstuvwxyz0123456789_-./ "
    room = VALUE_BYTES - (FIELDS - 1) * len(sep)
    for _ in range(UNIQUE):
        cuts = sorted(rng.sample(range(1, room // 8), FIELDS - 1))
        sizes = [8 * (b - a) for a, b in zip([0] + cuts, cuts + [room // 8])]
        sizes[-1] += room - sum(sizes)
        fields = []
        for size in sizes:
            quoted = rng.random() < quoted_share
            text = "".join(rng.choice(letters) for _ in range(size))
            if quoted:
                at = rng.randint(1, size - 5)
                text = '"' + text[1:at] + '""' + text[at + 2:-1] + '"'
            fields.append(text.encode())
        value = sep.join(fields)
        assert len(value) == VALUE_BYTES
        out.append(value)
    return out


def spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs_ms": [float(x) for x in ms]}


def timed_alternating(torch, fns, warm=3, runs=5):
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [spread(m) for m in ms]


def rates(k, n, nbytes):
    k["GBps"] = nbytes / (k["median_ms"] / 1e3) / 1e9
    k["ps_per_byte"] = k["median_ms"] * 1e9 / nbytes
    k["ns_per_value"] = k["median_ms"] * 1e6 / n
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csv_bench.json"))
    args = ap.parse_args()
    import torch
    from helpers import csv_cases as cc
    from loongcollector_amd import csv_decode, delimiter
    dev = torch.device("cuda:0")
    n, W = args.n, 16
    stream = torch.cuda.current_stream().cuda_stream
    total = n * VALUE_BYTES
    assert total < 2 ** 31
    reps = (n + UNIQUE - 1) // UNIQUE
    d_off = torch.arange(0, (n + 1) * VALUE_BYTES, VALUE_BYTES, dtype=torch.int32, device=dev)
    plain_cfg, trim_cfg, wide_cfg = {"SplitSep": ","}, {"SplitSep": ",", "TrimLeadingSpace": True}, {"SplitSep": WIDE}
    p_plain, p_trim, p_wide = (csv_decode.Processor(**c) for c in (plain_cfg, trim_cfg, wide_cfg))
    dl = delimiter.GpuDelimiter(b",", b'"', "extend", 1)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    rows = torch.empty((n, W, 2), dtype=torch.int32, device=dev)
    s_st = torch.empty(n, dtype=torch.uint8, device=dev)
    s_nc = torch.empty(n, dtype=torch.int32, device=dev)
    s_sp = torch.empty((n, W, 2), dtype=torch.int32, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "n": n, "bytes": total, "value_bytes": VALUE_BYTES, "fields_per_value": FIELDS, "fields_kept": W,
              "timing": "HIP events, 3 warm-up launches, 5 timed launches per row, rows of one corpus alternating in the same run",
              "not_measured": ["lc_csv_host (the trip)", "lc_csv_process_logs_json (the processor)", "values longer than 512 bytes", "hardware counters"]}

    def resident(uniq):
        tile = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev)
        return torch.cat([tile.repeat(reps)[:total], torch.zeros(16, dtype=torch.uint8, device=dev)])

    def verify(config, uniq, what):
        torch.cuda.synchronize()
        got_rows, got_cnt, got_st = rows[:UNIQUE].cpu().numpy(), cnt[:UNIQUE].cpu().numpy(), st[:UNIQUE].cpu().numpy()
        for i, v in enumerate(uniq[:min(UNIQUE, n)]):
            code, fields = cc.fields_of(cc.result_text(config, v))
            assert code == 0 and got_st[i] == 0 and got_cnt[i] == len(fields) == FIELDS, (what, i)
            assert csv_decode.field_texts(v, got_rows[i], FIELDS) == fields, (what, i)

    for name, share in (("unquoted", 0.0), ("quoted_20_percent", 0.2)):
        uniq, uniq_wide = corpus_values(share, b","), corpus_values(share, WIDE.encode())
        d_data, d_wide = resident(uniq), resident(uniq_wide)
        d_copy = torch.empty_like(d_data)
        fns = {
            "csv_split_kernel_trim_off": lambda: csv_decode.read_device(p_plain, d_data, d_off, n, W, st, cnt, rows, stream=stream),
            "csv_split_kernel_trim_on": lambda: csv_decode.read_device(p_trim, d_data, d_off, n, W, st, cnt, rows, stream=stream),
            "csv_split_kernel_three_byte_separator": lambda: csv_decode.read_device(p_wide, d_wide, d_off, n, W, st, cnt, rows, stream=stream),
            "delim_split_kernel_same_bytes": lambda: dl.split_device(d_data, d_off, n, W, s_st, s_nc, s_sp, stream=stream),
            "device_to_device_copy": lambda: d_copy.copy_(d_data),
        }
        # what each csv_split_kernel row computes, checked against the model before it is timed
        for key, config, values in (("csv_split_kernel_trim_off", plain_cfg, uniq), ("csv_split_kernel_trim_on", trim_cfg, uniq),
                                    ("csv_split_kernel_three_byte_separator", wide_cfg, uniq_wide)):
            fns[key]()
            verify(config, values, name + " / " + key)
        timings = timed_alternating(torch, list(fns.values()))
        block = {k: rates(t, n, total) for k, t in zip(fns, timings)}
        base = block["delim_split_kernel_same_bytes"]
        margin = base["max_ms"] - base["min_ms"]
        for k in block:
            if k.startswith("csv_split_kernel"):
                block[k]["over_delim_split_time"] = block[k]["median_ms"] / base["median_ms"]
                block[k]["no_slower_than_delim_split_within_its_spread"] = bool(block[k]["median_ms"] <= base["median_ms"] + margin)
        base["note"] = "separator `,`, quote `\"`, 16 columns kept; its columns of the first value: %d, status %d" % (int(s_nc[0]), int(s_st[0]))
        base["spread_ms"] = margin
        result[name] = block
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({c: {k: round(v["median_ms"], 4) for k, v in result[c].items()} for c in ("unquoted", "quoted_20_percent")}))


if __name__ == "__main__":
    main()
