"""Measures the key-value splitter on an MI355X -> profiles/kv_bench.json.

    python tools/kv_bench.py [--n 1048576] [--out profiles/kv_bench.json]

* the corpus: 1 Mi values of exactly 512 bytes, 10 pairs each (`key=value`, blank-delimited; 8192 distinct values, tiled), resident in
  device memory, in two forms: quote-free, and with 20 % of the pair values quoted (`key="text with blanks"`).
* kernels: HIP events, 3 warm-up launches, 5 timed launches, min / median / max; everything that is compared is timed in the SAME run,
  alternating, on the same bytes:
    - kv_split_kernel (W = 16): the no-quote and the long-quote form on the quote-free corpus, the one-byte-quote form on both corpora,
    - a device-to-device copy of the corpus,
    - delim_split_kernel with the delimiter (a blank) as its separator, 16 columns kept: the figure to beat is its time per byte, the
      margin the spread of its five runs.
* the first 8192 values of every kernel row are compared with tests/helpers/kv_model.py before anything is written.
Not measured here: the host entry, the processor, rocprofv3 traces and counters.
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

VALUE_BYTES, PAIRS, UNIQUE = 512, 10, 8192


def corpus_values(quoted_share, seed=11):
    """UNIQUE values of exactly VALUE_BYTES bytes and PAIRS pairs; quoted_share of the pair values are quoted and hold blanks"""
    rng, out = random.Random(seed), []
    letters = "abcdefghijklmnopqrstuvwxyz0123456789_-./"
    for _ in range(UNIQUE):
        room = VALUE_BYTES - (PAIRS - 1)
        cuts = sorted(rng.sample(range(1, room // 8), PAIRS - 1))
        sizes = [8 * (b - a) for a, b in zip([0] + cuts, cuts + [room // 8])]
        sizes[-1] += room - sum(sizes)
        pairs = []
        for size in sizes:
            quoted = rng.random() < quoted_share
            klen = rng.randint(2, min(12, size - (5 if quoted else 4)))
            key = "".join(rng.choice(letters[:26]) for _ in range(klen))
            vlen = size - klen - 1
            if quoted:
                text = "".join(rng.choice(letters + "    ") for _ in range(vlen - 2))
                text = "x" + text[1:-1] + "x"  # (no blank or backslash right at the quotes)
                pairs.append(key + '="' + text + '"')
            else:
                pairs.append(key + "=" + "".join(rng.choice(letters) for _ in range(vlen)))
        value = " ".join(pairs).encode()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_bench.json"))
    args = ap.parse_args()
    import torch
    from helpers import kv_cases as kc
    from loongcollector_amd import delimiter, kvsplit
    dev = torch.device("cuda:0")
    n, W = args.n, 16
    stream = torch.cuda.current_stream().cuda_stream
    total = n * VALUE_BYTES
    assert total < 2 ** 31
    reps = (n + UNIQUE - 1) // UNIQUE
    d_off = torch.arange(0, (n + 1) * VALUE_BYTES, VALUE_BYTES, dtype=torch.int32, device=dev)
    plain_cfg = {"Delimiter": " ", "Separator": "="}
    quote_cfg = dict(plain_cfg, Quote="\"")
    long_cfg = dict(plain_cfg, Quote="\"\"")
    p_plain, p_quote, p_long = kvsplit.Processor(**plain_cfg), kvsplit.Processor(**quote_cfg), kvsplit.Processor(**long_cfg)
    dl = delimiter.GpuDelimiter(b" ", b" ", "extend", 1)  # (Quote == Separator: its plain path, every blank splits)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    rows = torch.empty((n, W, 4), dtype=torch.int32, device=dev)
    s_st = torch.empty(n, dtype=torch.uint8, device=dev)
    s_nc = torch.empty(n, dtype=torch.int32, device=dev)
    s_sp = torch.empty((n, W, 2), dtype=torch.int32, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "n": n, "bytes": total, "value_bytes": VALUE_BYTES, "pairs_per_value": PAIRS, "pairs_kept": W,
              "timing": "HIP events, 3 warm-up launches, 5 timed launches per row, rows of one corpus alternating in the same run",
              "not_measured": ["lc_kvsplit_host (the trip)", "lc_kvsplit_process_logs_json", "rocprofv3 kernel trace", "hardware counters"]}

    def verify(proc, config, uniq, what):
        proc_rows, proc_cnt, proc_st = rows[:UNIQUE].cpu().numpy(), cnt[:UNIQUE].cpu().numpy(), st[:UNIQUE].cpu().numpy()
        for i, v in enumerate(uniq[:min(UNIQUE, n)]):
            want = kc.rows_of(kc.rows_text(config, v))
            assert proc_st[i] == 0 and proc_cnt[i] == len(want) and np.array_equal(proc_rows[i][:len(want)], want), (what, i)

    for name, share in (("quote_free", 0.0), ("quoted_20_percent", 0.2)):
        uniq = corpus_values(share)
        tile = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev)
        d_data = torch.cat([tile.repeat(reps)[:total], torch.zeros(16, dtype=torch.uint8, device=dev)])
        d_copy = torch.empty_like(d_data)
        fns = {
            "kv_split_kernel_quote": lambda: kvsplit.split_device(p_quote, d_data, d_off, n, W, st, cnt, rows, stream=stream),
            "device_to_device_copy": lambda: d_copy.copy_(d_data),
            "delim_split_kernel_same_bytes": lambda: dl.split_device(d_data, d_off, n, W, s_st, s_nc, s_sp, stream=stream),
        }
        if share == 0.0:
            # (the long-quote form on bytes that hold no quote: what the notes of the one-byte form save over comparing bytes)
            fns = dict({"kv_split_kernel_no_quote": lambda: kvsplit.split_device(p_plain, d_data, d_off, n, W, st, cnt, rows, stream=stream),
                        "kv_split_kernel_long_quote": lambda: kvsplit.split_device(p_long, d_data, d_off, n, W, st, cnt, rows, stream=stream)}, **fns)
        # what each kernel row computes, checked against the model before it is timed
        if share == 0.0:
            fns["kv_split_kernel_no_quote"]()
            torch.cuda.synchronize()
            verify(p_plain, plain_cfg, uniq, name + " / no quote")
            fns["kv_split_kernel_long_quote"]()
            torch.cuda.synchronize()
            verify(p_long, long_cfg, uniq, name + " / long quote")
        fns["kv_split_kernel_quote"]()
        torch.cuda.synchronize()
        verify(p_quote, quote_cfg, uniq, name + " / quote")
        assert int(cnt.min()) == PAIRS and int(cnt.max()) == PAIRS, "every value holds 10 pairs"
        timings = timed_alternating(torch, list(fns.values()))
        assert int(s_nc[0]) >= PAIRS, "the delimiter kernel did not split the corpus"
        block = {k: rates(t, n, total) for k, t in zip(fns, timings)}
        base = block["delim_split_kernel_same_bytes"]
        margin = base["max_ms"] - base["min_ms"]
        for k in block:
            if k.startswith("kv_split_kernel"):
                block[k]["over_delim_split_time"] = block[k]["median_ms"] / base["median_ms"]
                block[k]["no_slower_than_delim_split_within_its_spread"] = bool(block[k]["median_ms"] <= base["median_ms"] + margin)
        block["delim_split_kernel_same_bytes"]["note"] = "the delimiter (a blank) as its separator, plain path, 16 columns kept"
        block["delim_split_kernel_same_bytes"]["spread_ms"] = margin
        result[name] = block
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({c: {k: round(v["median_ms"], 4) for k, v in result[c].items()} for c in ("quote_free", "quoted_20_percent")}))


if __name__ == "__main__":
    main()
