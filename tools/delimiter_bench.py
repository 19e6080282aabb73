"""Measures the delimiter parser beside the only way the library could parse such lines before: the regex path with the equivalent
pattern ([^,]*),([^,]*),... (ten groups).  Same lines, same box, same run.

    python tools/delimiter_bench.py [--lines N] [--out profiles/delimiter_bench.json]

* device-resident: N (default 1 Mi) lines of 512 bytes with 10 comma-separated columns made of the headline corpus' fields, quote-free
  and with 20 % of the fields quoted.  HIP events around one launch, 3 warm-up launches, then five timed ones: min / median / max,
  bytes/s, fraction of 8 TB/s.  Baseline: lc_regex_match_device on the quote-free corpus; ratio = baseline median / delimiter median, and
  the spread of the five baseline runs (max - min) is recorded next to it.
* in-agent: 1000-line groups through lc_delimiter_processor_process (and lc_processor_process for the baseline) from 1 and 16 threads,
  lines per second over a fixed number of groups per thread.
Prints one JSON document and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINE = 512
COLS = 10
HBM_BYTES_PER_S = 8e12


def make_lines(n_pool, quoted_fraction, seed):
    """n_pool distinct CSV lines of exactly LINE bytes: the space-separated fields of headline-corpus lines, commas inside them
    removed, ten columns per line, the last one padded"""
    from loongcollector_amd import corpus
    data, off, length = corpus.apache_batch(n_pool, "A", line_bytes=LINE, seed=seed)
    rng = np.random.Generator(np.random.MT19937(seed))
    out = np.empty((n_pool, LINE), np.uint8)
    for i in range(n_pool):
        words = bytes(data[off[i]:off[i] + length[i]]).replace(b",", b";").replace(b'"', b"'").split(b" ")
        fields = [b" ".join(words[k::COLS]) for k in range(COLS)]
        if quoted_fraction:
            fields = [b'"' + f[:-2] + b'"' if len(f) > 2 and rng.random() < quoted_fraction else f for f in fields]
        line = b",".join(fields)[:LINE]
        line = line + b"x" * (LINE - len(line))
        if line.count(b'"') % 2:                      # (the cut may have taken a closing quote)
            line = line.replace(b'"', b"'")
        out[i] = np.frombuffer(line, np.uint8)
    return out


def device_leg(n_lines, quoted_fraction, regex_too):
    import torch
    from loongcollector_amd import binding, delimiter
    dev = torch.device("cuda:0")
    pool = make_lines(8192, quoted_fraction, 20261016)
    idx = np.random.Generator(np.random.MT19937(1)).integers(0, len(pool), size=n_lines)
    data = pool[idx].reshape(-1)
    off = (np.arange(n_lines + 1, dtype=np.int64) * LINE).astype(np.int32)
    d_data = torch.from_numpy(data).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        med = statistics.median(ms)
        return {"ms_min": min(ms), "ms_median": med, "ms_max": max(ms), "bytes_per_s": n_lines * LINE / (med * 1e-3),
                "frac_of_8TBps": n_lines * LINE / (med * 1e-3) / HBM_BYTES_PER_S}

    W = COLS + 10
    dl = delimiter.GpuDelimiter(b",", b'"', "extend", COLS)
    d_st = torch.empty((n_lines,), dtype=torch.uint8, device=dev)
    d_nc = torch.empty((n_lines,), dtype=torch.int32, device=dev)
    d_sp = torch.empty((n_lines, W, 2), dtype=torch.int32, device=dev)
    res = {"lines": n_lines, "line_bytes": LINE, "columns": COLS, "quoted_fraction": quoted_fraction,
           "delimiter": timed(lambda: dl.split_device(d_data, d_off, n_lines, W, d_st, d_nc, d_sp, stream=stream))}
    assert int((d_st == 1).sum()) == n_lines and int(d_nc.min()) == COLS and int(d_nc.max()) == COLS, "the corpus did not split into ten columns"
    if regex_too:
        rx = binding.GpuRegex(",".join(["([^,]*)"] * COLS))
        d_caps = torch.empty((n_lines, 2 * rx.groups), dtype=torch.int32, device=dev)
        d_off_u = d_off  # (same offsets; the regex entry takes n + 1 offsets and sep_bytes = 0)
        res["regex_baseline"] = timed(lambda: rx.match_device(d_data, d_off_u, None, n_lines, d_caps, d_st, sep_bytes=0, stream=stream))
        assert int((d_st == 1).sum()) == n_lines, "the baseline pattern did not match every line"
        res["regex_engine"] = rx.info()["engine"]
        base = res["regex_baseline"]
        res["ratio_baseline_over_delimiter"] = base["ms_median"] / res["delimiter"]["ms_median"]
        res["baseline_spread_ms"] = base["ms_max"] - base["ms_min"]
    return res


def agent_leg(threads, groups_per_thread=200):
    from loongcollector_amd import delimiter
    from loongcollector_amd.processor import EventGroup, Processor
    pool = make_lines(1000, 0.0, 99)
    data = pool.reshape(-1)
    off = (np.arange(1000, dtype=np.uint32) * LINE)
    length = np.full(1000, LINE, np.uint32)
    keys = ["c%d" % i for i in range(COLS)]
    out = {}
    for name, make in (("delimiter", lambda: delimiter.DelimiterProcessor({"SourceKey": "content", "Separator": ",", "Keys": keys})),
                       ("regex_baseline", lambda: Processor({"SourceKey": "content", "Regex": ",".join(["([^,]*)"] * COLS), "Keys": keys}))):
        p = make()

        def worker():
            for _ in range(groups_per_thread):
                g = EventGroup.from_lines(data, off, length)
                p.process(g)
                g.close()

        worker()                                     # warm-up: tables, staging, streams of the first thread
        ts = [threading.Thread(target=worker) for _ in range(threads)]
        t0 = time.perf_counter()
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        dt = time.perf_counter() - t0
        out[name + "_lines_per_s"] = threads * groups_per_thread * 1000 / dt
    out["ratio_delimiter_over_baseline"] = out["delimiter_lines_per_s"] / out["regex_baseline_lines_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delimiter_bench.json"))
    args = ap.parse_args()
    doc = {"device_quote_free": device_leg(args.lines, 0.0, True), "device_20pct_quoted": device_leg(args.lines, 0.2, False),
           "in_agent_1_thread": agent_leg(1), "in_agent_16_threads": agent_leg(16)}
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
