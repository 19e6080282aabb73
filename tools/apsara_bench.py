"""Measures the Apsara parser on an MI355X -> profiles/apsara_bench.json.

    python tools/apsara_bench.py [--n 1048576] [--out profiles/apsara_bench.json]

* kernel: 1 Mi lines of 512 bytes resident in device memory -- date form, four base fields, key:value pairs filling the rest (4096
  distinct lines, tiled); HIP events, 3 warm-up launches, 5 timed; every timing is reported with its spread.
* yardstick, in the SAME run: delim_split_kernel splitting the same bytes on TAB (the plain path).  It walks the same bytes through the
  same source (wave_tile_source.hpp) and stores one (begin, end) per column.
* host: a 64 Ki slice of the same buffer through the __host__ instantiation of the routine, one thread, no per-line copy
  (tests/native/apsara_double.cpp ad_parse_resident).
* in-agent: 1000-event groups through lc_apsara_processor_process from 1 and 16 threads.
"""
import argparse
import ctypes
import json
import os
import random
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LINE_BYTES = 512


def make_line(rng, i):
    head = "[2026-10-17 %02d:%02d:%02d.%06d]\t[%s]\t[%d]\t[src/core/worker_%d.cpp:%d]" % (
        rng.randrange(24), rng.randrange(60), rng.randrange(60), rng.randrange(10 ** 6), rng.choice(["INFO", "WARNING", "ERROR", "DEBUG"]),
        rng.randrange(10 ** 6), i % 97, rng.randrange(5000))
    parts = [head]
    size = len(head)
    k = 0
    while True:
        piece = "\tkey%d:%s" % (k, "v" * rng.randrange(1, 12))
        if size + len(piece) > LINE_BYTES - 8:
            break
        parts.append(piece)
        size += len(piece)
        k += 1
    last = "\tpad:"
    parts.append(last + "p" * (LINE_BYTES - size - len(last)))
    line = "".join(parts).encode()
    assert len(line) == LINE_BYTES
    return line, k + 1


def spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs_ms": [float(x) for x in ms]}


def timed(torch, fn, warm=3, runs=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "apsara_bench.json"))
    args = ap.parse_args()
    import torch
    from loongcollector_amd import apsara, delimiter
    from loongcollector_amd.processor import EventGroup
    from helpers import apsara_double as ad
    dev = torch.device("cuda:0")
    rng = random.Random(11)
    n = args.n
    made = [make_line(rng, i) for i in range(4096)]
    uniq = [m[0] for m in made]
    W = max(m[1] for m in made)
    tile = np.frombuffer(b"".join(uniq), np.uint8)
    data = np.concatenate([np.tile(tile, (n + 4095) // 4096)[:n * LINE_BYTES], np.zeros(16, np.uint8)])
    off = (np.arange(n + 1, dtype=np.int64) * LINE_BYTES).astype(np.int32)
    d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    result = {"device": torch.cuda.get_device_name(0), "n": n, "line_bytes": LINE_BYTES, "pairs_per_line_max": W}
    d_out = {"status": torch.empty(n, dtype=torch.uint8, device=dev), "secs": torch.empty(n, dtype=torch.int64, device=dev),
             "nanos": torch.empty(n, dtype=torch.int32, device=dev), "base": torch.empty((n, 4, 2), dtype=torch.int32, device=dev),
             "npairs": torch.empty(n, dtype=torch.int32, device=dev), "pairs": torch.empty((n, W, 3), dtype=torch.int32, device=dev)}
    k = timed(torch, lambda: apsara.parse_device(d_data, d_off, n, W, d_out, stream=stream))
    st, npairs = d_out["status"].cpu().numpy(), d_out["npairs"].cpu().numpy()
    assert (st == 5).all() and (npairs[:4096] == np.array([m[1] for m in made])).all(), "the kernel did not parse the corpus"
    k["GBps"] = n * LINE_BYTES / (k["median_ms"] / 1e3) / 1e9
    k["lines_per_s"] = n / (k["median_ms"] / 1e3)
    result["apsara_parse_kernel"] = k
    # the yardstick: the same bytes split on TAB, room for every column
    cols = W + 5
    dl = delimiter.GpuDelimiter(b"\t", b"\t", "extend", 1)   # (Quote == Separator: the plain path)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_nc = torch.empty(n, dtype=torch.int32, device=dev)
    d_sp = torch.empty((n, cols, 2), dtype=torch.int32, device=dev)
    y = timed(torch, lambda: dl.split_device(d_data, d_off, n, cols, d_st, d_nc, d_sp, stream=stream))
    assert int(d_nc.cpu().numpy()[0]) == made[0][1] + 4, "the delimiter kernel did not split the corpus"
    y["GBps"] = n * LINE_BYTES / (y["median_ms"] / 1e3) / 1e9
    result["delim_split_kernel_same_bytes"] = y
    result["ratio_to_delim_split_kernel"] = k["median_ms"] / y["median_ms"]
    # the same routine on one host thread: apsaraParseLine's __host__ instantiation over a 64 Ki slice of the resident buffer, no copy
    # and no allocation per line (tests/native/apsara_double.cpp ad_parse_resident), ONE native call
    L = ad.double()
    m = min(n, 1 << 16)
    res = {"status": np.zeros(m, np.uint8), "secs": np.zeros(m, np.int64), "nanos": np.zeros(m, np.uint32), "base": np.zeros((m, 4, 2), np.int32),
           "npairs": np.zeros(m, np.uint32), "pairs": np.zeros((m, W, 3), np.int32)}
    o = apsara.LcApsaraOut(*(res[x].ctypes.data for x in apsara.OUT_KEYS))
    native = []
    for _ in range(5):
        t0 = time.perf_counter()
        L.ad_parse_resident(data.ctypes.data, off.ctypes.data, m, W, ctypes.byref(o))
        native.append((time.perf_counter() - t0) * 1e3)
    assert (res["status"] == 5).all() and (res["npairs"] == npairs[:m]).all(), "the host routine and the kernel disagree"
    h = spread(native)
    h["lines"] = m
    h["GBps"] = m * LINE_BYTES / (h["median_ms"] / 1e3) / 1e9
    h["what"] = "apsaraParseLine compiled for the host over the resident buffer, one thread, no per-line copy (g++ -O2)"
    result["host_routine_one_thread"] = h
    result["kernel_over_host_routine"] = k["GBps"] / h["GBps"]
    # in-agent: 1000-event groups
    groups_json = json.dumps({"events": [{"contents": {"content": v.decode()}, "timestamp": 1, "type": 1} for v in uniq[:1000]]})
    result["in_agent"] = {}
    for threads in (1, 16):
        per = 20
        rates = []
        for _ in range(3):
            procs = [apsara.ApsaraProcessor({"SourceKey": "content"}) for _ in range(threads)]
            for p in procs:
                p.set_discard(False)
            groups = [[EventGroup(groups_json) for _ in range(per)] for _ in range(threads)]

            def work(p, gs):
                for g in gs:
                    p.process(g)
            for p in procs:   # warm-up: the main thread's staging
                p.process(EventGroup(groups_json))
            ths = [threading.Thread(target=work, args=(p, gs)) for p, gs in zip(procs, groups)]
            t0 = time.perf_counter()
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            rates.append(threads * per * 1000 / (time.perf_counter() - t0))
        result["in_agent"]["threads_%d" % threads] = {
            "events_per_s_median": float(np.median(rates)), "events_per_s_runs": [float(r) for r in rates], "group_events": 1000,
            "MBps_median": float(np.median(rates)) * LINE_BYTES / 1e6,
            "note": "warm-up groups run on the main thread; each worker thread pays its own first-trip allocation inside the timing"}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"apsara_ms": k["median_ms"], "delim_ms": y["median_ms"], "ratio": result["ratio_to_delim_split_kernel"]}))


if __name__ == "__main__":
    main()
