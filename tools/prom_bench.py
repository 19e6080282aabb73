"""Measures the Prometheus text-line parser on an MI355X -> profiles/prom_bench.json.

    python tools/prom_bench.py [--n 1048576] [--out profiles/prom_bench.json]

* the corpus: 1 Mi exposition lines (loongcollector_amd.corpus.prom_exposition_lines: names of 10 to 40 bytes, 0 to 8 labels, values
  drawn ONLY from the forms the device converts; 8192 distinct lines, tiled) resident in device memory.
* kernels: HIP events, 3 warm-up launches, 5 timed windows, every timing with its spread; the kernels that are compared are timed in
  the SAME run, alternating.
    - prom_parse_kernel (W = 8) per launch, beside
    - delim_split_kernel splitting the same bytes on a blank (4 columns kept): the project's yardstick for "one walk over these bytes".
* host: a 64 Ki slice of the same buffer through the __host__ instantiation of the routine, one thread, no per-line copy
  (tests/native/prom_double.cpp pd_parse_resident).
* deferral: 64 Ki lines through lc_prom_parse_host (upload, kernel, download, host finish), the clean corpus and the corpus with 5 % of
  the values left to the host, alternating in the same run.
* in-agent: 1000-event groups through lc_prom_processor_process from 1 and 16 threads.
"""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(ms, per=1):
    ms = [m / per for m in ms]
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs_ms": [float(x) for x in ms]}


def timed_alternating(torch, fns, warm=3, runs=5, reps=1):
    """every function of fns once per round, `runs` rounds: -> one spread per function (milliseconds per call)"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [spread(m, reps) for m in ms]


def rates(k, n, nbytes):
    k["GBps"] = nbytes / (k["median_ms"] / 1e3) / 1e9
    k["lines_per_s"] = n / (k["median_ms"] / 1e3)
    k["ns_per_line"] = k["median_ms"] * 1e6 / n
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prom_bench.json"))
    args = ap.parse_args()
    import torch
    from loongcollector_amd import corpus, delimiter, prom
    from helpers import prom_product as pp
    dev = torch.device("cuda:0")
    n, W = args.n, 8
    stream = torch.cuda.current_stream().cuda_stream
    uniq = corpus.prom_exposition_lines(8192)
    sizes = np.array([len(v) for v in uniq], np.int64)
    reps = (n + len(uniq) - 1) // len(uniq)
    lens = np.tile(sizes, reps)[:n]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[n])
    assert total < 2 ** 31
    tile = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev)
    d_data = torch.cat([tile.repeat(reps)[:total], torch.zeros(16, dtype=torch.uint8, device=dev)])
    d_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "n": n, "bytes": total, "mean_line_bytes": total / n, "labels_kept": W,
              "corpus": "corpus.prom_exposition_lines(8192), tiled; every value of a device-path form"}

    # ---- the kernel beside the delimiter kernel, same bytes, same run
    d_out = {k: torch.empty(s, dtype={np.uint8: torch.uint8, np.int32: torch.int32, np.uint64: torch.int64, np.int64: torch.int64, np.uint32: torch.int32}[t],
                            device=dev) for k, (s, t) in prom.out_shapes(n, W).items()}
    cols = 4
    dl = delimiter.GpuDelimiter(b" ", b" ", "extend", 1)   # (Quote == Separator: the plain path)
    s_st = torch.empty(n, dtype=torch.uint8, device=dev)
    s_nc = torch.empty(n, dtype=torch.int32, device=dev)
    s_sp = torch.empty((n, cols, 2), dtype=torch.int32, device=dev)
    k, y = timed_alternating(torch, [lambda: prom.parse_device(True, d_data, d_off, n, d_out, W, stream=stream),
                                     lambda: dl.split_device(d_data, d_off, n, cols, s_st, s_nc, s_sp, stream=stream)])
    st, fl = d_out["status"].cpu().numpy(), d_out["flags"].cpu().numpy()
    assert (st == 0).all() and not (fl & 3).any(), "the corpus must defer 0 tokens and fail 0 lines"
    assert int(s_nc.cpu().numpy()[0]) >= 2, "the delimiter kernel did not split the corpus"
    result["prom_parse_kernel"] = rates(k, n, total)
    result["delim_split_kernel_same_bytes"] = rates(y, n, total)
    result["delim_split_kernel_same_bytes"]["note"] = "splits every blank of the line, keeps 4 columns"
    result["prom_over_delim_split_time"] = k["median_ms"] / y["median_ms"]

    # ---- the routine on one host thread over a 64 Ki slice of the resident buffer, ONE native call
    L = pp.double()
    h = min(n, 1 << 16)
    host_data = d_data[:int(off[h]) + 16].cpu().numpy()
    off_h = off[:h + 1].astype(np.int32)
    res = pp.out_arrays(h, W)
    o = pp.LcPromOut(*(res[x].ctypes.data for x in pp.OUT_KEYS))
    native = []
    for _ in range(5):
        t0 = time.perf_counter()
        L.pd_parse_resident(1, host_data.ctypes.data, off_h.ctypes.data, h, ctypes.byref(o), W, 0)
        native.append((time.perf_counter() - t0) * 1e3)
    assert (res["status"] == 0).all() and np.array_equal(res["value"], d_out["value"][:h].cpu().numpy().view(np.uint64)), "the host routine and the kernel disagree"
    r = rates(spread(native), h, int(off[h]))
    r["what"] = "promParseLine of prom_vm.hpp compiled for the host over the resident buffer, one thread, no per-line copy (g++ -O2)"
    result["host_routine_one_thread"] = r
    result["kernel_over_host_routine"] = result["prom_parse_kernel"]["lines_per_s"] / r["lines_per_s"]

    # ---- what deferral costs: the host entry on the clean corpus and with 5 % of the values left to the host, same run, alternating
    m = min(n, 1 << 16)
    clean = corpus.prom_exposition_lines(m)
    mixed = corpus.prom_exposition_lines(m, deferred=0.05)
    wall = {"clean": [], "deferred_5_percent": []}
    deferred = {}
    for _ in range(2):  # warm-up: the thread's staging
        prom.parse_host(clean[:4096], True, W)
    for _ in range(5):
        for name, lines in (("clean", clean), ("deferred_5_percent", mixed)):
            t0 = time.perf_counter()
            got = prom.parse_host(lines, True, W)
            wall[name].append((time.perf_counter() - t0) * 1e3)
            deferred[name] = got["deferred"]
    assert deferred["clean"] == 0 and deferred["deferred_5_percent"] > m // 30
    result["host_entry"] = {name: dict(rates(spread(ms), m, sum(len(v) for v in (clean if name == "clean" else mixed))), deferred_tokens=deferred[name])
                            for name, ms in wall.items()}
    result["host_entry"]["note"] = ("wall time of loongcollector_amd.prom.parse_host (packing in Python, upload, kernel, download, host finish); "
                                    "the difference of the two rows is what finishing the deferred tokens with strtod costs")
    result["host_entry"]["deferral_cost_ms"] = result["host_entry"]["deferred_5_percent"]["median_ms"] - result["host_entry"]["clean"]["median_ms"]

    # ---- in-agent: 1000-event groups
    result["in_agent"] = {}
    group_lines = corpus.prom_exposition_lines(1000, seed=5)
    group_bytes = sum(len(v) for v in group_lines)
    for threads in (1, 16):
        per = 20
        runs = []
        for _ in range(3):
            procs = [prom.PromProcessor({"job_name": "bench"}) for _ in range(threads)]
            groups = [[prom.RawGroup(group_lines, 1700000000123) for _ in range(per)] for _ in range(threads)]

            def work(p, gs):
                for g in gs:
                    p.process(g)
            for p in procs:   # warm-up: the main thread's staging
                p.process(prom.RawGroup(group_lines, 1700000000123))
            ths = [threading.Thread(target=work, args=(p, gs)) for p, gs in zip(procs, groups)]
            t0 = time.perf_counter()
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            runs.append(threads * per * 1000 / (time.perf_counter() - t0))
        result["in_agent"]["threads_%d" % threads] = {
            "events_per_s_median": float(np.median(runs)), "events_per_s_runs": [float(r) for r in runs], "group_events": 1000,
            "MBps_median": float(np.median(runs)) * group_bytes / 1000 / 1e6,
            "note": "warm-up groups run on the main thread; each worker thread pays its own first-trip allocation inside the timing"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"prom_ms": result["prom_parse_kernel"]["median_ms"], "delim_ms": result["delim_split_kernel_same_bytes"]["median_ms"],
                      "host_routine_ms_64Ki": result["host_routine_one_thread"]["median_ms"],
                      "host_entry_clean_ms": result["host_entry"]["clean"]["median_ms"],
                      "host_entry_deferred_ms": result["host_entry"]["deferred_5_percent"]["median_ms"],
                      "in_agent_events_per_s": {k: v["events_per_s_median"] for k, v in result["in_agent"].items()}}))


if __name__ == "__main__":
    main()
