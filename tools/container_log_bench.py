"""Measures the container stdout parser on an MI355X -> profiles/container_log_bench.json.

    python tools/container_log_bench.py [--n 1048576] [--out profiles/container_log_bench.json]

* kernels: 1 Mi lines of 512 bytes resident in device memory (4096 distinct lines, tiled); HIP events, 3 warm-up launches, 5 timed
  windows; every timing is reported with its spread.  Two kernels that are compared are timed in the SAME run, alternating.
    - clog_docker_kernel on lines whose "log" ends in `\\n"`, beside json_walk_kernel (W = 3) on the same bytes: the generic JSON
      parser is what a user has today.
    - clog_containerd_kernel beside delim_split_kernel splitting the same bytes on a blank (4 columns kept).
* the structural claim: the containerd kernel's time per line does not follow the content's length.  Offsets are 32-bit, so 1 Mi lines
  of 16 KiB (16 GiB) cannot be one batch: 96 Ki lines of 512 B and 96 Ki lines of 16 KiB + header, alternating in the same run, each
  window 20 launches.
* host: a 64 Ki slice of the 512-byte buffers through the __host__ instantiation of the routines, one thread, no per-line copy
  (tests/native/container_log_double.cpp cd_parse_resident).
* in-agent: 1000-event groups through lc_container_log_processor_process from 1 and 16 threads, both formats.
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
WORDS = ["request", "served", "in", "ms", "status", "ok", "user", "path=/api/v1/items", "GET", "POST", "cache", "miss", "retry", "n=3"]


def text_of(rng, size):
    out = []
    left = size
    while left > 0:
        w = rng.choice(WORDS)[:left]
        out.append(w)
        left -= len(w)
        if left > 0:
            out.append(" ")
            left -= 1
    return "".join(out)


def containerd_line(rng, i, size=LINE_BYTES):
    head = "2026-10-19T%02d:%02d:%02d.%09d+08:00 %s %s " % (rng.randrange(24), rng.randrange(60), rng.randrange(60), rng.randrange(10 ** 9),
                                                          "stderr" if i % 5 == 0 else "stdout", "P" if i % 4 == 0 else "F")
    line = (head + text_of(rng, size - len(head))).encode()
    assert len(line) == size
    return line


def docker_line(rng, i):
    tail = '\\n","stream":"%s","time":"2026-10-19T%02d:%02d:%02d.%09dZ"}' % ("stderr" if i % 5 == 0 else "stdout", rng.randrange(24), rng.randrange(60),
                                                                           rng.randrange(60), rng.randrange(10 ** 9))
    head = '{"log":"'
    line = (head + text_of(rng, LINE_BYTES - len(head) - len(tail)) + tail).encode()
    assert len(line) == LINE_BYTES
    return line


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


def resident(torch, dev, uniq, n, size):
    tile = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev)
    d_data = torch.cat([tile.repeat((n + len(uniq) - 1) // len(uniq))[:n * size], torch.zeros(16, dtype=torch.uint8, device=dev)])
    off = (np.arange(n + 1, dtype=np.int64) * size).astype(np.int32)
    return d_data, torch.from_numpy(off).to(dev), off


def clog_out(torch, dev, n):
    return {"status": torch.empty(n, dtype=torch.uint8, device=dev), "flags": torch.empty(n, dtype=torch.uint8, device=dev),
            "spans": torch.empty((n, 3, 2), dtype=torch.int32, device=dev), "rewrite_begin": torch.empty(n, dtype=torch.int32, device=dev)}


def rates(k, n, size):
    k["GBps"] = n * size / (k["median_ms"] / 1e3) / 1e9
    k["lines_per_s"] = n / (k["median_ms"] / 1e3)
    k["ns_per_line"] = k["median_ms"] * 1e6 / n
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "container_log_bench.json"))
    args = ap.parse_args()
    import torch
    from loongcollector_amd import container_log as clog, delimiter, json_parse
    from loongcollector_amd.processor import EventGroup
    from helpers import container_log_product as cp
    dev = torch.device("cuda:0")
    rng = random.Random(19)
    n = args.n
    stream = torch.cuda.current_stream().cuda_stream
    result = {"device": torch.cuda.get_device_name(0), "n": n, "line_bytes": LINE_BYTES}

    # ---- Docker beside the generic JSON parser, same bytes, same run
    d_uniq = [docker_line(rng, i) for i in range(4096)]
    d_data, d_off, _ = resident(torch, dev, d_uniq, n, LINE_BYTES)
    d_shadow = torch.empty_like(d_data)
    out = clog_out(torch, dev, n)
    W = 3
    j_status = torch.empty(n, dtype=torch.uint8, device=dev)
    j_nm = torch.empty(n, dtype=torch.int32, device=dev)
    j_err = torch.empty(n, dtype=torch.int32, device=dev)
    j_rec = torch.empty((n, W, 20), dtype=torch.uint8, device=dev)
    j_shadow = torch.empty_like(d_data)
    gj = json_parse.GpuJson()
    k, y = timed_alternating(torch, [lambda: clog.parse_device(clog.LC_CLOG_DOCKER, d_data, d_off, n, out, d_shadow, stream=stream),
                                     lambda: gj.walk_device(d_data, d_off, n, W, j_status, j_nm, j_err, j_rec, j_shadow, stream=stream)])
    st, fl = out["status"].cpu().numpy(), out["flags"].cpu().numpy()
    assert (st == 0).all() and ((fl & 12) == 4).all(), "the Docker kernel did not parse the corpus"
    assert (j_status.cpu().numpy() == json_parse.LC_JSON_OK).all() and (j_nm.cpu().numpy() == 3).all(), "the JSON kernel did not parse the corpus"
    result["clog_docker_kernel"] = rates(k, n, LINE_BYTES)
    result["json_walk_kernel_same_bytes"] = rates(y, n, LINE_BYTES)
    result["json_walk_kernel_same_bytes"]["note"] = "two launches per call (the second finds no deep line); W = 3"
    result["docker_speedup_over_json_walk_kernel"] = y["median_ms"] / k["median_ms"]
    docker_host = (d_data[:(1 << 16) * LINE_BYTES + 16].cpu().numpy(), st[:1 << 16].copy())
    del d_data, d_shadow, j_shadow, j_rec

    # ---- containerd beside the delimiter parser splitting the same bytes on a blank
    c_uniq = [containerd_line(rng, i) for i in range(4096)]
    c_data, c_off, _ = resident(torch, dev, c_uniq, n, LINE_BYTES)
    cols = 4
    dl = delimiter.GpuDelimiter(b" ", b" ", "extend", 1)   # (Quote == Separator: the plain path)
    s_st = torch.empty(n, dtype=torch.uint8, device=dev)
    s_nc = torch.empty(n, dtype=torch.int32, device=dev)
    s_sp = torch.empty((n, cols, 2), dtype=torch.int32, device=dev)
    k, y = timed_alternating(torch, [lambda: clog.parse_device(clog.LC_CLOG_CONTAINERD, c_data, c_off, n, out, None, stream=stream),
                                     lambda: dl.split_device(c_data, c_off, n, cols, s_st, s_nc, s_sp, stream=stream)])
    st = out["status"].cpu().numpy()
    assert (st == 0).all() and int(((out["flags"].cpu().numpy() & 2) != 0).sum()) == n // 4, "the containerd kernel did not parse the corpus"
    assert int(s_nc.cpu().numpy()[0]) >= 4, "the delimiter kernel did not split the corpus"
    result["clog_containerd_kernel"] = rates(k, n, LINE_BYTES)
    result["delim_split_kernel_same_bytes"] = rates(y, n, LINE_BYTES)
    result["delim_split_kernel_same_bytes"]["note"] = "splits every blank of the line, keeps 4 columns"
    result["containerd_speedup_over_delim_split_kernel"] = y["median_ms"] / k["median_ms"]
    containerd_host = c_data[:(1 << 16) * LINE_BYTES + 16].cpu().numpy()

    # ---- the structural claim: time per line against content length, same run, alternating
    m = min(n, 96 * 1024)
    big = 16384 + 64
    b_uniq = [containerd_line(rng, i, big) for i in range(256)]
    b_data, b_off, _ = resident(torch, dev, b_uniq, m, big)
    out_m = clog_out(torch, dev, m)
    s_, b_ = timed_alternating(torch, [lambda: clog.parse_device(clog.LC_CLOG_CONTAINERD, c_data, c_off, m, out_m, None, stream=stream),
                                       lambda: clog.parse_device(clog.LC_CLOG_CONTAINERD, b_data, b_off, m, out_m, None, stream=stream)], reps=20)
    assert (out_m["status"].cpu().numpy() == 0).all()
    spread_ms = max(s_["max_ms"] - s_["min_ms"], b_["max_ms"] - b_["min_ms"])
    result["containerd_content_length"] = {
        "lines": m, "launches_per_window": 20, "lines_512B": rates(s_, m, LINE_BYTES), "lines_16KiB": rates(b_, m, big),
        "difference_ms": b_["median_ms"] - s_["median_ms"], "five_run_spread_ms": spread_ms,
        "difference_within_spread": abs(b_["median_ms"] - s_["median_ms"]) <= spread_ms,
        "note": "offsets are 32-bit: 1 Mi lines of 16 KiB cannot be one batch.  A line's row starts 16 KiB apart instead of 512 B apart: "
                "the same number of 64-byte stage loads per line (stage 0 and the prefetch of stage 1), from as many more DRAM pages"}
    del b_data

    # ---- the routines on one host thread over a 64 Ki slice of the resident buffers, ONE native call each
    L = cp.double()
    h = min(n, 1 << 16)
    off_h = (np.arange(h + 1, dtype=np.int64) * LINE_BYTES).astype(np.int32)
    res = {"status": np.zeros(h, np.uint8), "flags": np.zeros(h, np.uint8), "spans": np.zeros((h, 3, 2), np.int32), "rewrite_begin": np.zeros(h, np.int32)}
    o = clog.LcClogOut(*(res[x].ctypes.data for x in clog.OUT_KEYS))
    result["host_routine_one_thread"] = {}
    for name, fmt, data in (("containerd", 1, containerd_host), ("docker", 2, docker_host[0])):
        shadow = np.zeros(len(data), np.uint8)
        native = []
        for _ in range(5):
            t0 = time.perf_counter()
            L.cd_parse_resident(fmt, data.ctypes.data, off_h.ctypes.data, h, ctypes.byref(o), shadow.ctypes.data)
            native.append((time.perf_counter() - t0) * 1e3)
        assert (res["status"] == 0).all(), "the host routine and the kernel disagree"
        r = rates(spread(native), h, LINE_BYTES)
        r["what"] = "the routine of clog_vm.hpp compiled for the host over the resident buffer, one thread, no per-line copy (g++ -O2)"
        result["host_routine_one_thread"][name] = r
    result["kernel_over_host_routine"] = {
        "containerd": result["clog_containerd_kernel"]["lines_per_s"] / result["host_routine_one_thread"]["containerd"]["lines_per_s"],
        "docker": result["clog_docker_kernel"]["lines_per_s"] / result["host_routine_one_thread"]["docker"]["lines_per_s"]}

    # ---- in-agent: 1000-event groups
    result["in_agent"] = {}
    for name, fmt, uniq in (("containerd", "1", c_uniq), ("docker", "2", d_uniq)):
        groups_json = json.dumps({"metadata": {"container.type": fmt},
                                  "events": [{"contents": {"content": v.decode()}, "timestamp": 1, "type": 1} for v in uniq[:1000]]})
        for threads in (1, 16):
            per = 20
            runs = []
            for _ in range(3):
                procs = [clog.ContainerLogProcessor({}) for _ in range(threads)]
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
                runs.append(threads * per * 1000 / (time.perf_counter() - t0))
            result["in_agent"]["%s_threads_%d" % (name, threads)] = {
                "events_per_s_median": float(np.median(runs)), "events_per_s_runs": [float(r) for r in runs], "group_events": 1000,
                "MBps_median": float(np.median(runs)) * LINE_BYTES / 1e6,
                "note": "warm-up groups run on the main thread; each worker thread pays its own first-trip allocation inside the timing"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"docker_ms": result["clog_docker_kernel"]["median_ms"], "json_ms": result["json_walk_kernel_same_bytes"]["median_ms"],
                      "containerd_ms": result["clog_containerd_kernel"]["median_ms"], "delim_ms": result["delim_split_kernel_same_bytes"]["median_ms"],
                      "content_length": {k: v for k, v in result["containerd_content_length"].items() if k.endswith("_ms") or k.endswith("spread")}}))


if __name__ == "__main__":
    main()
