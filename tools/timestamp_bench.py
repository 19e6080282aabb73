"""Measures the timestamp parser on an MI355X -> profiles/timestamp_bench.json.

    python tools/timestamp_bench.py [--n 1048576] [--out profiles/timestamp_bench.json]

* kernel: 1 Mi values of "%Y-%m-%d %H:%M:%S.%f" and of the nginx form "%d/%b/%Y:%H:%M:%S %z", resident in device memory; HIP events,
  3 warm-up launches, 5 timed; every timing is reported with its spread.
* host: the same values through the __host__ instantiation of the routine (tests/native/timestamp_double.cpp), one thread.
* in-agent: 1000-event groups through lc_timestamp_processor_process from 1 and 16 threads.
* fused: regex parse + timestamp on one stream against the regex parse alone on the same lines: the ADDED time.
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

MONTHS = ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"]


def values_for(fmt, n, rng):
    out, sec = [], 1703400000
    for _ in range(n):
        sec += rng.choice([0, 0, 0, 1])
        t = time.gmtime(sec)
        if fmt.endswith("%f"):
            out.append(("%04d-%02d-%02d %02d:%02d:%02d.%06d" % (t.tm_year, t.tm_mon, t.tm_mday, t.tm_hour, t.tm_min, t.tm_sec, rng.randrange(10 ** 6))).encode())
        else:
            out.append(("%02d/%s/%04d:%02d:%02d:%02d +0800" % (t.tm_mday, MONTHS[t.tm_mon - 1], t.tm_year, t.tm_hour, t.tm_min, t.tm_sec)).encode())
    return out


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timestamp_bench.json"))
    args = ap.parse_args()
    import torch
    from loongcollector_amd import binding, corpus, timestamp
    from loongcollector_amd.processor import EventGroup
    from helpers.timestamp_double import Format
    dev = torch.device("cuda:0")
    rng = random.Random(5)
    result = {"device": torch.cuda.get_device_name(0), "n": args.n, "kernel": {}, "host_one_thread": {}, "in_agent": {}, "fused": {}}
    stream = torch.cuda.current_stream().cuda_stream
    for fmt in ("%Y-%m-%d %H:%M:%S.%f", "%d/%b/%Y:%H:%M:%S %z"):
        vals = values_for(fmt, args.n, rng)
        lens = np.array([len(v) for v in vals], np.int32)
        blob = b"".join(vals)
        data = np.frombuffer(blob + b"\0" * (16 - len(blob) % 16), np.uint8).copy()
        off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int32)
        spans = np.stack([np.zeros(args.n, np.int32), lens], axis=1).copy()
        d_data, d_off, d_spans = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(spans).to(dev)
        t = timestamp.GpuStrptime(fmt)
        out = t.device_outputs(args.n, dev)
        k = timed(torch, lambda: t.parse_spans_device(d_data, d_off, d_spans, args.n, out, stream=stream))
        k["values_per_s"] = args.n / (k["median_ms"] / 1e3)
        k["value_bytes"] = int(lens.sum())
        result["kernel"][fmt] = k
        # the same routine on one host thread: a 64 Ki slice through the CPU double's lc_strptime_parse_host (tests/native/
        # timestamp_double.cpp: strptimeRun per value plus a copy of each value and the same_as_prev compare), ONE native call
        f = Format(fmt)
        m = min(args.n, 1 << 16)
        L = f.L
        ptrs = (data.ctypes.data + off[:m].astype(np.int64)).astype(np.uint64)
        hl = lens[:m].astype(np.uint32)
        res = {"status": np.zeros(m, np.uint8), "secs": np.zeros(m, np.int64), "nanos": np.zeros(m, np.uint32), "matched": np.zeros(m, np.int32),
               "frac_len": np.zeros(m, np.int32), "same_as_prev": np.zeros(m, np.uint8)}
        o = timestamp.LcTsOut(*(res[x].ctypes.data for x in ("status", "secs", "nanos", "matched", "frac_len", "same_as_prev")))
        native = []
        for _ in range(5):
            t0 = time.perf_counter()
            L.lc_strptime_parse_host(f.h, ptrs.ctypes.data, hl.ctypes.data, m, ctypes.byref(o))
            native.append((time.perf_counter() - t0) * 1e3)
        h = spread(native)
        h["values"] = m
        h["values_per_s"] = m / (h["median_ms"] / 1e3)
        result["host_one_thread"][fmt] = h
        # in-agent: 1000-event groups
        cfg = {"SourceKey": "time", "SourceFormat": fmt, "SourceTimezone": "GMT+00:00"}
        groups_json = json.dumps({"events": [{"contents": {"time": v.decode()}, "timestamp": 1, "type": 1} for v in vals[:1000]]})
        for threads in (1, 16):
            per = 40
            rates = []
            for _ in range(3):
                procs = [timestamp.TimestampProcessor(cfg) for _ in range(threads)]
                for p in procs:
                    p.set_discard(False)
                groups = [[EventGroup(groups_json) for _ in range(per)] for _ in range(threads)]

                def work(p, gs):
                    for g in gs:
                        p.process(g)
                for p, gs in zip(procs, groups):   # warm-up: the threads' staging
                    p.process(EventGroup(groups_json))
                ths = [threading.Thread(target=work, args=(p, gs)) for p, gs in zip(procs, groups)]
                t0 = time.perf_counter()
                for th in ths:
                    th.start()
                for th in ths:
                    th.join()
                rates.append(threads * per * 1000 / (time.perf_counter() - t0))
            result["in_agent"].setdefault(fmt, {})["threads_%d" % threads] = {
                "events_per_s_median": float(np.median(rates)), "events_per_s_runs": [float(r) for r in rates], "group_events": 1000,
                "note": "warm-up groups run on the main thread; each worker thread pays its own first-trip allocation inside the timing"}
    # fused: regex A parse alone, and parse + timestamp on the same stream
    n = 1 << 18
    cdata, coff, clen = corpus.apache_batch(n, "A")
    rx = binding.GpuRegex(corpus.REGEX_A)
    G = rx.groups
    d_data, d_off = torch.from_numpy(cdata).to(dev), torch.from_numpy(coff.astype(np.int32)).to(dev)
    d_caps = torch.empty((n, 2 * G), dtype=torch.int32, device=dev)
    d_status = torch.empty((n,), dtype=torch.uint8, device=dev)
    t = timestamp.GpuStrptime("%d/%b/%Y:%H:%M:%S")
    out = t.device_outputs(n, dev)
    # which group holds the time: the one whose first capture reads dd/Mon/...
    rx.match_device(d_data, d_off, None, n, d_caps, d_status, sep_bytes=1, stream=stream)
    torch.cuda.synchronize()
    caps0, status0 = d_caps.cpu().numpy(), d_status.cpu().numpy()
    first = int(np.nonzero(status0 == 1)[0][0])
    line0 = bytes(cdata[coff[first]:coff[first] + clen[first]])
    group = next(g for g in range(G) if line0[caps0[first, 2 * g] + 2:caps0[first, 2 * g] + 3] == b"/")

    def parse_only():
        rx.match_device(d_data, d_off, None, n, d_caps, d_status, sep_bytes=1, stream=stream)

    def parse_and_time():
        rx.match_device(d_data, d_off, None, n, d_caps, d_status, sep_bytes=1, stream=stream)
        t.parse_captures_device(d_data, d_off, d_caps, G, group, d_status, 1, n, out, stream=stream)
    parse_and_time()
    torch.cuda.synchronize()
    st = out["status"].cpu().numpy()
    assert np.all(st[status0 == 1] & 1), "the timestamp kernel did not parse the time field of every matched line"
    a, b = timed(torch, parse_only), timed(torch, parse_and_time)
    result["fused"] = {"lines": n, "line_bytes": int(clen.sum()), "time_group": group, "parse_only": a, "parse_plus_timestamp": b,
                       "added_ms_median": b["median_ms"] - a["median_ms"],
                       "note": "parse_only is the parent commit's trip: nothing on its path changed"}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"kernel": {k: v["median_ms"] for k, v in result["kernel"].items()}, "fused_added_ms": result["fused"]["added_ms_median"]}))


if __name__ == "__main__":
    main()
