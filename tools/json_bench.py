"""Measures the JSON parser: json_walk_kernel on lines resident in HBM, the same per-line routine on one host thread, and the
processor inside an agent-shaped loop.

    python tools/json_bench.py [--lines N] [--device-only] [--out profiles/json_bench.json]

* resident: N (default 1 Mi) lines of exactly 512 bytes of the bench corpus' JSON shape (corpus.mixed_batch: time, level, msg) with a few
  integer members -- flat; the same with 20 % of the lines carrying escapes in msg; the same with a nested member.  HIP events around
  one lc_json_walk_device call (BOTH its launches: the walk and the second launch for lines nested deeper than 64 levels, which finds
  none here), 3 warm-up calls, then five timed ones: min / median / max, bytes/s, fraction of 8 TB/s.  W = 8.
* yardsticks on file: delim_split_kernel on the same byte volume (profiles/delimiter_bench.json, read here and copied next to the result
  with the ratio), and the host routine: jsonWalkLine compiled for the host (tests/native/json_host_check.cpp) over 64 Ki of the flat
  lines on one thread.
* in agent: 1000-event groups of the flat lines through lc_json_processor_process from 1 and 16 threads, events per second.
Prints one JSON document and writes it to --out."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINE = 512
HBM_BYTES_PER_S = 8e12
W = 8
LEVELS = [b"info", b"warn", b"error", b"debug"]


def make_lines(n_pool, kind, seed):
    """n_pool distinct lines of exactly LINE bytes.  kind: flat / escapes (20 % of the lines) / nested"""
    rng = np.random.Generator(np.random.MT19937(seed))
    words = [b"request", b"served", b"from", b"cache", b"upstream", b"timeout", b"user", b"session", b"GET", b"/api/v1/items", b"200", b"ms"]
    out = np.empty((n_pool, LINE), np.uint8)
    for i in range(n_pool):
        head = b'{"time":"2024-06-25T23:%02d:%02dZ","level":"%s","status":%d,"bytes":%d,"latency_us":%d,' % (
            rng.integers(60), rng.integers(60), LEVELS[rng.integers(4)], rng.integers(100, 600), rng.integers(10 ** 7), rng.integers(10 ** 6))
        if kind == "nested":
            head += b'"ctx":{"ids":[%d,%d,{"trace":null}],"flags":{"retry":false,"tags":["a","b%d"]}},' % (
                rng.integers(10 ** 6), rng.integers(10 ** 6), rng.integers(100))
        head += b'"msg":"'
        escaped = kind == "escapes" and rng.random() < 0.2
        body = b""
        room = LINE - len(head) - 2
        while len(body) < room:
            body += words[rng.integers(len(words))] + b" "
            if escaped and rng.random() < 0.15:
                body += [b'\\n', b'\\"q\\"', b"\\u00e9", b"\\t", b"\\\\"][rng.integers(5)]
        body = body[:room]
        while body.endswith(b"\\") or (escaped and b"\\" in body[-6:]):      # (the cut may have split an escape)
            body = body[:body.rindex(b"\\")] if b"\\" in body[-6:] else body[:-1]
        line = head + body + b"x" * (room - len(body)) + b'"}'
        assert len(line) == LINE
        out[i] = np.frombuffer(line, np.uint8)
    return out


def resident_leg(n_lines, kind):
    import torch
    from loongcollector_amd import json_parse
    dev = torch.device("cuda:0")
    pool = make_lines(8192, kind, 20261017)
    idx = np.random.Generator(np.random.MT19937(1)).integers(0, len(pool), size=n_lines)
    data = pool[idx].reshape(-1)
    off = (np.arange(n_lines + 1, dtype=np.int64) * LINE).astype(np.int32)
    d_data = torch.from_numpy(data).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_st = torch.empty((n_lines,), dtype=torch.uint8, device=dev)
    d_nm = torch.empty((n_lines,), dtype=torch.int32, device=dev)
    d_err = torch.empty((n_lines,), dtype=torch.int32, device=dev)
    d_rec = torch.empty((n_lines, W, 20), dtype=torch.uint8, device=dev)
    d_sh = torch.empty((len(data),), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    js = json_parse.GpuJson()

    def fn():
        js.walk_device(d_data, d_off, n_lines, W, d_st, d_nm, d_err, d_rec, d_sh, stream=stream)

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
    members = 7 if kind == "nested" else 6
    assert int((d_st == 1).sum()) == n_lines and int(d_nm.min()) == members and int(d_nm.max()) == members, "the corpus did not parse"
    return {"lines": n_lines, "line_bytes": LINE, "members": members, "W": W, "ms_min": min(ms), "ms_median": med, "ms_max": max(ms),
            "spread_ms": max(ms) - min(ms), "bytes_per_s": n_lines * LINE / (med * 1e-3), "frac_of_8TBps": n_lines * LINE / (med * 1e-3) / HBM_BYTES_PER_S,
            "ns_per_byte": med * 1e6 / (n_lines * LINE)}


def host_leg(n_lines=1 << 16):
    """jsonWalkLine on one host thread"""
    so = os.path.join(ROOT, "loongcollector_amd", "lib", "libjson_host_check.so")
    src = os.path.join(ROOT, "tests", "native", "json_host_check.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(os.path.join(ROOT, "loongcollector_amd", "csrc", "json_vm.hpp"))):
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-o", so, src])
    L = ctypes.CDLL(so)
    L.jh_walk_batch.restype = None
    L.jh_walk_batch.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint32] * 2 + [ctypes.c_void_p] * 5
    pool = make_lines(8192, "flat", 20261017)
    idx = np.random.Generator(np.random.MT19937(1)).integers(0, len(pool), size=n_lines)
    data = np.ascontiguousarray(pool[idx].reshape(-1))
    off = np.arange(n_lines + 1, dtype=np.int64) * LINE
    st = np.zeros(n_lines, np.uint8)
    nm = np.zeros(n_lines, np.uint32)
    err = np.zeros(n_lines, np.uint32)
    rec = np.zeros(n_lines * W * 20, np.uint8)
    sh = np.zeros(len(data), np.uint8)
    secs = []
    for _ in range(4):
        t0 = time.perf_counter()
        L.jh_walk_batch(data.ctypes.data, off.ctypes.data, n_lines, W, st.ctypes.data, nm.ctypes.data, err.ctypes.data, rec.ctypes.data, sh.ctypes.data)
        secs.append(time.perf_counter() - t0)
    assert int((st == 1).sum()) == n_lines
    best = min(secs[1:])
    return {"lines": n_lines, "line_bytes": LINE, "seconds_best_of_3": best, "bytes_per_s": n_lines * LINE / best, "ns_per_byte": best * 1e9 / (n_lines * LINE),
            "what": "jsonWalkLine through JsonHostSource (16-byte quads rebuilt byte by byte), g++ -O3, one thread"}


def agent_leg(threads, groups_per_thread=200):
    from loongcollector_amd import json_parse
    from loongcollector_amd.processor import EventGroup
    pool = make_lines(1000, "flat", 99)
    data = pool.reshape(-1)
    off = (np.arange(1000, dtype=np.uint32) * LINE)
    length = np.full(1000, LINE, np.uint32)
    p = json_parse.JsonProcessor({"SourceKey": "content"})

    def worker():
        for _ in range(groups_per_thread):
            g = EventGroup.from_lines(data, off, length)
            p.process(g)
            g.close()

    worker()                                     # warm-up: staging and stream of the first thread
    ts = [threading.Thread(target=worker) for _ in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    c = p.counters()
    assert c["out_successful_events_total"] == (threads + 1) * groups_per_thread * 1000 and c["device_failed_events_total"] == 0
    return {"threads": threads, "events_per_s": threads * groups_per_thread * 1000 / dt, "event_bytes": LINE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--device-only", action="store_true", help="the resident legs only (what a profiler run wants)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "json_bench.json"))
    args = ap.parse_args()
    doc = {"resident_flat": resident_leg(args.lines, "flat"), "resident_20pct_escapes": resident_leg(args.lines, "escapes"),
           "resident_nested": resident_leg(args.lines, "nested")}
    try:
        with open(os.path.join(ROOT, "profiles", "delimiter_bench.json")) as f:
            d = json.load(f)["device_quote_free"]
        per_byte = d["delimiter"]["ms_median"] * 1e6 / (d["lines"] * d["line_bytes"])
        doc["yardstick_delim_split_kernel"] = {"file": "profiles/delimiter_bench.json", "ms_median": d["delimiter"]["ms_median"], "lines": d["lines"],
                                               "line_bytes": d["line_bytes"], "ns_per_byte": per_byte,
                                               "json_flat_over_delimiter_per_byte": doc["resident_flat"]["ns_per_byte"] / per_byte}
    except (OSError, KeyError):
        pass
    if not args.device_only:
        doc["host_routine_one_thread"] = host_leg()
        doc["kernel_over_host_routine_bytes_per_s"] = doc["resident_flat"]["bytes_per_s"] / doc["host_routine_one_thread"]["bytes_per_s"]
        doc["in_agent_1_thread"] = agent_leg(1)
        doc["in_agent_16_threads"] = agent_leg(16)
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if not args.device_only:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
