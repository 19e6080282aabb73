"""Measures the desensitize processor on an MI355X -> profiles/desensitize_bench.json.

    python tools/desensitize_bench.py [--n 1048576] [--out profiles/desensitize_bench.json]

* batches: 1 Mi lines of 512 bytes resident in device memory (4096 distinct lines, tiled), ONE and THREE secrets per line, `const` and
  `md5`, ReplacingAll on; HIP events, 2 warm-up calls, 5 timed runs, every timing with its spread.  Alternating in the same run, on
  the same bytes:
    - lc_desens_apply_device (every search round, the collect / size / scan / write kernels, the host's reads of the round counts);
    - lc_regex_match_device of the SAME handle: what finding the first match costs -- the difference is what collecting, the further
      rounds and rewriting add;
    - a device-to-device copy of the batch: the floor of the write kernel, which reads and writes every byte of a changed value once.
* host: the per-value routine (outLen + writeValue of csrc/desens_vm.hpp compiled for the host) on one thread over a 64 Ki slice with
  PRECOMPUTED cuts (tests/native/desens_double.cpp dd_write_resident): no search is timed.
* in-agent: 1000-event groups through lc_desensitize_process from 1 and 16 threads.
There is no pass mark; what bounds each number is said in DESIGN.md.
"""
import argparse
import ctypes
import json
import os
import random
import re
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LINE_BYTES = 512
WORDS = ["request", "served", "in", "ms", "status", "ok", "user", "path=/api/v1/items", "GET", "POST", "cache", "miss", "retry", "n=3"]
RULE = ("pwd=", "[^,]+", "********")


def line_of(rng, secrets):
    parts = [b"pwd=" + bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(rng.randrange(6, 17))) + b"," for _ in range(secrets)]
    room = LINE_BYTES - sum(map(len, parts))
    text = bytearray()
    while len(text) < room:
        text += rng.choice(WORDS).encode() + b" "
    text = bytes(text[:room])
    cuts = sorted(rng.randrange(room + 1) for _ in parts)
    out, at = [], 0
    for c, p in zip(cuts, parts):
        out += [text[at:c], p]
        at = c
    out.append(text[at:])
    line = b"".join(out)
    assert len(line) == LINE_BYTES
    return line


def spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs_ms": [float(x) for x in ms]}


def timed_alternating(torch, fns, warm=2, runs=5):
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


def rates(k, n, size):
    k["GBps_in"] = n * size / (k["median_ms"] / 1e3) / 1e9
    k["lines_per_s"] = n / (k["median_ms"] / 1e3)
    k["ns_per_line"] = k["median_ms"] * 1e6 / n
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "desensitize_bench.json"))
    args = ap.parse_args()
    import torch
    from loongcollector_amd import binding, desensitize
    from loongcollector_amd.processor import EventGroup
    from helpers import desensitize_product as dp
    dev = torch.device("cuda:0")
    rng = random.Random(23)
    n = args.n
    stream = torch.cuda.current_stream().cuda_stream
    L = desensitize._lib()
    result = {"device": torch.cuda.get_device_name(0), "n": n, "line_bytes": LINE_BYTES, "rule": {"before": RULE[0], "content": RULE[1], "replacing": RULE[2]},
              "batches": {}}
    corpora = {}
    for secrets in (1, 3):
        uniq = [line_of(rng, secrets) for _ in range(4096)]
        corpora[secrets] = uniq
        tile = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev)
        d_data = torch.cat([tile.repeat((n + len(uniq) - 1) // len(uniq))[:n * LINE_BYTES], torch.zeros(16, dtype=torch.uint8, device=dev)])
        d_off = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * LINE_BYTES).astype(np.int32)).to(dev)
        d_copy = torch.empty_like(d_data)
        d_flags = torch.empty(n, dtype=torch.uint8, device=dev)
        d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        for method in ("const", "md5"):
            eng = desensitize.GpuDesensitize(method, RULE[0], RULE[1], RULE[2], True)
            try:
                eng.apply_device(d_data, d_off, None, n, d_flags, d_out_off, None, stream=stream)
                raise AssertionError("nothing changed")
            except desensitize.DesensitizeOverflow as e:
                needed = e.needed
            d_out = torch.empty(needed, dtype=torch.uint8, device=dev)
            G = 2
            d_caps = torch.empty((n, 2 * G), dtype=torch.int32, device=dev)
            d_status = torch.empty(n, dtype=torch.uint8, device=dev)
            re_handle = L.lc_desens_regex(eng._h)
            stats = {}

            def apply():
                stats.update(eng.apply_device(d_data, d_off, None, n, d_flags, d_out_off, d_out, stream=stream)[1])

            def match():
                binding._check(L.lc_regex_match_device(re_handle, d_data.data_ptr(), d_off.data_ptr(), None, 0, n, G, d_caps.data_ptr(),
                                                       d_status.data_ptr(), stream), "lc_regex_match_device")

            a, m, c = timed_alternating(torch, [apply, match, lambda: d_copy.copy_(d_data)])
            assert int(d_flags.sum().item()) == n and int(d_status.sum().item()) == n, "not every line was found and changed"
            # one line against Python's own re / hashlib
            first = bytes(d_out[:int(d_out_off[1].item())].cpu().numpy())
            import hashlib
            want = re.sub(rb"(pwd=)([^,]+)", (lambda q: q.group(1) + RULE[2].encode()) if method == "const" else
                          (lambda q: q.group(1) + hashlib.md5(q.group(2)).hexdigest().upper().encode()), uniq[0])
            assert first == want, (first, want)
            entry = {"apply_device": rates(a, n, LINE_BYTES), "match_device_same_handle": rates(m, n, LINE_BYTES),
                     "device_to_device_copy": rates(c, n, LINE_BYTES), "rounds": stats["rounds"], "searches": stats["searches"],
                     "output_bytes": needed, "apply_over_match": a["median_ms"] / m["median_ms"], "apply_over_copy": a["median_ms"] / c["median_ms"]}
            result["batches"]["%s_%d_secret%s" % (method, secrets, "" if secrets == 1 else "s")] = entry
            del d_out, d_caps
        del d_data, d_copy, tile
        torch.cuda.empty_cache()

    # ---- the per-value routine on one host thread over precomputed cuts
    D = dp.double()
    h = min(n, 1 << 16)
    result["host_routine_one_thread"] = {}
    for secrets in (1, 3):
        uniq = corpora[secrets]
        lines = [uniq[i % len(uniq)] for i in range(h)]
        data = np.frombuffer(b"".join(lines) + b"\0" * 16, np.uint8).copy()
        off = (np.arange(h + 1, dtype=np.int64) * LINE_BYTES).astype(np.uint32)
        counts = np.zeros(h, np.uint32)
        rows = []
        for i, ln in enumerate(lines):
            found = list(re.finditer(rb"pwd=[^,]+", ln))
            counts[i] = len(found)
            for q in found:
                rows += [q.start(), q.end(), q.start(), q.start() + 4]
        rows = np.array(rows, np.int32)
        for method in ("const", "md5"):
            eng = dp.Engine(method, RULE[0], RULE[1], RULE[2], True)
            out = np.zeros(h * (LINE_BYTES + 3 * 40), np.uint8)
            secs = ctypes.c_double(0)
            runs = []
            for _ in range(5):
                wrote = D.dd_write_resident(eng._h, data.ctypes.data, off.ctypes.data, h, counts.ctypes.data, rows.ctypes.data, 2, out.ctypes.data,
                                            ctypes.byref(secs))
                runs.append(secs.value * 1e3)
            r = rates(spread(runs), h, LINE_BYTES)
            r["output_bytes"] = int(wrote)
            r["what"] = "outLen + writeValue of desens_vm.hpp compiled for the host (g++ -O2), one thread, cuts precomputed, no search"
            result["host_routine_one_thread"]["%s_%d" % (method, secrets)] = r

    # ---- in-agent: 1000-event groups
    result["in_agent"] = {}
    for method in ("const", "md5"):
        config = {"SourceKey": "content", "Method": method, "ReplacingString": RULE[2], "ContentPatternBeforeReplacedString": RULE[0],
                  "ReplacedContentPattern": RULE[1], "ReplacingAll": True}
        group_json = json.dumps({"events": [{"contents": {"content": v.decode()}, "timestamp": 1, "type": 1} for v in corpora[3][:1000]]})
        for threads in (1, 16):
            per = 20
            runs = []
            for _ in range(3):
                procs = [desensitize.DesensitizeProcessor(config) for _ in range(threads)]
                groups = [[EventGroup(group_json) for _ in range(per)] for _ in range(threads)]

                def work(p, gs):
                    for g in gs:
                        p.process(g)
                for p in procs:   # warm-up: the main thread's staging
                    p.process(EventGroup(group_json))
                ths = [threading.Thread(target=work, args=(p, gs)) for p, gs in zip(procs, groups)]
                t0 = time.perf_counter()
                for th in ths:
                    th.start()
                for th in ths:
                    th.join()
                runs.append(threads * per * 1000 / (time.perf_counter() - t0))
            result["in_agent"]["%s_threads_%d" % (method, threads)] = {
                "events_per_s_median": float(np.median(runs)), "events_per_s_runs": [float(r) for r in runs], "group_events": 1000, "secrets_per_event": 3,
                "MBps_median": float(np.median(runs)) * LINE_BYTES / 1e6,
                "note": "warm-up groups run on the main thread; each worker thread pays its own first-trip allocation inside the timing"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {"apply_ms": v["apply_device"]["median_ms"], "match_ms": v["match_device_same_handle"]["median_ms"],
                          "copy_ms": v["device_to_device_copy"]["median_ms"], "rounds": v["rounds"]} for k, v in result["batches"].items()}))


if __name__ == "__main__":
    main()
