"""Measures the LZ4 block writer on an MI355X -> profiles/lz4_bench.json.

    python tools/lz4_bench.py [--n 1048576] [--out profiles/lz4_bench.json] [--skip-agent] [--skip-engine] [--chunks 4096,16384,65536]
                              [--merge-trace 4096=DIR ...]

* the engine, resident in device memory, two inputs of the same size: the SLS records of 1 Mi lines of 512 bytes of the headline corpus
  (tools/sls_bench.py's payload) cut into segments of 1000 records, and the multiline corpus (4 MiB of it, repeated: no match reaches
  from one copy into the next) cut into segments of the same mean size.  HIP events, 3 warm-up launches, 5 timed launches, min / median /
  max; everything that is compared is timed in the SAME run, alternating, per chunk size:
    - lc_lz4_compress_device with room (every kernel),
    - the same with out_cap 0 (lz4_emit_kernel returns before its first store) -- the emit kernel's stores by difference,
    - lc_sls_encode_device on the batch the records came from (sls_write_kernel among its kernels),
    - a device-to-device copy of the input.
  The first segments are decoded (tests/helpers/lz4_block.py) before anything is timed; the ratio stands beside LZ4_compress_default of
  the system's liblz4 on the same first segments, where there is one ("not measured" otherwise).
  Per-kernel times come from a kernel trace taken in a run of its own (one per chunk size) and folded in with --merge-trace.
* in an agent: groups of 1000 such lines, 1 and 16 runner threads, in the same run:
    - lc_lz4_match_encode_compress_host at every chunk size (only the block comes down),
    - lc_sls_match_encode_host alone (the records come down uncompressed),
    - lc_sls_match_encode_host followed by LZ4_compress_default on the calling thread: what an agent does today.
  lines/s over all threads.
Not measured here: hardware counters, lines of other lengths, other tag sets."""
import argparse
import csv
import ctypes
import glob
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LINE_BYTES, GROUP_LINES = 512, 1000
TAGS = [(b"__topic__", b"bench"), (b"__source__", b"10.0.0.1"), (b"__machine_uuid__", b"0123456789abcdef"), (b"__tag__:__path__", b"/var/log/access.log")]


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


def engine(torch, n, chunks, runs):
    from helpers import lz4_block as decoder
    from helpers import lz4_cases as lc
    from loongcollector_amd import binding, corpus, lz4_block, sls
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    data, off, length = corpus.apache_batch(n, "A", line_bytes=LINE_BYTES)
    rx = binding.GpuRegex(corpus.REGEX_A)
    G = rx.groups
    plan = sls.Plan([k.encode() for k in corpus.KEYS_A], [(g - 1, g) for g in range(1, G + 1)], [])
    d_data = torch.from_numpy(data).to(dev)
    d_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    d_caps = torch.empty((n, 2 * G), dtype=torch.int32, device=dev)
    d_status = torch.empty((n,), dtype=torch.uint8, device=dev)
    d_time = torch.full((n,), 1700000000, dtype=torch.int32, device=dev)
    d_rec = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_sls_scratch = torch.empty(sls.scratch_bytes(n), dtype=torch.uint8, device=dev)
    rx.match_device(d_data, d_off, None, n, d_caps, d_status, sep_bytes=1, stream=stream)
    sls.encode_device(plan, d_data, d_off, None, 1, n, G, d_caps, d_status, d_time, None, 0, None, 0, d_rec, d_sls_scratch, stream=stream)
    torch.cuda.synchronize()
    total = int(d_rec[n])
    d_records = torch.zeros(total + 64, dtype=torch.uint8, device=dev)

    def sls_encode():
        sls.encode_device(plan, d_data, d_off, None, 1, n, G, d_caps, d_status, d_time, None, 0, d_records, total, d_rec, d_sls_scratch, stream=stream)
    sls_encode()
    torch.cuda.synchronize()
    rec = d_rec.cpu().numpy()
    cuts = np.append(rec[0:n:GROUP_LINES], rec[n]).astype(np.int64)
    # the multiline corpus, repeated to the same size, cut into segments of the same mean size
    unit = np.frombuffer(corpus.multiline_buffer(4 << 20), np.uint8)
    reps = -(-total // len(unit))
    d_multi = torch.from_numpy(unit.copy()).to(dev).repeat(reps)[:total].contiguous()
    seg = int(np.diff(cuts).mean())
    mcuts = np.append(np.arange(0, total, seg, dtype=np.int64), total)
    L = lc.system_lz4()
    d_copy = torch.empty(total, dtype=torch.uint8, device=dev)
    out = {"n": n, "line_bytes": LINE_BYTES, "input_bytes": total, "sls_encode_device": None, "inputs": {}}
    sls_timing = None
    for name, d_in, c in (("sls_records_of_headline_lines", d_records, cuts), ("multiline_corpus", d_multi, mcuts)):
        n_seg = len(c) - 1
        d_begin = torch.from_numpy(c[:-1].copy()).to(dev)
        d_len = torch.from_numpy(np.diff(c).astype(np.uint32).view(np.int32).copy()).to(dev)
        d_out = torch.empty(lz4_block.bound(total) + 16 * n_seg, dtype=torch.uint8, device=dev)
        d_out_off = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
        rows = {"segments": n_seg}
        check = min(n_seg, 100)
        host_in = d_in[:int(c[check])].cpu().numpy()
        if L is not None:
            ref_bytes = sum(len(lc.system_compress(L, host_in[c[s]:c[s + 1]].tobytes())) for s in range(check))
            rows["liblz4_ratio_first_segments"] = ref_bytes / int(c[check])
        else:
            rows["liblz4_ratio_first_segments"] = "not measured"
        for chunk in chunks:
            ctx = lz4_block.Lz4(chunk)
            d_scratch = torch.empty(ctx.scratch_bytes(total, n_seg), dtype=torch.uint8, device=dev)

            def full():
                ctx.compress_device(d_in, d_begin, d_len, n_seg, d_out, d_out.numel(), d_out_off, d_scratch, stream=stream)

            def no_room():
                ctx.compress_device(d_in, d_begin, d_len, n_seg, d_out, 0, d_out_off, d_scratch, stream=stream)
            full()
            torch.cuda.synchronize()
            o = d_out_off.cpu().numpy()
            blocks = d_out[:int(o[check])].cpu().numpy().tobytes()
            for s in range(0, check, 7):
                assert decoder.decode(blocks[o[s]:o[s + 1]], int(c[s + 1] - c[s]))[0] == host_in[c[s]:c[s + 1]].tobytes(), "segment %d does not decode" % s
            names = ["compress_device", "compress_device_out_cap_0", "sls_encode_device", "device_to_device_copy_of_the_input"]
            t = dict(zip(names, timed_alternating(torch, [full, no_room, sls_encode, lambda: d_copy.copy_(d_in[:total])], runs=runs)))
            t["emit_stores_by_difference_ms"] = t["compress_device"]["median_ms"] - t["compress_device_out_cap_0"]["median_ms"]
            t["input_GBps"] = total / (t["compress_device"]["median_ms"] / 1e3) / 1e9
            t["over_the_copy"] = t["compress_device"]["median_ms"] / t["device_to_device_copy_of_the_input"]["median_ms"]
            t["ratio"] = int(o[n_seg]) / total
            t["ratio_first_segments"] = int(o[check]) / int(c[check])
            if L is not None:
                t["size_over_liblz4_first_segments"] = t["ratio_first_segments"] / rows["liblz4_ratio_first_segments"]
            t["scratch_bytes"] = int(d_scratch.numel())
            rows["chunk_%d" % chunk] = t
            del d_scratch
        out["inputs"][name] = rows
    out["default_chunk_bytes"] = lz4_block.Lz4().chunk_bytes
    return out


def agent(threads_list, groups_per_thread, chunks):
    from helpers import lz4_cases as lc
    from loongcollector_amd import binding, corpus, lz4_block, sls
    S, Z = sls.load(), lz4_block.load()
    system = lc.system_lz4()
    data, off, length = corpus.apache_batch(GROUP_LINES * 64, "A", line_bytes=LINE_BYTES)
    rx = binding.GpuRegex(corpus.REGEX_A)
    G = rx.groups
    plan = sls.Plan([k.encode() for k in corpus.KEYS_A], [(g - 1, g) for g in range(1, G + 1)], [])
    ctxs = {"lz4_match_encode_compress_host_chunk_%d" % c: lz4_block.Lz4(c) for c in chunks}
    tags = np.frombuffer(sls.append_tags(TAGS), np.uint8).copy()
    ptrs = (data.ctypes.data + off[:-1].astype(np.uint64)).astype(np.uint64)
    lens = length.astype(np.uint32)
    times = np.full(GROUP_LINES, 1700000000, np.uint32)
    legs_names = list(ctxs) + ["sls_match_encode_host"] + (["sls_match_encode_host_then_LZ4_compress_default"] if system is not None else [])
    out = {}
    for threads in threads_list:
        per = groups_per_thread[threads]
        legs = {}
        for leg in legs_names:
            barrier = threading.Barrier(threads + 1)
            down = [0] * threads
            raw = [0] * threads

            def runner(t):
                o, n, r = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()
                status = np.zeros(GROUP_LINES, np.uint8)
                room = ctypes.create_string_buffer(lz4_block.bound(GROUP_LINES * 1024))

                def one(k):
                    at = ((t * per + k) % 64) * GROUP_LINES
                    p, ln = ptrs[at:at + GROUP_LINES], lens[at:at + GROUP_LINES]
                    if leg in ctxs:
                        assert Z.lc_lz4_match_encode_compress_host(ctxs[leg].handle, plan.handle, rx.handle, p.ctypes.data, ln.ctypes.data, GROUP_LINES,
                                                                   times.ctypes.data, None, 0, tags.ctypes.data, len(tags), ctypes.byref(o),
                                                                   ctypes.byref(n), ctypes.byref(r), None, status.ctypes.data) == 0
                        return n.value, r.value
                    assert S.lc_sls_match_encode_host(plan.handle, rx.handle, p.ctypes.data, ln.ctypes.data, GROUP_LINES, times.ctypes.data, None, 0,
                                                      ctypes.byref(o), ctypes.byref(n), None, status.ctypes.data) == 0
                    if leg == "sls_match_encode_host":
                        return n.value, n.value
                    got = system.LZ4_compress_default(ctypes.cast(o, ctypes.c_char_p), room, n.value, len(room))
                    assert got > 0
                    return got, n.value
                one(0)   # (one group outside the clock: the thread's staging, stream and tables)
                barrier.wait()
                for k in range(per):
                    d, w = one(k)
                    down[t] += d
                    raw[t] += w
                barrier.wait()
                Z.lc_lz4_thread_release()
                S.lc_sls_thread_release()

            ts = [threading.Thread(target=runner, args=(t,)) for t in range(threads)]
            for t in ts:
                t.start()
            barrier.wait()
            t0 = time.perf_counter()
            barrier.wait()
            dt = time.perf_counter() - t0
            for t in ts:
                t.join()
            lines = threads * per * GROUP_LINES
            legs[leg] = {"seconds": dt, "groups": threads * per, "lines_per_s": lines / dt, "us_per_group_per_thread": dt / per * 1e6,
                         "raw_bytes": sum(raw), "bytes_handed_to_the_sender": sum(down)}
        for name in ctxs:
            legs[name]["over_the_uncompressed_trip"] = legs[name]["lines_per_s"] / legs["sls_match_encode_host"]["lines_per_s"]
            if system is not None:
                legs[name]["over_encode_then_host_lz4"] = legs[name]["lines_per_s"] / legs["sls_match_encode_host_then_LZ4_compress_default"]["lines_per_s"]
        out["threads_%d" % threads] = legs
    return out


def kernel_trace(directory):
    """median duration per kernel name of a rocprofv3 --kernel-trace CSV below `directory` (the LZ4 kernels and sls_write_kernel)"""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"].split("(")[0].split("::")[-1].split("<")[0]
                if name.startswith("lz4_") or name.startswith("sls_write"):
                    full = r["Kernel_Name"].split("(")[0].split("::")[-1]
                    rows.setdefault(full, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "dispatches": len(v)} for k, v in sorted(rows.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz4_bench.json"))
    ap.add_argument("--chunks", default="4096,16384,65536")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-agent", action="store_true")
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--merge-trace", nargs="*", default=[], help="CHUNK=DIR: fold a kernel trace taken in a run of its own into --out")
    args = ap.parse_args()
    if args.merge_trace:
        with open(args.out) as f:
            result = json.load(f)
        result["kernel_trace"] = {"how": "rocprofv3 --kernel-trace, one run of its own per chunk size over both inputs (all dispatches of the run: "
                                         "warm-up and timed, both inputs together)"}
        for item in args.merge_trace:
            chunk, directory = item.split("=", 1)
            result["kernel_trace"]["chunk_%s" % chunk] = kernel_trace(directory)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps(result["kernel_trace"]))
        return
    import torch
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "engine: HIP events, 3 warm-up launches, %d timed launches per row, rows alternating in the same run; agent: wall clock "
                        "between two barriers around all threads' groups, one group per thread before the clock" % args.runs,
              "not_measured": ["hardware counters", "lines of other lengths", "other tag sets", "chunk sizes other than those listed"]}
    if not args.skip_engine:
        result["engine"] = engine(torch, args.n, [int(c) for c in args.chunks.split(",")], args.runs)
    if not args.skip_agent:
        result["agent"] = agent([1, 16], {1: 200, 16: 40}, [int(c) for c in args.chunks.split(",")])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    brief = {}
    if "engine" in result:
        brief["engine"] = {name: {k: {"ms": round(v["compress_device"]["median_ms"], 3), "x_copy": round(v["over_the_copy"], 2), "ratio": round(v["ratio"], 4)}
                                  for k, v in rows.items() if isinstance(v, dict)} for name, rows in result["engine"]["inputs"].items()}
    if "agent" in result:
        brief["agent_lines_per_s"] = {t: {k: round(v["lines_per_s"]) for k, v in legs.items() if isinstance(v, dict)} for t, legs in result["agent"].items()}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
