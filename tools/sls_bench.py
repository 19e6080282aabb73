"""Measures the SLS encoder on an MI355X -> profiles/sls_bench.json.

    python tools/sls_bench.py [--n 1048576] [--out profiles/sls_bench.json] [--skip-agent]

* the engine: 1 Mi lines of 512 bytes of the headline corpus, regex A, resident in device memory; the plan writes regex A's ten keys
  for a matched line and nothing for any other.  HIP events, 3 warm-up launches, 5 timed launches, min / median / max; everything that
  is compared is timed in the SAME run, alternating:
    - lc_sls_encode_device with room (sls_size_kernel + the scan + sls_write_kernel),
    - the same with out_cap 0 (size + scan; sls_write_kernel returns at its first test) -- the write kernel's own time is the difference
      of the two medians, not a measurement of its own,
    - lc_regex_match_device on the same batch,
    - a device-to-device copy of as many bytes as the payload has.
  The first 2048 records are compared with tests/helpers/sls_wire.py before anything is timed.
* in an agent: groups of 1000 such lines (lc_group_from_lines), 1 and 16 runner threads, in the same run:
    - lc_sls_processor_serialize on the device path,
    - lc_processor_process on the same groups,
    - lc_processor_process followed by lc_sls_serialize_group_host: what an agent does today.
  lines/s over all threads; every thread works through its own groups, each group once per leg where the leg consumes it.
Not measured here: hardware counters and a kernel trace (taken separately), lines of other lengths, the tags."""
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

LINE_BYTES, GROUP_LINES = 512, 1000


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


def engine(torch, n):
    from helpers import sls_wire
    from loongcollector_amd import binding, corpus, sls
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    data, off, length = corpus.apache_batch(n, "A", line_bytes=LINE_BYTES)
    rx = binding.GpuRegex(corpus.REGEX_A)
    G = rx.groups
    keys = [k.encode() for k in corpus.KEYS_A]
    assert len(keys) == G
    plan = sls.Plan(keys, [(g - 1, g) for g in range(1, G + 1)], [])
    d_data = torch.from_numpy(data).to(dev)
    d_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    d_caps = torch.empty((n, 2 * G), dtype=torch.int32, device=dev)
    d_status = torch.empty((n,), dtype=torch.uint8, device=dev)
    d_time = torch.full((n,), 1700000000, dtype=torch.int32, device=dev)
    d_rec = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_scratch = torch.empty(sls.scratch_bytes(n), dtype=torch.uint8, device=dev)

    def match():
        rx.match_device(d_data, d_off, None, n, d_caps, d_status, sep_bytes=1, stream=stream)
    match()
    sls.encode_device(plan, d_data, d_off, None, 1, n, G, d_caps, d_status, d_time, None, 0, None, 0, d_rec, d_scratch, stream=stream)
    torch.cuda.synchronize()
    total = int(d_rec[n])
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    d_copy = torch.empty(total, dtype=torch.uint8, device=dev)

    def full():
        sls.encode_device(plan, d_data, d_off, None, 1, n, G, d_caps, d_status, d_time, None, 0, d_out, total, d_rec, d_scratch, stream=stream)

    def size_scan():
        sls.encode_device(plan, d_data, d_off, None, 1, n, G, d_caps, d_status, d_time, None, 0, d_out, 0, d_rec, d_scratch, stream=stream)
    full()
    torch.cuda.synchronize()
    # the first records against the model
    check = min(n, 2048)
    caps, status, rec = d_caps[:check].cpu().numpy(), d_status[:check].cpu().numpy(), d_rec[:check + 1].cpu().numpy()
    got = d_out[:int(rec[check])].cpu().numpy().tobytes()
    want = b""
    for i in range(check):
        line = data[off[i]:off[i] + length[i]].tobytes()
        contents = [(keys[g], line[caps[i, 2 * g]:caps[i, 2 * g + 1]] if caps[i, 2 * g] >= 0 else b"") for g in range(G)] if status[i] == 1 else []
        want += sls_wire.record(1700000000, None, contents, 0)
    assert got == want, "the first %d records differ from the model" % check
    names = ["encode_size_scan_write", "encode_size_scan_only", "regex_match_device", "device_to_device_copy_of_the_payload"]
    timings = timed_alternating(torch, [full, size_scan, match, lambda: d_copy.copy_(d_out[:total])])
    block = dict(zip(names, timings))
    write_ms = block["encode_size_scan_write"]["median_ms"] - block["encode_size_scan_only"]["median_ms"]
    copy_ms = block["device_to_device_copy_of_the_payload"]["median_ms"]
    block["write_kernel_by_difference"] = {"median_ms": write_ms, "payload_GBps": total / (write_ms / 1e3) / 1e9, "over_the_copy": write_ms / copy_ms}
    block["encode_size_scan_write"]["over_the_copy"] = block["encode_size_scan_write"]["median_ms"] / copy_ms
    block["encode_size_scan_write"]["over_the_match"] = block["encode_size_scan_write"]["median_ms"] / block["regex_match_device"]["median_ms"]
    block.update({"n": n, "line_bytes": LINE_BYTES, "input_bytes": int(length.sum()), "payload_bytes": total, "matched": int(d_status.sum()), "keys": G})
    return block


def agent(threads_list, groups_per_thread):
    from loongcollector_amd import binding, corpus, sls
    L, S = binding.load(), sls.load()
    config = {"SourceKey": "content", "Regex": corpus.REGEX_A, "Keys": corpus.KEYS_A}
    data, off, length = corpus.apache_batch(GROUP_LINES * 64, "A", line_bytes=LINE_BYTES)
    off32, len32 = off[:-1].astype(np.uint32), length.astype(np.uint32)

    def new_group(k):
        at = (k % 64) * GROUP_LINES
        return L.lc_group_from_lines(data.ctypes.data, off32[at:at + GROUP_LINES].ctypes.data, len32[at:at + GROUP_LINES].ctypes.data, GROUP_LINES, b"content")

    out = {}
    for threads in threads_list:
        per = groups_per_thread[threads]
        sproc = sls.Processor(config)
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        assert L.lc_processor_create(json.dumps(config).encode(), ctypes.byref(h), err, 512) == 0, err.value
        legs = {}
        for leg in ("sls_processor_serialize_device_path", "processor_process", "processor_process_then_host_writer"):
            groups = [[new_group(t * per + k) for k in range(per)] for t in range(threads)]
            barrier = threading.Barrier(threads + 1)
            bytes_out = [0] * threads
            fused = [0] * threads

            def runner(t):
                o, n, f = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
                # (one group outside the clock: the thread's staging, stream and tables)
                warm = new_group(t)
                if leg == "sls_processor_serialize_device_path":
                    assert S.lc_sls_processor_serialize(sproc._h, warm, 0, ctypes.byref(o), ctypes.byref(n), ctypes.byref(f)) == 0
                else:
                    assert L.lc_processor_process(h, warm) == 0
                L.lc_group_free(warm)
                barrier.wait()
                for g in groups[t]:
                    if leg == "sls_processor_serialize_device_path":
                        assert S.lc_sls_processor_serialize(sproc._h, g, 0, ctypes.byref(o), ctypes.byref(n), ctypes.byref(f)) == 0
                        fused[t] += f.value
                        bytes_out[t] += n.value
                    else:
                        assert L.lc_processor_process(h, g) == 0
                        if leg == "processor_process_then_host_writer":
                            assert S.lc_sls_serialize_group_host(g, 0, ctypes.byref(o), ctypes.byref(n)) == 0
                            bytes_out[t] += n.value
                barrier.wait()
                S.lc_sls_thread_release()
                L.lc_thread_release()

            ts = [threading.Thread(target=runner, args=(t,)) for t in range(threads)]
            for t in ts:
                t.start()
            barrier.wait()
            t0 = time.perf_counter()
            barrier.wait()
            dt = time.perf_counter() - t0
            for t in ts:
                t.join()
            for row in groups:
                for g in row:
                    L.lc_group_free(g)
            lines = threads * per * GROUP_LINES
            legs[leg] = {"seconds": dt, "groups": threads * per, "lines_per_s": lines / dt, "input_MBps": lines * LINE_BYTES / dt / 1e6,
                         "us_per_group_per_thread": dt / per * 1e6, "wire_bytes": sum(bytes_out)}
            if leg == "sls_processor_serialize_device_path":
                assert sum(fused) == threads * per, "a group left the device path"
        assert legs["sls_processor_serialize_device_path"]["wire_bytes"] == legs["processor_process_then_host_writer"]["wire_bytes"]
        legs["device_path_over_today"] = legs["sls_processor_serialize_device_path"]["lines_per_s"] / legs["processor_process_then_host_writer"]["lines_per_s"]
        out["threads_%d" % threads] = legs
        L.lc_processor_destroy(h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sls_bench.json"))
    ap.add_argument("--skip-agent", action="store_true")
    ap.add_argument("--skip-engine", action="store_true")
    args = ap.parse_args()
    import torch
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "engine: HIP events, 3 warm-up launches, 5 timed launches per row, rows alternating in the same run; agent: wall clock "
                        "between two barriers around all threads' groups, one group per thread before the clock",
              "not_measured": ["hardware counters", "a kernel trace", "lines of other lengths", "lc_sls_append_tags"]}
    if not args.skip_engine:
        result["engine"] = engine(torch, args.n)
    if not args.skip_agent:
        result["agent"] = agent([1, 16], {1: 300, 16: 60})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    brief = {}
    if "engine" in result:
        brief["engine_ms"] = {k: round(v["median_ms"], 4) for k, v in result["engine"].items() if isinstance(v, dict)}
    if "agent" in result:
        brief["agent_lines_per_s"] = {t: {k: round(v["lines_per_s"]) for k, v in legs.items() if isinstance(v, dict)} for t, legs in result["agent"].items()}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
