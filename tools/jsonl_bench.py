"""Measures the JSON-lines encoder on an MI355X -> profiles/jsonl_bench.json.

    python tools/jsonl_bench.py [--n 1048576] [--out profiles/jsonl_bench.json] [--skip-agent] [--skip-engine] [--lib liblc_jsonl.so]

* the engine, on three corpora of 1 Mi lines of 512 bytes of the headline corpus resident in device memory (regex A's rows and status bytes
  are matched once, before the clock):
    - headline:       regex A's ten keys for a matched line, nothing for any other -- the clean path;
    - one_in_five:    the same, with a quote and a backslash stored into one captured group in five -- those items take the dirty path;
    - whole_line:     every line under the unmatched list's one key, the whole line -- three quoted fields each: all dirty.
  Per corpus, HIP events, 3 warm-up launches, 5 timed launches, min / median / max, everything timed in the SAME run, alternating:
    - lc_jsonl_encode_device with room (jsonl_size_kernel + the scan + jsonl_write_kernel),
    - the same with out_cap 0 (size + scan; jsonl_write_kernel returns at its first test) -- the write kernel's own time is the
      difference of the two medians, not a measurement of its own,
    - lc_sls_encode_device on the same batch and plan shape,
    - a device-to-device copy of as many bytes as the JSON payload has.
  The first 2048 records are compared with tests/helpers/jsonl_model.py before anything is timed.
* --lib: another build of the library (csrc/jsonl_device.hip compiled with -DLC_JSONL_LANES=4 .. 64): the sweep of lanes per event is
  this tool run once per build with --skip-agent.
* in an agent: groups of 1000 such lines (lc_group_from_lines), 1 and 16 runner threads, in the same run:
    - lc_jsonl_processor_serialize on the device path,
    - lc_processor_process followed by lc_jsonl_serialize_group_host: what an agent does today.
Not measured here: hardware counters and a kernel trace (taken separately), lines of other lengths, tags (the head is {"__time__":)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sls_bench import GROUP_LINES, LINE_BYTES, timed_alternating  # noqa: E402


def engine(torch, n):
    from helpers import jsonl_cases as jc
    from helpers import jsonl_model as jm
    from loongcollector_amd import binding, corpus, jsonl, sls
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    data, off, length = corpus.apache_batch(n, "A", line_bytes=LINE_BYTES)
    rx = binding.GpuRegex(corpus.REGEX_A)
    G = rx.groups
    keys = [k.encode() for k in corpus.KEYS_A]
    d_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    d_caps = torch.empty((n, 2 * G), dtype=torch.int32, device=dev)
    d_status = torch.empty((n,), dtype=torch.uint8, device=dev)
    d_time = torch.full((n,), 1700000000, dtype=torch.int32, device=dev)
    d_rec = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    head = jm.head()
    d_head = torch.from_numpy(np.frombuffer(head, np.uint8).copy()).to(dev)
    d_data = torch.from_numpy(data).to(dev)
    rx.match_device(d_data, d_off, None, n, d_caps, d_status, sep_bytes=1, stream=stream)
    torch.cuda.synchronize()
    caps, status = d_caps.cpu().numpy(), d_status.cpu().numpy()
    # one group in five with a quote and a backslash as its first two bytes (the rows stay as matched)
    dirty = data.copy()
    pick = (np.arange(n * G).reshape(n, G) % 5 == 0) & (caps[:, 0::2] >= 0) & (caps[:, 1::2] - caps[:, 0::2] >= 2) & (status[:, None] == 1)
    at = (off[:n, None].astype(np.int64) + caps[:, 0::2])[pick]
    dirty[at] = 0x22
    dirty[at + 1] = 0x5C
    corpora = {
        "headline": (data, status, (keys, [(g - 1, g) for g in range(1, G + 1)], [])),
        "one_in_five": (dirty, status, (keys, [(g - 1, g) for g in range(1, G + 1)], [])),
        "whole_line": (data, np.zeros(n, np.uint8), ([b"content"], [], [(0, 0)])),
    }
    out = {}
    for name, (bytes_, st, spec) in corpora.items():
        jplan, splan = jsonl.Plan(*spec), sls.Plan(*spec)
        d_data = torch.from_numpy(bytes_).to(dev)
        d_st = torch.from_numpy(st).to(dev)
        d_scratch = torch.empty(jsonl.scratch_bytes(jplan, n), dtype=torch.uint8, device=dev)
        d_sscratch = torch.empty(sls.scratch_bytes(n), dtype=torch.uint8, device=dev)

        def jenc(d_out, cap):
            jsonl.encode_device(jplan, d_data, d_off, None, 1, n, G, d_caps, d_st, d_time, d_head, len(head), d_out, cap, d_rec, d_scratch, stream=stream)

        def senc(d_out, cap):
            sls.encode_device(splan, d_data, d_off, None, 1, n, G, d_caps, d_st, d_time, None, 0, d_out, cap, d_rec, d_sscratch, stream=stream)
        senc(None, 0)
        torch.cuda.synchronize()
        stotal = int(d_rec[n])
        jenc(None, 0)
        torch.cuda.synchronize()
        total = int(d_rec[n])
        d_out = torch.zeros(max(total, stotal) + 64, dtype=torch.uint8, device=dev)
        d_copy = torch.empty(total, dtype=torch.uint8, device=dev)
        jenc(d_out, total)
        torch.cuda.synchronize()
        check = min(n, 2048)
        rec = d_rec[:check + 1].cpu().numpy()
        got = d_out[:int(rec[check])].cpu().numpy().tobytes()
        rows = [(bytes_[off[i]:off[i] + length[i]].tobytes(), int(st[i]), list(caps[i]), 1700000000) for i in range(check)]
        assert got == jc.model_batch(*spec, rows)[1], "%s: the first %d records differ from the model" % (name, check)
        names = ["jsonl_size_scan_write", "jsonl_size_scan_only", "sls_encode_device", "device_to_device_copy_of_the_payload"]
        timings = timed_alternating(torch, [lambda: jenc(d_out, total), lambda: jenc(d_out, 0), lambda: senc(d_out, stotal),
                                            lambda: d_copy.copy_(d_out[:total])])
        block = dict(zip(names, timings))
        full, copy_ms = block["jsonl_size_scan_write"]["median_ms"], block["device_to_device_copy_of_the_payload"]["median_ms"]
        write_ms = full - block["jsonl_size_scan_only"]["median_ms"]
        block["write_kernel_by_difference"] = {"median_ms": write_ms, "payload_GBps": total / (write_ms / 1e3) / 1e9, "over_the_copy": write_ms / copy_ms}
        block["jsonl_size_scan_write"]["over_the_copy"] = full / copy_ms
        block["jsonl_size_scan_write"]["over_the_sls_encode"] = full / block["sls_encode_device"]["median_ms"]
        block.update({"n": n, "line_bytes": LINE_BYTES, "input_bytes": int(length.sum()), "payload_bytes": total, "sls_payload_bytes": stotal,
                      "records": int((st == 1).sum()) if spec[1] else n})
        out[name] = block
        del d_out, d_copy, d_data
    return out


def agent(threads_list, groups_per_thread):
    from loongcollector_amd import binding, corpus, jsonl
    L, J = binding.load(), jsonl.load()
    config = {"SourceKey": "content", "Regex": corpus.REGEX_A, "Keys": corpus.KEYS_A}
    data, off, length = corpus.apache_batch(GROUP_LINES * 64, "A", line_bytes=LINE_BYTES)
    off32, len32 = off[:-1].astype(np.uint32), length.astype(np.uint32)

    def new_group(k):
        at = (k % 64) * GROUP_LINES
        return L.lc_group_from_lines(data.ctypes.data, off32[at:at + GROUP_LINES].ctypes.data, len32[at:at + GROUP_LINES].ctypes.data, GROUP_LINES, b"content")

    out = {}
    for threads in threads_list:
        per = groups_per_thread[threads]
        jproc = jsonl.Processor(config)
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        assert L.lc_processor_create(json.dumps(config).encode(), ctypes.byref(h), err, 512) == 0, err.value
        legs = {}
        for leg in ("jsonl_processor_serialize_device_path", "processor_process_then_host_writer"):
            device_leg = leg == "jsonl_processor_serialize_device_path"
            groups = [[new_group(t * per + k) for k in range(per)] for t in range(threads)]
            barrier = threading.Barrier(threads + 1)
            bytes_out, fused = [0] * threads, [0] * threads

            def runner(t):
                o, n, f = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
                warm = new_group(t)     # (one group outside the clock: the thread's staging, stream and tables)
                if device_leg:
                    assert J.lc_jsonl_processor_serialize(jproc._h, warm, ctypes.byref(o), ctypes.byref(n), ctypes.byref(f)) == 0
                else:
                    assert L.lc_processor_process(h, warm) == 0
                L.lc_group_free(warm)
                barrier.wait()
                for g in groups[t]:
                    if device_leg:
                        assert J.lc_jsonl_processor_serialize(jproc._h, g, ctypes.byref(o), ctypes.byref(n), ctypes.byref(f)) == 0
                        fused[t] += f.value
                    else:
                        assert L.lc_processor_process(h, g) == 0
                        assert J.lc_jsonl_serialize_group_host(g, ctypes.byref(o), ctypes.byref(n)) == 0
                    bytes_out[t] += n.value
                barrier.wait()
                J.lc_jsonl_thread_release()
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
                         "us_per_group_per_thread": dt / per * 1e6, "bytes": sum(bytes_out)}
            if device_leg:
                assert sum(fused) == threads * per, "a group left the device path"
        assert legs["jsonl_processor_serialize_device_path"]["bytes"] == legs["processor_process_then_host_writer"]["bytes"]
        legs["device_path_over_today"] = legs["jsonl_processor_serialize_device_path"]["lines_per_s"] / legs["processor_process_then_host_writer"]["lines_per_s"]
        out["threads_%d" % threads] = legs
        L.lc_processor_destroy(h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jsonl_bench.json"))
    ap.add_argument("--skip-agent", action="store_true")
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of liblc_jsonl.so (the sweep of lanes per event)")
    args = ap.parse_args()
    import torch
    from loongcollector_amd import jsonl
    if args.lib:
        jsonl.LIB_PATH = os.path.abspath(args.lib)
    result = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(jsonl.LIB_PATH),
              "timing": "engine: HIP events, 3 warm-up launches, 5 timed launches per row, rows alternating in the same run; agent: wall clock "
                        "between two barriers around all threads' groups, one group per thread before the clock",
              "not_measured": ["hardware counters", "lines of other lengths", "tags in the head"]}
    if not args.skip_engine:
        result["engine"] = engine(torch, args.n)
    if not args.skip_agent:
        result["agent"] = agent([1, 16], {1: 300, 16: 60})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    brief = {}
    if "engine" in result:
        brief["engine_ms"] = {c: {k: round(v["median_ms"], 4) for k, v in block.items() if isinstance(v, dict)} for c, block in result["engine"].items()}
    if "agent" in result:
        brief["agent_lines_per_s"] = {t: {k: round(v["lines_per_s"]) for k, v in legs.items() if isinstance(v, dict)} for t, legs in result["agent"].items()}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
