"""Measures the anchor processor on an MI355X -> profiles/anchor_bench.json.

    python tools/anchor_bench.py [--n 1048576] [--out profiles/anchor_bench.json]

* the corpus: 1 Mi lines of exactly 512 bytes, 16 fields each (`k00=text;k01=text;...`, 8192 distinct lines, tiled), resident in device
  memory.  Anchor a is Start `kAA=` / Stop `;`, so 1, 4 and 16 anchors per line end in the line's first 32, 128 and 512 bytes; one more
  row takes ONE anchor that is the line's LAST field, so that no wavefront can leave early.
* kernels: HIP events, 3 warm-up launches, 5 timed launches (five windows), min / median / max; everything that is compared is timed in
  the SAME run, alternating, on the same bytes:
    - anchor_locate_kernel at 1, 4, 16 anchors and at the one last-field anchor,
    - a device-to-device copy of the corpus,
    - delim_split_kernel with `;` as its separator, 16 columns kept,
    - lc_regex_match_device with `.*?k00=(.*?);.*` (the one-anchor case as a regex; the engine matches whole lines, hence the frame).
* the early exit: 96 Ki lines of 512 bytes against 96 Ki lines of 16 KiB, four anchors, all of them in the first 64 bytes.
* the first 8192 lines of every anchor row are compared with tests/helpers/anchor_model.py, the regex row with the anchor row, before
  anything is written.
* the host: the per-value routine (csrc/anchor_vm.hpp compiled for the host, through the tests' double, which copies every value into an
  exactly-sized block first) on one thread, and 1000-log groups through lc_anchor_process_logs_json from 1 and from 16 threads.
Not measured here: rocprofv3 traces and hardware counters.
"""
import argparse
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

LINE_BYTES, FIELDS, UNIQUE = 512, 16, 8192


def corpus_lines(line_bytes=LINE_BYTES, seed=13):
    """UNIQUE lines of exactly line_bytes bytes: FIELDS fields of 32 bytes `kAA=<27 letters>;`, the rest filled with letters"""
    rng, out = random.Random(seed), []
    letters = "abcdefghijlmnopqrstuvwxyz0123456789_-./ "  # (no k, = or ;)
    for _ in range(UNIQUE):
        line = "".join("k%02d=%s;" % (a, "".join(rng.choice(letters) for _ in range(27))) for a in range(FIELDS))
        line += "".join(rng.choice(letters) for _ in range(line_bytes - len(line)))
        assert len(line) == line_bytes
        out.append(line.encode())
    return out


def front_lines(line_bytes, seed=17):
    """UNIQUE lines whose four fields all lie in the first 64 bytes"""
    rng, out = random.Random(seed), []
    letters = "abcdefghijlmnopqrstuvwxyz0123456789_-./ "
    for _ in range(UNIQUE):
        line = "".join("k%02d=%s;" % (a, "".join(rng.choice(letters) for _ in range(rng.randint(4, 10)))) for a in range(4))
        assert len(line) <= 64
        line += "".join(rng.choice(letters) for _ in range(512 - len(line)))
        out.append((line + "." * (line_bytes - 512)).encode())
    return out


def anchors(names):
    return {"Anchors": [{"Start": "k%02d=" % a, "Stop": ";", "FieldName": "f%02d" % a} for a in names]}


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


def rates(k, n, nbytes):
    k["GBps"] = nbytes / (k["median_ms"] / 1e3) / 1e9
    k["ps_per_byte"] = k["median_ms"] * 1e9 / nbytes
    k["ns_per_value"] = k["median_ms"] * 1e6 / n
    return k


def resident(torch, dev, uniq, n, line_bytes):
    total = n * line_bytes
    assert total < 2 ** 31
    tile = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev)
    d_data = torch.cat([tile.repeat((n + UNIQUE - 1) // UNIQUE)[:total], torch.zeros(16, dtype=torch.uint8, device=dev)])
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev).mul_(line_bytes).to(torch.int32)
    return d_data, d_off, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_bench.json"))
    args = ap.parse_args()
    import torch
    from helpers import anchor_cases as ac
    from loongcollector_amd import anchor, binding, delimiter
    dev = torch.device("cuda:0")
    n = args.n
    stream = torch.cuda.current_stream().cuda_stream
    result = {"device": torch.cuda.get_device_name(0), "n": n, "line_bytes": LINE_BYTES, "fields_per_line": FIELDS,
              "timing": "HIP events, 3 warm-up launches, 5 timed launches per row, rows of one corpus alternating in the same run",
              "not_measured": ["rocprofv3 kernel trace", "hardware counters"]}

    def verify(config, spans, uniq, what):
        got = spans[:min(UNIQUE, spans.shape[0])].cpu().numpy()
        for i, v in enumerate(uniq[:len(got)]):
            want = ac.rows_of(ac.rows_text(config, v), got.shape[1])
            assert np.array_equal(got[i], want), (what, i)

    # ---- 1 Mi x 512 B
    uniq = corpus_lines()
    d_data, d_off, total = resident(torch, dev, uniq, n, LINE_BYTES)
    result["bytes"] = total
    d_copy = torch.empty_like(d_data)
    rows = {"anchors_1": anchors([0]), "anchors_4": anchors(range(4)), "anchors_16": anchors(range(16)), "anchors_1_last_field": anchors([15])}
    procs = {k: anchor.Processor(**c) for k, c in rows.items()}
    spans = {k: torch.empty((n, p.stride, 2), dtype=torch.int32, device=dev) for k, p in procs.items()}
    dl = delimiter.GpuDelimiter(b";", b";", "extend", 1)  # (Quote == Separator: its plain path, every `;` splits)
    s_st = torch.empty(n, dtype=torch.uint8, device=dev)
    s_nc = torch.empty(n, dtype=torch.int32, device=dev)
    s_sp = torch.empty((n, 16, 2), dtype=torch.int32, device=dev)
    rx = binding.GpuRegex(r".*?k00=(.*?);.*")
    r_caps = torch.empty((n, 2 * rx.groups), dtype=torch.int32, device=dev)
    r_st = torch.empty(n, dtype=torch.uint8, device=dev)
    fns = {k: (lambda k=k: anchor.locate_device(procs[k], d_data, d_off, n, spans[k], stream=stream)) for k in rows}
    fns["device_to_device_copy"] = lambda: d_copy.copy_(d_data)
    fns["delim_split_kernel_same_bytes"] = lambda: dl.split_device(d_data, d_off, n, 16, s_st, s_nc, s_sp, stream=stream)
    fns["regex_match_device_one_anchor"] = lambda: rx.match_device(d_data, d_off, None, n, r_caps, r_st, sep_bytes=0, stream=stream)
    binding.launched_kernels()
    for k in rows:
        fns[k]()
        torch.cuda.synchronize()
        verify(rows[k], spans[k], uniq, k)
    fns["regex_match_device_one_anchor"]()
    torch.cuda.synchronize()
    result["regex_engine"] = rx.info()["engine"]
    caps = r_caps[:UNIQUE].cpu().numpy()
    assert int(r_st.min()) == 1 and np.array_equal(caps[:, -2:], spans["anchors_1"][:UNIQUE, 0].cpu().numpy()), "the regex row computes another field"
    timings = timed_alternating(torch, list(fns.values()))
    result["kernels_launched"] = binding.launched_kernels()
    assert int(s_nc[0]) >= FIELDS, "the delimiter kernel did not split the corpus"
    block = {k: rates(t, n, total) for k, t in zip(fns, timings)}
    for k in rows:
        for base in ("device_to_device_copy", "delim_split_kernel_same_bytes", "regex_match_device_one_anchor"):
            block[k]["over_" + base] = block[k]["median_ms"] / block[base]["median_ms"]
    result["lines_512"] = block
    del d_copy, spans, s_sp, r_caps

    # ---- the early exit: 96 Ki lines of 512 B against 96 Ki lines of 16 KiB, four anchors in the first 64 bytes
    m = min(96 << 10, n)
    cfg4 = anchors(range(4))
    p4 = anchor.Processor(**cfg4)
    exit_block = {}
    for name, line_bytes in (("lines_512", 512), ("lines_16384", 16384)):
        fu = front_lines(line_bytes)
        f_data, f_off, f_total = resident(torch, dev, fu, m, line_bytes)
        f_spans = torch.empty((m, p4.stride, 2), dtype=torch.int32, device=dev)
        f_copy = torch.empty_like(f_data)
        anchor.locate_device(p4, f_data, f_off, m, f_spans, stream=stream)
        torch.cuda.synchronize()
        verify(cfg4, f_spans, fu, "early exit / " + name)
        t = timed_alternating(torch, [lambda: anchor.locate_device(p4, f_data, f_off, m, f_spans, stream=stream), lambda: f_copy.copy_(f_data)])
        exit_block[name] = {"n": m, "bytes": f_total, "anchor_locate_kernel": rates(t[0], m, f_total), "device_to_device_copy": rates(t[1], m, f_total)}
        del f_data, f_copy, f_spans
    exit_block["time_16384_over_512"] = exit_block["lines_16384"]["anchor_locate_kernel"]["median_ms"] / exit_block["lines_512"]["anchor_locate_kernel"]["median_ms"]
    exit_block["bytes_16384_over_512"] = 32.0
    result["early_exit_4_anchors_in_first_64_bytes"] = exit_block

    # ---- the host: the routine on one thread, the processor from 1 and 16 threads
    from helpers import anchor_product as apd
    lines = uniq[:4096]
    host = {}
    for k in ("anchors_1", "anchors_4", "anchors_16"):
        cpu = apd.processor(**rows[k])
        blob = np.frombuffer(b"".join(lines), np.uint8).copy()
        lens = np.full(len(lines), LINE_BYTES, np.uint32)
        ptrs = (blob.ctypes.data + np.arange(len(lines), dtype=np.uint64) * LINE_BYTES).astype(np.uint64)
        out = np.zeros((len(lines), cpu.stride, 2), np.int32)
        best = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            assert apd.double().lc_anchor_locate_host(cpu.handle, ptrs.ctypes.data, lens.ctypes.data, len(lines), out.ctypes.data) == 0
            best = min(best, time.perf_counter() - t0)
        host[k] = {"values": len(lines), "best_of_5_s": best, "ns_per_value": best * 1e9 / len(lines), "MBps": len(lines) * LINE_BYTES / best / 1e6}
    result["host_routine_one_thread"] = dict(host, note="anchorLocate() compiled for the host behind the tests' double, which copies every value first")
    group = [[("host", "h"), ("content", v.decode())] for v in uniq[:1000]]
    proc_block = {}
    for threads in (1, 16):
        ps = [anchor.Processor(SourceKey="content", **rows["anchors_4"]) for _ in range(threads)]
        groups_each = 20
        for p in ps:
            p.process_logs(group)  # (warm: staging, stream)
        def work(p):
            for _ in range(groups_each):
                p.process_logs(group)
        t0 = time.perf_counter()
        ts = [threading.Thread(target=work, args=(p,)) for p in ps]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        dt = time.perf_counter() - t0
        proc_block["threads_%d" % threads] = {"groups": threads * groups_each, "logs_per_group": 1000, "seconds": dt,
                                              "logs_per_second": threads * groups_each * 1000 / dt}
    proc_block["note"] = "lc_anchor_process_logs_json through the Python binding, 4 anchors, 512-byte values: the JSON form both ways is inside the time"
    result["processor_1000_log_groups"] = proc_block

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"lines_512": {k: round(v["median_ms"], 4) for k, v in block.items()},
                      "early_exit": {k: round(exit_block[k]["anchor_locate_kernel"]["median_ms"], 4) for k in ("lines_512", "lines_16384")},
                      "processor": {k: round(v["logs_per_second"]) for k, v in proc_block.items() if k != "note"}}))


if __name__ == "__main__":
    main()
