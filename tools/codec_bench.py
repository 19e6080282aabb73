"""Measures the field codecs (base64 encode / decode, MD5) on an MI355X -> profiles/codec_bench.json.

    python tools/codec_bench.py [--n 1048576] [--out profiles/codec_bench.json] [--lib liblc_codec_variant.so] [--cases a,b]
    python tools/codec_bench.py --only encode --calls 5       # nothing but that case's calls: the run to put under a kernel trace

* the corpus: 1 Mi values of exactly 512 bytes of text (8192 distinct ones, tiled), resident in device memory.  Four cases:
    - encode          the 512-byte values -> 684 characters each (688 bytes of d_out: a value's output begins 16-byte aligned),
    - decode_clean    that encode's output,
    - decode_mime     the same payload as MIME lines (76 characters + CRLF),
    - md5             the 512-byte values -> 32 hex digits each.
* every case is timed against yardsticks on the SAME batch in the same run, alternating (HIP events, 3 warm-up calls, 5 timed, the
  spread reported):
    - a device-to-device copy of (input + output) bytes, one call,
    - delim_split_kernel with `;` as its separator,
    - lc_strrep_apply_device, const with a Match that does not occur: the cheapest rewrite stage there was,
    - (md5 only) lc_desens_apply_device, method md5, with a rule that matches the whole value behind its first byte,
  and, apart from them, the host routine of csrc/codec_vm.hpp on one CPU thread over the first 65536 values (wall clock, scaled).
  lc_codec_apply_device is timed as a CALL: its waits for the stream (the batch's extent, the total) are inside.
* the first 8192 values of every case are compared with CPython's base64 / hashlib before anything is written.
Not measured here: hardware counters, the size / write split of a call (run --only under a kernel trace).
"""
import argparse
import base64
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VALUE_BYTES, UNIQUE, HOST_VALUES = 512, 8192, 65536
LETTERS = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789 .,:-_/"


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


def plain_value(i):
    body = ("v%07d;" % i).encode()
    rnd = np.random.RandomState(i)
    return body + bytes(LETTERS[k] for k in rnd.randint(0, len(LETTERS), VALUE_BYTES - len(body)))


def mime(value):
    return base64.encodebytes(value).replace(b"\n", b"\r\n")


def cases():
    plain = [plain_value(i) for i in range(UNIQUE)]
    return {
        "encode": ("base64_encode", plain, [base64.b64encode(v) for v in plain]),
        "decode_clean": ("base64_decode", [base64.b64encode(v) for v in plain], plain),
        "decode_mime": ("base64_decode", [mime(v) for v in plain], plain),
        "md5": ("md5", plain, [hashlib.md5(v).hexdigest().encode() for v in plain]),
    }


def host_routine_ms(op, values):
    """the host walk of csrc/codec_vm.hpp (the tests' double of the device trip, g++ -O2) over `values`, one thread, wall clock"""
    from helpers import codec_product as cp
    p = cp.processor(Op=op)
    n = len(values)
    blob = np.frombuffer(b"".join(values) + b"\0", np.uint8).copy()
    lens = np.array([len(v) for v in values], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens[:-1])
    ptrs = (blob.ctypes.data + off).astype(np.uint64)
    flags, err_off, out_off, out_len = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.zeros(n, np.uint32)
    best = None
    for _ in range(3):
        out = ctypes.c_void_p()
        t = time.perf_counter()
        rc = p._L.lc_codec_apply_host(p.handle, ptrs.ctypes.data, lens.ctypes.data, n, flags.ctypes.data, err_off.ctypes.data, out_off.ctypes.data,
                                      out_len.ctypes.data, ctypes.byref(out))
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0
        p._L.lc_codec_free_string(out)
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_bench.json"))
    ap.add_argument("--lib", default=None, help="another build of liblc_codec.so (-DLC_CODEC_LANES=..) to time instead")
    ap.add_argument("--only", default=None, help="run nothing but this case's lc_codec_apply_device calls (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cases", default=None, help="comma-separated case names: time only these")
    args = ap.parse_args()
    import torch
    from loongcollector_amd import abi, binding, codec, delimiter, desensitize, string_replace as sr
    dev = torch.device("cuda:0")
    n = args.n
    binding.load()
    L = abi.bind(ctypes.CDLL(args.lib), abi.CODEC_PROTOTYPES) if args.lib else codec.load()
    stream = torch.cuda.current_stream().cuda_stream
    result = {"device": torch.cuda.get_device_name(0), "n": n, "value_bytes": VALUE_BYTES, "library": args.lib or "liblc_codec.so",
              "timing": "HIP events around whole calls, 3 warm-up calls, 5 timed calls per row, rows of one batch alternating in the same run",
              "copy": "one device-to-device copy of (input + output) bytes",
              "host_routine": "codec_vm.hpp's host walk, g++ -O2, one thread, best of 3 over %d values, scaled to n" % HOST_VALUES,
              "not_measured": ["hardware counters", "the size / write split of a call"], "cases": {}}
    needed = ctypes.c_uint64(0)
    nothing = sr.Processor(SourceKey="k", Method="const", Match="#", ReplaceString="")
    for name, (op, uniq, expect) in cases().items():
        if (args.only and name != args.only) or (args.cases and name not in args.cases.split(",")):
            continue
        each = len(uniq[0])
        assert all(len(v) == each for v in uniq)
        total = n * each
        assert total < 2 ** 31
        tile = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev)
        d_data = torch.cat([tile.repeat((n + UNIQUE - 1) // UNIQUE)[:total], torch.zeros(16, dtype=torch.uint8, device=dev)])
        d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev).mul_(each).to(torch.int32)
        d_flags = torch.empty(n, dtype=torch.uint8, device=dev)
        d_err = torch.empty(n, dtype=torch.int32, device=dev)
        d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_out_len = torch.empty(n, dtype=torch.int32, device=dev)
        out_each = (len(expect[0]) + 15) // 16 * 16
        d_out = torch.empty(n * out_each + 16, dtype=torch.uint8, device=dev)
        p = codec.Processor(lib=L, Op=op)

        def run():
            rc = L.lc_codec_apply_device(p.handle, d_data.data_ptr(), d_off.data_ptr(), n, d_flags.data_ptr(), d_err.data_ptr(), d_out_off.data_ptr(),
                                         d_out_len.data_ptr(), d_out.data_ptr(), d_out.numel(), ctypes.byref(needed), stream)
            assert rc == 0, rc
        binding.launched_kernels()
        run()
        torch.cuda.synchronize()
        launched = binding.launched_kernels()
        m = min(UNIQUE, n)
        flags, offs, lens = d_flags[:m].cpu().numpy(), d_out_off[:m + 1].cpu().numpy(), d_out_len[:m].cpu().numpy()
        out = d_out[:int(offs[m])].cpu().numpy()
        for i in range(m):
            assert int(flags[i]) == 1 and out[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes() == expect[i], (name, i)
        if args.only:
            for _ in range(args.calls):
                run()
            torch.cuda.synchronize()
            print(json.dumps({"case": name, "calls": args.calls + 1, "output_bytes": int(needed.value)}))
            return
        out_bytes = int(needed.value)
        d_src, d_dst = torch.empty(total + out_bytes, dtype=torch.uint8, device=dev), torch.empty(total + out_bytes, dtype=torch.uint8, device=dev)
        fns = {"lc_codec_apply_device": run, "device_to_device_copy": lambda: d_dst.copy_(d_src)}
        dl = delimiter.GpuDelimiter(b";", b";", "extend", 1)  # (Quote == Separator: its plain path, every `;` splits)
        s_st = torch.empty(n, dtype=torch.uint8, device=dev)
        s_nc = torch.empty(n, dtype=torch.int32, device=dev)
        s_sp = torch.empty((n, 16, 2), dtype=torch.int32, device=dev)
        fns["delim_split_kernel_same_bytes"] = lambda: dl.split_device(d_data, d_off, n, 16, s_st, s_nc, s_sp, stream=stream)
        r_flags, r_off = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
        r_needed = ctypes.c_uint64(0)

        def strrep_nothing():
            rc = sr.load().lc_strrep_apply_device(nothing.handle, d_data.data_ptr(), d_off.data_ptr(), n, r_flags.data_ptr(), r_off.data_ptr(), None, 0,
                                                  ctypes.byref(r_needed), stream)
            assert rc == 0 and r_needed.value == 0, (rc, r_needed.value)
        fns["lc_strrep_apply_device_no_occurrence"] = strrep_nothing
        block = {"op": op, "input_bytes": total, "output_bytes": out_bytes, "kernels_launched": launched}
        if name == "md5":
            try:
                ds = desensitize.GpuDesensitize("md5", "v", ".*")
                x_flags, x_off = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
                x_out = torch.empty(total + 64, dtype=torch.uint8, device=dev)
                desens = lambda: ds.apply_device(d_data, d_off, None, n, x_flags, x_off, x_out, stream=stream)  # noqa: E731
                desens()
                torch.cuda.synchronize()
                got = x_out[:33].cpu().numpy().tobytes()
                assert got == b"v" + hashlib.md5(uniq[0][1:]).hexdigest().upper().encode(), got
                fns["lc_desens_apply_device_md5_whole_value"] = desens
            except Exception as e:  # the row is named as not measured, with the reason
                block["lc_desens_apply_device_md5_whole_value"] = {"not_measured": repr(e)[:300]}
        timings = dict(zip(fns, timed_alternating(torch, list(fns.values()))))
        for k, t in timings.items():
            t["GBps_of_input"] = total / (t["median_ms"] / 1e3) / 1e9
            block[k] = t
        for base in list(fns)[1:]:
            block["over_" + base] = timings["lc_codec_apply_device"]["median_ms"] / timings[base]["median_ms"]
        host_n = min(HOST_VALUES, n)
        host_ms = host_routine_ms(op, [uniq[i % UNIQUE] for i in range(host_n)])
        block["host_routine_one_thread"] = {"values": host_n, "ms": host_ms, "ms_scaled_to_n": host_ms * n / host_n,
                                            "MBps_of_input": host_n * each / (host_ms / 1e3) / 1e6}
        block["over_host_routine_one_thread"] = timings["lc_codec_apply_device"]["median_ms"] / (host_ms * n / host_n)
        result["cases"][name] = block
        print(name, {k: round(v["median_ms"], 3) for k, v in timings.items()}, "host %.1f ms" % (host_ms * n / host_n), flush=True)
        del d_data, d_out, d_src, d_dst, s_sp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: round(v["lc_codec_apply_device"]["median_ms"], 3) for k, v in result["cases"].items()}))


if __name__ == "__main__":
    main()
