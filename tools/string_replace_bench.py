"""Measures the string-replace processor on an MI355X -> profiles/string_replace_bench.json.

    python tools/string_replace_bench.py [--n 1048576] [--out profiles/string_replace_bench.json] [--lib liblc_strrep_variant.so] [--cases a,b]
    python tools/string_replace_bench.py --only const_1_x10 --calls 5          # nothing but that case's calls: the run to put under
                                                                               # rocprofv3 --kernel-trace --stats for the size / write split

* the corpus: 1 Mi values of exactly 512 bytes (8192 distinct ones, tiled), resident in device memory, one batch per case:
    - const with a 1-byte and a 16-byte Match, ReplaceString "", at 0, 1 and 10 occurrences per value,
    - unquote on the reference's benchmark shapes: the three bytes backslash backslash underscore x 1, x 10, x 100 per value, padded with `a`,
    - unquote on the nginx shape of the reference's unquote1 case (its value repeated, padded with `a`).
* every case is timed against three yardsticks on the SAME batch in the same run, alternating (HIP events, 3 warm-up calls, 5 timed):
    - a device-to-device copy of the input bytes,
    - delim_split_kernel with `;` as its separator,
    - (const only) lc_desens_apply_device with the literal as its pattern doing the same replacement: the only way to rewrite on the
      device before this processor.
  lc_strrep_apply_device is timed as a CALL: its two waits for the stream (the batch's extent, the total) are inside.
* the first 8192 values of every case are compared with tests/helpers/strrep_model.py before anything is written.
Not measured here: hardware counters.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VALUE_BYTES, UNIQUE = 512, 8192
NEEDLE_1, NEEDLE_16 = "#", "NEEDLE16BYTESxyz"


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


def padded(i, pieces):
    """a 512-byte value: a counter, the pieces spread evenly, letters between them (no needle, no backslash, no quote, no `;` but one)"""
    body = ("v%07d;" % i).encode()
    room = VALUE_BYTES - len(body) - sum(len(p) for p in pieces)
    gap, out = room // (len(pieces) + 1), [body]
    for p in pieces:
        out += [b"a" * gap, p]
    value = b"".join(out)
    return value + b"a" * (VALUE_BYTES - len(value))


def cases(unquote1):
    from helpers import strrep_cases as sc
    out = {}
    for name, needle in (("const_1", NEEDLE_1), ("const_16", NEEDLE_16)):
        for count in (0, 1, 10):
            out["%s_x%d" % (name, count)] = (sc.const(needle, ""), [padded(i, [needle.encode()] * count) for i in range(UNIQUE)])
    for count in (1, 10, 100):  # benchmarkReplace: the groups in front, then the padding
        out["unquote_double_dash_x%d" % count] = (sc.UNQUOTE, [(b"\\\\_" * count + ("%07d" % i).encode()).ljust(VALUE_BYTES, b"a") for i in range(UNIQUE)])
    reps = VALUE_BYTES // len(unquote1)
    out["unquote_nginx"] = (sc.UNQUOTE, [(unquote1 * reps + ("%07d" % i).encode()).ljust(VALUE_BYTES, b"a") for i in range(UNIQUE)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_replace_bench.json"))
    ap.add_argument("--lib", default=None, help="another build of liblc_strrep.so (-DLC_STRREP_LANES=..) to time instead")
    ap.add_argument("--only", default=None, help="run nothing but this case's lc_strrep_apply_device calls (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cases", default=None, help="comma-separated case names: time only these")
    args = ap.parse_args()
    import torch
    from helpers import strrep_cases as sc
    from helpers import strrep_model as model
    from loongcollector_amd import abi, binding, delimiter, desensitize, string_replace as sr
    dev = torch.device("cuda:0")
    n = args.n
    binding.load()
    L = abi.bind(ctypes.CDLL(args.lib), abi.STRREP_PROTOTYPES) if args.lib else sr.load()
    stream = torch.cuda.current_stream().cuda_stream
    unquote1 = sc.load_vectors()["cases"][1]["log"][0][1].encode()
    result = {"device": torch.cuda.get_device_name(0), "n": n, "value_bytes": VALUE_BYTES, "bytes": n * VALUE_BYTES, "library": args.lib or "liblc_strrep.so",
              "timing": "HIP events around whole calls, 3 warm-up calls, 5 timed calls per row, rows of one batch alternating in the same run",
              "not_measured": ["hardware counters"], "cases": {}}
    total = n * VALUE_BYTES
    assert total < 2 ** 31
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev).mul_(VALUE_BYTES).to(torch.int32)
    d_flags = torch.empty(n, dtype=torch.uint8, device=dev)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_out = torch.empty(total + 16, dtype=torch.uint8, device=dev)  # (no case here grows a value)
    d_copy = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    needed = ctypes.c_uint64(0)
    for name, (config, uniq) in cases(unquote1).items():
        if (args.only and name != args.only) or (args.cases and name not in args.cases.split(",")):
            continue
        tile = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev)
        d_data = torch.cat([tile.repeat((n + UNIQUE - 1) // UNIQUE)[:total], torch.zeros(16, dtype=torch.uint8, device=dev)])
        p = sr.Processor(lib=L, **config)

        def strrep():
            rc = L.lc_strrep_apply_device(p.handle, d_data.data_ptr(), d_off.data_ptr(), n, d_flags.data_ptr(), d_out_off.data_ptr(), d_out.data_ptr(),
                                          d_out.numel(), ctypes.byref(needed), stream)
            assert rc == 0, rc
        binding.launched_kernels()
        strrep()
        torch.cuda.synchronize()
        launched = binding.launched_kernels()
        m = min(UNIQUE, n)
        flags, offs = d_flags[:m].cpu().numpy(), d_out_off[:m + 1].cpu().numpy()
        out = d_out[:int(offs[m])].cpu().numpy()
        for i in range(m):
            want_flags, want = model.apply(config, uniq[i])
            assert int(flags[i]) == want_flags and out[int(offs[i]):int(offs[i + 1])].tobytes() == (want or b""), (name, i)
        if args.only:
            for _ in range(args.calls):
                strrep()
            torch.cuda.synchronize()
            print(json.dumps({"case": name, "calls": args.calls + 1, "output_bytes": int(needed.value)}))
            return
        fns = {"lc_strrep_apply_device": strrep, "device_to_device_copy": lambda: d_copy.copy_(d_data)}
        dl = delimiter.GpuDelimiter(b";", b";", "extend", 1)  # (Quote == Separator: its plain path, every `;` splits)
        s_st = torch.empty(n, dtype=torch.uint8, device=dev)
        s_nc = torch.empty(n, dtype=torch.int32, device=dev)
        s_sp = torch.empty((n, 16, 2), dtype=torch.int32, device=dev)
        fns["delim_split_kernel_same_bytes"] = lambda: dl.split_device(d_data, d_off, n, 16, s_st, s_nc, s_sp, stream=stream)
        if config["Method"] == "const":
            ds = desensitize.GpuDesensitize("const", "", config["Match"], config["ReplaceString"], replacing_all=True)
            x_flags, x_off = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
            x_out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
            fns["lc_desens_apply_device_same_job"] = lambda: ds.apply_device(d_data, d_off, None, n, x_flags, x_off, x_out, stream=stream)
            fns["lc_desens_apply_device_same_job"]()
            torch.cuda.synchronize()
            assert torch.equal(x_off, d_out_off) and torch.equal(x_out[:int(needed.value)], d_out[:int(needed.value)]), "the desensitize route computes other bytes"
        timings = dict(zip(fns, timed_alternating(torch, list(fns.values()))))
        block = {"config": config, "output_bytes": int(needed.value), "kernels_launched": launched}
        for k, t in timings.items():
            t["GBps_of_input"] = total / (t["median_ms"] / 1e3) / 1e9
            block[k] = t
        for base in list(fns)[1:]:
            block["over_" + base] = timings["lc_strrep_apply_device"]["median_ms"] / timings[base]["median_ms"]
        result["cases"][name] = block
        print(name, {k: round(v["median_ms"], 3) for k, v in timings.items()}, flush=True)
        del d_data, s_sp
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: round(v["lc_strrep_apply_device"]["median_ms"], 3) for k, v in result["cases"].items()}))


if __name__ == "__main__":
    main()
