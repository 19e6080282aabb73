"""processor_string_replace on the device: strrep_size_kernel, the scan and strrep_write_kernel through lc_strrep_apply_device and
lc_strrep_apply_host against tests/helpers/strrep_model.py -- occurrences, escapes and UTF-8 sequences on chosen tile offsets for every
residue of the value's first byte, the self-overlapping needles, every error rule, value lengths 0-65, short last wavefronts, one long
value in a wavefront, batches in which nothing / everything changes, the overflow contract, sentinel bytes around every output array,
argument errors -- and the processor on a 1000-log batch against the CPU double.

Every batch goes through the device entry TWICE: with no room at all (LC_ERR_OVERFLOW unless nothing changed; flags, offsets and
`needed` must be right already) and again with exactly `needed` bytes between two rows of sentinel bytes."""
import ctypes
import functools
import json
import random

import numpy as np
import pytest

from helpers import strrep_cases as sc
from helpers import strrep_model as model
from loongcollector_amd import string_replace as sr

pytestmark = pytest.mark.gpu
SENT = 0xA5
GUARD = 64  # sentinel bytes before and behind d_flags, d_out_off and d_out
FILL = b"."  # no needle holds it, nothing to decode
LC_OK, LC_ERR_ARG, LC_ERR_OVERFLOW = 0, 5, 6


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@functools.lru_cache(maxsize=None)
def _proc(config_json):
    return sr.Processor(**json.loads(config_json))


def proc(config):
    return _proc(json.dumps(config, sort_keys=True))


def junk(config, n):
    """n bytes the kernels would react to: Match's first byte, or backslashes"""
    first = config["Match"].encode("utf-8")[:1] if config["Method"] == "const" else b"\\"
    return first * n


def pack(config, values, pad_front=0):
    """values back to back behind pad_front bytes -> (data uint8, padded to whole 16-byte units with bytes the kernels would react to, off)"""
    blob = junk(config, pad_front) + b"".join(values)
    size = max((len(blob) + 15) // 16 * 16 + 16, 16)
    data = np.frombuffer(blob + junk(config, size - len(blob)), np.uint8).copy()
    off = np.zeros(len(values) + 1, np.uint32)
    off[1:] = np.cumsum([len(v) for v in values])
    return data, (off + pad_front).astype(np.int32)


def at_residues(wanted):
    """wanted: [(residue of its first byte, value)] -> values with filler values between them so that every wanted one begins at its
    residue (the fillers are rewritten and compared like every other value)"""
    values, at = [], 0
    for residue, value in wanted:
        gap = (residue - at) % 16
        if gap:
            values.append(FILL * gap)
            at += gap
        values.append(value)
        at += len(value)
    return values


class Guarded:
    """an array between two rows of sentinel bytes, itself pre-filled with the sentinel"""

    def __init__(self, torch, nbytes):
        self.n = nbytes
        self.full = torch.full((2 * GUARD + nbytes + 8,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.full.data_ptr() % 8 == 0
        self.ptr = self.full.data_ptr() + GUARD

    def bytes(self, what):
        raw = self.full.cpu().numpy()
        assert (raw[:GUARD] == SENT).all() and (raw[GUARD + self.n:] == SENT).all(), "a sentinel byte around %s was written" % what
        return raw[GUARD:GUARD + self.n]


def device_apply(torch, config, data, off, cap="needed"):
    """-> (rc of the last call, flags, out_off, out bytes, needed).  cap: "needed", or the out_cap of the one call to make"""
    n = len(off) - 1
    p = proc(config)
    L = sr.load()
    d_data, d_off = torch.from_numpy(data).to("cuda:0"), torch.from_numpy(off).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    needed = ctypes.c_uint64(0)

    def call(out_cap, out_ptr):
        flags, out_off = Guarded(torch, n), Guarded(torch, 8 * (n + 1))
        rc = L.lc_strrep_apply_device(p.handle, d_data.data_ptr(), d_off.data_ptr(), n, flags.ptr, out_off.ptr, out_ptr, out_cap, ctypes.byref(needed), stream)
        torch.cuda.synchronize()
        return rc, flags.bytes("d_flags").copy(), out_off.bytes("d_out_off").view(np.uint64).copy()

    if cap != "needed":
        out = Guarded(torch, cap)
        rc, flags, out_off = call(cap, out.ptr)
        return rc, flags, out_off, out.bytes("d_out").copy(), int(needed.value)
    rc0, flags0, off0 = call(0, None)
    want = int(needed.value)
    assert rc0 == (LC_ERR_OVERFLOW if want else LC_OK) and int(off0[n]) == want
    out = Guarded(torch, want)
    rc, flags, out_off = call(want, out.ptr)
    assert rc == LC_OK and int(needed.value) == want
    assert np.array_equal(flags, flags0) and np.array_equal(out_off, off0), "the repeated call disagrees with the one that overflowed"
    return rc, flags, out_off, out.bytes("d_out").copy(), want


def against_model(config, values, flags, out_off, out, what):
    assert int(out_off[0]) == 0 and len(out) == int(out_off[len(values)])
    for i, value in enumerate(values):
        want_flags, want = model.apply(config, value)
        got = out[int(out_off[i]):int(out_off[i + 1])].tobytes()
        assert int(flags[i]) == want_flags, (what, i, value[:120], int(flags[i]), want_flags)
        assert got == (want if want_flags & model.CHANGED else b""), (what, i, value[:120], got[:160], want)


def check(torch, config, values, pad_front=0, what="device"):
    data, off = pack(config, values, pad_front)
    _, flags, out_off, out, _ = device_apply(torch, config, data, off)
    against_model(config, values, flags, out_off, out, what)
    return flags


def check_host_entry(config, values, what):
    flags, outs = sr.apply_host(proc(config), values)
    assert [(int(f), o) for f, o in zip(flags, outs)] == [model.apply(config, v) for v in values], what


def by_config(cases):
    groups = {}
    for config, residue, value in cases:
        groups.setdefault(json.dumps(config, sort_keys=True), []).append((residue, value))
    return [(json.loads(k), v) for k, v in groups.items()]


def run_groups(torch, cases, what, host_every=0):
    for k, (config, wanted) in enumerate(by_config(cases)):
        values = at_residues(wanted)
        check(torch, config, values, pad_front=0, what="%s %s" % (what, config.get("Match", "unquote")))
        if host_every and k % host_every == 0:
            check_host_entry(config, values, what + ", host entry")


def test_reference_unit_test_values_and_kernel_names():
    torch = _torch()
    sr.binding.launched_kernels()
    for e in sc.load_vectors()["cases"]:
        value = e["log"][0][1].encode("utf-8")
        check(torch, e["config"], [value], what=e["case"])
        assert model.result(e["config"], value) == e["contents"][0][1].encode("utf-8")
    names = sr.binding.launched_kernels()
    assert "strrep_size_kernel" in names and "strrep_write_kernel" in names and "scan64_kernel" in names


def test_const_occurrences_on_the_borders_for_every_residue():
    """the first and the last byte of an occurrence on tile offsets 15/16/17, 63/64/65, 127/128/129, all 16 residues, needles of 1, 2, 3,
    16, 17 and 32 bytes"""
    torch = _torch()
    cases = sc.const_border_cases()
    assert len({c["Match"] for c, _, _ in cases}) == 6 and len(cases) > 1300
    run_groups(torch, cases, "const borders", host_every=3)


def test_const_occurrence_shapes():
    """near misses, occurrences cut by the value's end, back to back across a border, `aa` and `aba` on runs whose cover crosses the
    border, ReplaceString empty / shorter / equal / longer, values that are only occurrences"""
    torch = _torch()
    cases = sc.const_shape_cases()
    assert any(c["Match"] == "aa" for c, _, _ in cases) and any(c["Match"] == "aba" for c, _, _ in cases)
    assert {len(c["ReplaceString"]) for c, _, _ in cases} >= {0, 1, 2, 64, 256}
    run_groups(torch, cases, "const shapes", host_every=7)


def test_unquote_escapes_and_backslash_runs_on_the_borders():
    torch = _torch()
    cases = sc.unquote_border_cases()
    assert (sc.UNQUOTE, 0, b'a\\"b') in cases and model.apply(sc.UNQUOTE, b'a\\"b') == (model.CHANGED, b"a\\x22b")
    run_groups(torch, cases, "unquote borders", host_every=1)


def test_unquote_errors():
    torch = _torch()
    cases = sc.unquote_error_cases()
    flags = check(torch, sc.UNQUOTE, at_residues([(r, v) for _, r, v in cases]), what="unquote errors")
    assert (flags == model.ERROR).sum() >= len(cases) - 10  # (a few of the bordered ones decode: the model says which)


def test_unquote_utf8():
    torch = _torch()
    cases = sc.unquote_utf8_cases()
    assert model.apply(sc.UNQUOTE, b"\xff" * 64) == (model.CHANGED, b"\xef\xbf\xbd" * 64)  # 192 bytes
    run_groups(torch, cases, "unquote utf-8", host_every=1)


def test_unquote_special_values_and_every_byte_value():
    torch = _torch()
    cases = sc.unquote_special_cases()
    assert len(cases) >= 3 * 256 + 6
    run_groups(torch, cases, "unquote special")


def test_value_lengths_0_to_65():
    torch = _torch()
    run_groups(torch, sc.length_cases(), "lengths", host_every=2)


def test_seeded_corpus():
    torch = _torch()
    run_groups(torch, sc.random_cases(5100, 150, longest=200), "corpus", host_every=4)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_short_last_wavefronts(n):
    torch = _torch()
    for config in (sc.const("ab", "<->"), sc.UNQUOTE):
        values = [v for c, _, v in sc.random_cases(900 + n, 260, longest=90) if c["Method"] == "unquote" or c["Match"] == "aba"][:n]
        assert len(values) == n
        if n:
            check(torch, config, values, pad_front=n % 16, what="n = %d" % n)
            check_host_entry(config, values, "n = %d, host entry" % n)
        else:  # n = 0 touches nothing: not even its pointers
            needed = ctypes.c_uint64(7)
            assert sr.load().lc_strrep_apply_device(proc(config).handle, None, None, 0, None, None, None, 0, ctypes.byref(needed), None) == LC_OK
            assert needed.value == 0


@pytest.mark.parametrize("where", ["lane0", "lane63", "wave3"])
def test_one_4096_byte_value(where):
    """one long value among short ones: in lane 0, in lane 63, and as the only value of wave 3 that has bytes"""
    torch = _torch()
    for config, big, short in ((sc.const("ab", "0123"), (b"ab" + b"." * 62) * 64, [b"x%dab" % i for i in range(256)]),
                               (sc.UNQUOTE, (b"\\x41" + "啊".encode() + b'"' + b"." * 56) * 64, [b"v%d\\t" % i for i in range(256)])):
        assert len(big) == 4096
        if where == "lane0":
            values = [big] + short[1:]
        elif where == "lane63":
            values = short[:63] + [big] + short[64:]
        else:
            values = short[:192] + [b""] * 20 + [big] + [b""] * 43
        check(torch, config, values, pad_front=5, what=where)


def test_nothing_changes_and_everything_changes():
    torch = _torch()
    for config, same, other in ((sc.const("needle", "N"), b"no such thing here, need le", b"a needle and a needle"),
                                (sc.UNQUOTE, b'plain "quoted" text', b"tab\\there")):
        values = [same + b"%d" % i for i in range(300)]
        data, off = pack(config, values, pad_front=3)
        rc, flags, out_off, out, needed = device_apply(torch, config, data, off, cap=512)
        assert rc == LC_OK and needed == 0 and not flags.any() and not out_off.any()
        assert (out == SENT).all()  # d_out is untouched
        values = [other + b"%d" % i for i in range(300)]
        assert (check(torch, config, values, pad_front=11, what="everything changes") == model.CHANGED).all()


def test_overflow_writes_nothing_and_the_call_may_be_repeated():
    torch = _torch()
    for config, values in ((sc.const("o", "0o0"), [b"foo boo %d" % i for i in range(200)]), (sc.UNQUOTE, [b"\\u554a %d \xff" % i for i in range(200)])):
        data, off = pack(config, values, pad_front=7)
        _, flags, out_off, out, needed = device_apply(torch, config, data, off)
        against_model(config, values, flags, out_off, out, "reference run")
        rc, flags1, off1, out1, needed1 = device_apply(torch, config, data, off, cap=needed - 1)
        assert rc == LC_ERR_OVERFLOW and needed1 == needed
        assert (out1 == SENT).all(), "something was written to d_out although it does not fit"
        assert np.array_equal(flags1, flags) and np.array_equal(off1, out_off)
        rc, flags2, off2, out2, _ = device_apply(torch, config, data, off, cap=needed)
        assert rc == LC_OK and np.array_equal(out2, out) and np.array_equal(flags2, flags) and np.array_equal(off2, out_off)


def test_argument_errors():
    torch = _torch()
    config = sc.const("a", "b")
    data, off = pack(config, [b"banana"])
    d_data, d_off = torch.from_numpy(data).to("cuda:0"), torch.from_numpy(off).to("cuda:0")
    flags, out_off, out = Guarded(torch, 1), Guarded(torch, 16), Guarded(torch, 16)
    L, h = sr.load(), proc(config).handle
    needed = ctypes.c_uint64(0)
    good = [h, d_data.data_ptr(), d_off.data_ptr(), 1, flags.ptr, out_off.ptr, out.ptr, 16, ctypes.byref(needed), None]
    for k in (0, 1, 2, 4, 5, 6):  # a NULL handle, a NULL array
        args = list(good)
        args[k] = None
        assert L.lc_strrep_apply_device(*args) == LC_ERR_ARG, k
    args = list(good)
    args[5] = out_off.ptr + 4  # the offsets are 8-byte words
    assert L.lc_strrep_apply_device(*args) == LC_ERR_ARG
    big = torch.from_numpy(np.array([0, 1 << 31], np.uint32).view(np.int32)).to("cuda:0")  # a batch of 2 GiB: refused before any byte is read
    args = list(good)
    args[2] = big.data_ptr()
    assert L.lc_strrep_apply_device(*args) == LC_ERR_ARG
    torch.cuda.synchronize()
    assert (flags.bytes("d_flags") == SENT).all() and (out_off.bytes("d_out_off") == SENT).all() and (out.bytes("d_out") == SENT).all()
    assert L.lc_strrep_apply_device(*good) == LC_OK and needed.value == 6
    assert out.bytes("d_out")[:6].tobytes() == b"bbnbnb" and flags.bytes("d_flags")[0] == 1


def test_a_tensor_on_another_device_is_refused():
    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    config = sc.const("a", "b")
    data, off = pack(config, [b"banana"])
    other = torch.device("cuda:1")
    d_data, d_off = torch.from_numpy(data).to(other), torch.from_numpy(off).to(other)
    scratch = torch.zeros(64, dtype=torch.uint8, device=other)
    needed = ctypes.c_uint64(0)
    torch.cuda.set_device(0)
    assert sr.load().lc_strrep_apply_device(proc(config).handle, d_data.data_ptr(), d_off.data_ptr(), 1, scratch.data_ptr(), scratch.data_ptr() + 8,
                                            scratch.data_ptr() + 32, 16, ctypes.byref(needed), None) == LC_ERR_ARG


def test_processor_on_a_1000_log_batch():
    """lc_strrep_process_logs_json on the device against the same processor code over the CPU double, and both against the model"""
    from helpers import strrep_product as sp
    _torch()
    symbols = ["\\x22", "\\t", "\\u554a", "\\", "\"", "啊", "plain ", "x", "\\q", "N/A "]
    rnd = random.Random(77)
    values = ["".join(rnd.choice(symbols) for _ in range(rnd.randrange(0, 30))) for _ in range(1000)]
    logs = [[("host", "h%d" % i), ("content", v), ("content", v[::-1])] if i % 7 else [("host", "only")] for i, v in enumerate(values)]
    for config in ({"SourceKey": "content", "Method": "unquote", "DestKey": "decoded"}, {"SourceKey": "content", "Method": "const", "Match": "N/A ", "ReplaceString": ""}):
        on_device, on_double = sr.Processor(**config), sp.processor(**config)
        sr.binding.launched_kernels()
        got, want = on_device.process_logs(logs), on_double.process_logs(logs)
        assert "strrep_size_kernel" in sr.binding.launched_kernels()
        expected, alarms, counters = model.process_logs(config, logs)
        assert got == want == expected
        assert on_device.counters() == on_double.counters() == counters and counters["changed"] > 100
        assert on_device.collect_alarms() == on_double.collect_alarms() == alarms
        if config["Method"] == "unquote":
            assert counters["unquote_errors"] > 100 and len(alarms) == counters["unquote_errors"]
