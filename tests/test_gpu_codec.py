"""The field codecs on the device: codec_len_kernel, b64_encode_kernel, b64_decode_size_kernel, b64_decode_write_kernel, md5_field_kernel
and the scan through lc_codec_apply_device and lc_codec_apply_host against tests/helpers/codec_model.py, bit for bit -- the whole
deterministic corpus of tests/helpers/codec_cases.py for every residue of the value's first byte, short last wavefronts, one long value in
a wavefront, a wavefront of empty values, the overflow contract, four sentinel rows around every output array and the sentinel in the
padding between two values' outputs, argument errors -- and the processors on the reference's unit-test vectors.

Every batch goes through the device entry TWICE: with no room at all (LC_ERR_OVERFLOW unless there is no output; flags, offsets, lengths
and `needed` must be right already) and again with exactly `needed` bytes between the sentinel rows."""
import ctypes
import functools

import numpy as np
import pytest

from helpers import codec_cases as cc
from helpers import codec_model as model
from loongcollector_amd import codec

pytestmark = pytest.mark.gpu
SENT = 0xA5
GUARD = 64  # four 16-byte rows of sentinel bytes before and behind d_flags, d_err_off, d_out_off, d_out_len and d_out
LC_OK, LC_ERR_ARG, LC_ERR_OVERFLOW = 0, 5, 6
KERNELS = {"base64_encode": ("codec_len_kernel", "scan64_kernel", "b64_encode_kernel"),
           "base64_decode": ("b64_decode_size_kernel", "scan64_kernel", "b64_decode_write_kernel"),
           "md5": ("codec_len_kernel", "md5_field_kernel")}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@functools.lru_cache(maxsize=None)
def proc(op):
    return codec.Processor(Op=op)


def pack(values, pad_front=0):
    """values back to back behind pad_front bytes -> (data uint8, padded to whole 16-byte units with bytes the kernels would react to, off)"""
    junk = b"=Q\r\n"
    blob = (junk * 4)[:pad_front] + b"".join(values)
    size = max((len(blob) + 15) // 16 * 16 + 16, 16)
    data = np.frombuffer(blob + (junk * (size // 4 + 1))[:size - len(blob)], np.uint8).copy()
    off = np.zeros(len(values) + 1, np.uint32)
    off[1:] = np.cumsum([len(v) for v in values])
    return data, (off + pad_front).astype(np.int32)


def at_residues(wanted):
    """wanted: [(residue of its first byte, value)] -> values with filler values between them so that every wanted one begins at its
    residue (the fillers are coded and compared like every other value)"""
    values, at = [], 0
    for residue, value in wanted:
        gap = (residue - at) % 16
        if gap:
            values.append(b"QUJD"[:1] * gap)
            at += gap
        values.append(value)
        at += len(value)
    return values


class Guarded:
    """an array between two times four rows of sentinel bytes, itself pre-filled with the sentinel"""

    def __init__(self, torch, nbytes):
        self.n = nbytes
        self.full = torch.full((2 * GUARD + nbytes + 16,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.full.data_ptr() % 16 == 0
        self.ptr = self.full.data_ptr() + GUARD

    def bytes(self, what):
        raw = self.full.cpu().numpy()
        assert (raw[:GUARD] == SENT).all() and (raw[GUARD + self.n:] == SENT).all(), "a sentinel byte around %s was written" % what
        return raw[GUARD:GUARD + self.n]


def device_apply(torch, op, data, off, cap="needed", with_err_off=True):
    """-> (rc of the last call, flags, err_off, out_off, out_len, out bytes, needed).  cap: "needed", or the out_cap of the one call to make"""
    n = len(off) - 1
    L = codec.load()
    d_data, d_off = torch.from_numpy(data).to("cuda:0"), torch.from_numpy(off).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    needed = ctypes.c_uint64(0)

    def call(out_cap, out_ptr):
        flags, err_off, out_off, out_len = Guarded(torch, n), Guarded(torch, 4 * n), Guarded(torch, 8 * (n + 1)), Guarded(torch, 4 * n)
        rc = L.lc_codec_apply_device(proc(op).handle, d_data.data_ptr(), d_off.data_ptr(), n, flags.ptr, err_off.ptr if with_err_off else None, out_off.ptr,
                                     out_len.ptr, out_ptr, out_cap, ctypes.byref(needed), stream)
        torch.cuda.synchronize()
        return (rc, flags.bytes("d_flags").copy(), err_off.bytes("d_err_off").view(np.uint32).copy(), out_off.bytes("d_out_off").view(np.uint64).copy(),
                out_len.bytes("d_out_len").view(np.uint32).copy())

    if cap != "needed":
        out = Guarded(torch, cap)
        rc, flags, err_off, out_off, out_len = call(cap, out.ptr)
        return rc, flags, err_off, out_off, out_len, out.bytes("d_out").copy(), int(needed.value)
    rc0, flags0, err0, off0, len0 = call(0, None)
    want = int(needed.value)
    assert rc0 == (LC_ERR_OVERFLOW if want else LC_OK) and int(off0[n]) == want
    out = Guarded(torch, want)
    rc, flags, err_off, out_off, out_len = call(want, out.ptr)
    assert rc == LC_OK and int(needed.value) == want
    assert np.array_equal(flags, flags0) and np.array_equal(out_off, off0) and np.array_equal(out_len, len0) and np.array_equal(err_off, err0), \
        "the repeated call disagrees with the one that overflowed"
    return rc, flags, err_off, out_off, out_len, out.bytes("d_out").copy(), want


def against_model(op, values, flags, err_off, out_off, out_len, out, what, with_err_off=True):
    n = len(values)
    assert int(out_off[0]) == 0 and len(out) == int(out_off[n])
    assert not (out_off % 16).any(), "out_off: multiples of 16"
    untouched = np.ones(len(out), bool)
    for i, value in enumerate(values):
        want_flags, want, want_err = model.apply(op, value)
        at, size = int(out_off[i]), int(out_len[i])
        assert int(flags[i]) == want_flags, (what, i, value[:120], int(flags[i]), want_flags)
        assert size == (len(want) if want is not None else 0), (what, i, value[:120], size)
        assert int(out_off[i + 1]) - at == (size + 15) // 16 * 16, (what, i, "out_off ascends in whole 16-byte units")
        assert out[at:at + size].tobytes() == (want or b""), (what, i, value[:120], out[at:at + size].tobytes()[:160], want)
        untouched[at:at + size] = False
        if want_err is not None and with_err_off:
            assert int(err_off[i]) == want_err, (what, i, value[:120], int(err_off[i]), want_err)
        else:
            assert int(err_off[i]) == 0xA5A5A5A5, (what, i, "d_err_off is written for errors only")
    assert (out[untouched] == SENT).all(), (what, "the padding between two values' outputs was written")


def check(torch, op, values, pad_front=0, what="device", with_err_off=True):
    data, off = pack(values, pad_front)
    _, flags, err_off, out_off, out_len, out, _ = device_apply(torch, op, data, off, with_err_off=with_err_off)
    against_model(op, values, flags, err_off, out_off, out_len, out, "%s %s" % (op, what), with_err_off)
    return flags


def check_host_entry(op, values, what):
    assert codec.apply_host(proc(op), values) == [model.apply(op, v) for v in values], (op, what)


@pytest.mark.parametrize("op", model.OPS)
def test_the_whole_corpus_for_every_residue(op):
    torch = _torch()
    wanted = cc.cases(op)
    assert {r for r, _ in wanted} == set(range(16))
    values = at_residues(wanted)
    codec.binding.launched_kernels()
    flags = check(torch, op, values, what="corpus")
    names = codec.binding.launched_kernels()
    for name in KERNELS[op]:
        assert name in names, name
    if op == "base64_decode":
        assert (flags == model.ERROR).sum() > 3000 and (flags == model.OUT).sum() > 3000
        check_host_entry(op, values[::5], "corpus, host entry")
    else:
        assert (flags == model.OUT).all()
        check_host_entry(op, values[::3], "corpus, host entry")


def test_reference_unit_test_vectors_on_the_device():
    _torch()
    for e in cc.load_vectors()["cases"]:
        p = codec.Processor(**e["config"])
        assert [list(kv) for kv in p.process_logs([[tuple(kv) for kv in e["log"]]])[0]] == e["contents"], e["case"]
        assert p.collect_alarms() == [(a["kind"], a["text"].encode()) for a in e["alarms"]], e["case"]


def _mixed(op, n):
    pool = [v for _, v in cc.cases(op)]
    step = max(1, len(pool) // 300)
    return (pool[::step] * 2)[:n]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_short_last_wavefronts(n):
    torch = _torch()
    for op in model.OPS:
        values = _mixed(op, n)
        assert len(values) == n
        if n:
            check(torch, op, values, pad_front=n % 16, what="n = %d" % n)
            check_host_entry(op, values, "n = %d, host entry" % n)
        else:  # n = 0 touches nothing: not even its pointers
            needed = ctypes.c_uint64(7)
            assert codec.load().lc_codec_apply_device(proc(op).handle, None, None, 0, None, None, None, None, None, 0, ctypes.byref(needed), None) == LC_OK
            assert needed.value == 0
            assert codec.apply_host(proc(op), []) == []


BIG = cc.payload(4096, 9)
BIG_SHAPES = [("base64_encode", BIG), ("md5", BIG), ("base64_decode", model.encode(BIG)[:4096]), ("base64_decode", cc.mime(BIG[:2994])[:-2])]


@pytest.mark.parametrize("where", ["lane0", "lane63", "alone"])
def test_one_4096_byte_value(where):
    """one long value among short ones: in lane 0, in lane 63, and as the only value of a wavefront that has bytes; for the decode both
    clean and with a CRLF every 76 characters"""
    torch = _torch()
    assert [len(b) for _, b in BIG_SHAPES] == [4096] * 4 and BIG_SHAPES[3][1].count(b"\r\n") == 52
    for op, big in BIG_SHAPES:
        short = [b"QUJD" * (i % 5) for i in range(256)]
        if where == "lane0":
            values = [big] + short[1:]
        elif where == "lane63":
            values = short[:63] + [big] + short[64:]
        else:
            values = short[:192] + [b""] * 20 + [big] + [b""] * 43
        flags = check(torch, op, values, pad_front=5, what=where)
        assert (flags == model.OUT).all()


def test_a_wavefront_of_empty_values_in_front_of_a_normal_one():
    torch = _torch()
    for op in model.OPS:
        normal = model.encode(cc.payload(100, 1))
        check(torch, op, [b""] * 64 + [normal], pad_front=3, what="64 empty values")
        check(torch, op, [b""] * 64, what="nothing but empty values")


def test_overflow_writes_nothing_and_the_call_may_be_repeated():
    torch = _torch()
    for op in model.OPS:
        values = _mixed(op, 200)
        data, off = pack(values, pad_front=7)
        _, flags, err_off, out_off, out_len, out, needed = device_apply(torch, op, data, off)
        against_model(op, values, flags, err_off, out_off, out_len, out, "reference run")
        rc, flags1, err1, off1, len1, out1, needed1 = device_apply(torch, op, data, off, cap=needed - 1)
        assert rc == LC_ERR_OVERFLOW and needed1 == needed
        assert (out1 == SENT).all(), "something was written to d_out although it does not fit"
        assert np.array_equal(flags1, flags) and np.array_equal(off1, out_off) and np.array_equal(len1, out_len) and np.array_equal(err1, err_off)
        rc, flags2, _, off2, len2, out2, _ = device_apply(torch, op, data, off, cap=needed)
        assert rc == LC_OK and np.array_equal(out2, out) and np.array_equal(flags2, flags) and np.array_equal(off2, out_off) and np.array_equal(len2, out_len)


def test_a_null_err_off():
    torch = _torch()
    values = [v for _, v in cc.decode_error_cases()[::40]] + [b"QUJD"]
    flags = check(torch, "base64_decode", values, what="no d_err_off", with_err_off=False)
    assert (flags == model.ERROR).sum() > 30
    entries = codec.apply_host(proc("base64_decode"), values)
    assert entries == [model.apply("base64_decode", v) for v in values]


def test_the_host_entry_in_two_trips():
    _torch()
    L = codec.load()
    for op in model.OPS:
        values = _mixed(op, 120)
        total = sum(len(v) for v in values)
        L.lc_codec_set_trip_bytes(total // 2 + max(len(v) for v in values))
        try:
            check_host_entry(op, values, "two trips")
        finally:
            assert L.lc_codec_set_trip_bytes(0) == 2, "the batch took two trips"
        check_host_entry(op, values[:50], "one trip")
        assert L.lc_codec_set_trip_bytes(0) == 1


def test_argument_errors():
    torch = _torch()
    data, off = pack([b"QUJD"])
    d_data, d_off = torch.from_numpy(data).to("cuda:0"), torch.from_numpy(off).to("cuda:0")
    flags, err_off, out_off, out_len, out = Guarded(torch, 1), Guarded(torch, 4), Guarded(torch, 16), Guarded(torch, 4), Guarded(torch, 16)
    L, h = codec.load(), proc("base64_decode").handle
    needed = ctypes.c_uint64(0)
    good = [h, d_data.data_ptr(), d_off.data_ptr(), 1, flags.ptr, err_off.ptr, out_off.ptr, out_len.ptr, out.ptr, 16, ctypes.byref(needed), None]
    for k in (0, 1, 2, 4, 6, 7, 8):  # a NULL handle, a NULL array (d_err_off may be NULL)
        args = list(good)
        args[k] = None
        assert L.lc_codec_apply_device(*args) == LC_ERR_ARG, k
    for k, by in ((6, 4), (8, 8), (8, 4)):  # the offsets are 8-byte words, d_out is 16-byte aligned
        args = list(good)
        args[k] = good[k] + by
        assert L.lc_codec_apply_device(*args) == LC_ERR_ARG, (k, by)
    big = torch.from_numpy(np.array([0, 1 << 31], np.uint32).view(np.int32)).to("cuda:0")  # a batch of 2 GiB: refused before any byte is read
    args = list(good)
    args[2] = big.data_ptr()
    assert L.lc_codec_apply_device(*args) == LC_ERR_ARG
    torch.cuda.synchronize()
    for g, what in ((flags, "d_flags"), (err_off, "d_err_off"), (out_off, "d_out_off"), (out_len, "d_out_len"), (out, "d_out")):
        assert (g.bytes(what) == SENT).all(), what
    assert L.lc_codec_apply_device(*good) == LC_OK and needed.value == 16
    assert out.bytes("d_out")[:3].tobytes() == b"ABC" and (out.bytes("d_out")[3:] == SENT).all() and flags.bytes("d_flags")[0] == 1
    assert out_len.bytes("d_out_len").view(np.uint32)[0] == 3


def test_a_tensor_on_another_device_is_refused():
    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    data, off = pack([b"QUJD"])
    other = torch.device("cuda:1")
    d_data, d_off = torch.from_numpy(data).to(other), torch.from_numpy(off).to(other)
    scratch = torch.zeros(128, dtype=torch.uint8, device=other)
    needed = ctypes.c_uint64(0)
    torch.cuda.set_device(0)
    base = scratch.data_ptr()
    assert codec.load().lc_codec_apply_device(proc("md5").handle, d_data.data_ptr(), d_off.data_ptr(), 1, base, base + 8, base + 16, base + 32, base + 64, 32,
                                              ctypes.byref(needed), None) == LC_ERR_ARG


def test_processors_on_a_600_log_batch():
    """lc_codec_process_logs_json on the device against the same processor code over the CPU double, and both against the model"""
    from helpers import codec_product as cp
    _torch()
    texts = ["", "123", "a NUL \x00 inside", "啊" * 40, "🙂 and text " * 9, "line\r\nbreaks\n", "x" * 300]
    encoded = [model.encode(t.encode("utf-8")).decode() for t in texts]
    broken = ["QUJDRE=x", "test_value", "QUJD=", "Q", "QUJDRE=", encoded[4][:-1] + "-"]
    mimes = [cc.mime(t.encode("utf-8")).decode() for t in texts]
    pool = {"base64_encode": texts, "md5": texts, "base64_decode": encoded + broken + mimes}
    for config in ({"Op": "base64_encode", "SourceKey": "src", "NewKey": ""}, {"Op": "base64_encode", "SourceKey": "src", "NewKey": "b64", "NoKeyError": True},
                   {"Op": "base64_decode", "SourceKey": "src", "NewKey": "plain", "DecodeError": True, "NoKeyError": True},
                   {"Op": "md5", "SourceKey": "src", "MD5Key": "digest"}):
        source = pool[config["Op"]]
        logs = [[("host", "h%d" % i), ("src", source[i % len(source)]), ("src", "never visited")] if i % 7 else [("host", "only")] for i in range(600)]
        on_device, on_double = codec.Processor(**config), cp.processor(**config)
        codec.binding.launched_kernels()
        got, want = on_device.process_logs(logs), on_double.process_logs(logs)
        assert KERNELS[config["Op"]][0] in codec.binding.launched_kernels()
        expected, alarms, counters = model.process_logs(config, logs)
        assert got == want == expected
        assert on_device.counters() == on_double.counters() == counters and counters["out"] > 300 and counters["no_key"] == 86
        assert on_device.collect_alarms() == on_double.collect_alarms() == alarms
        if config["Op"] == "base64_decode":
            assert counters["decode_errors"] > 100 and len(alarms) == counters["decode_errors"] + 86
