"""processor_split_key_value on the device: kv_split_kernel through lc_kvsplit_device and lc_kvsplit_host against
tests/helpers/kv_model.py (the Go restated line by line) -- every fixture case, every decision byte on chosen offsets for every residue of
the value's first byte, long needles across the quad / stage / tile borders, pair counts around W, short last wavefronts, sentinel-filled
and guarded outputs, argument errors -- and the processor on a 1000-log batch against the CPU double."""
import functools
import json

import numpy as np
import pytest

from helpers import kv_cases as kc
from helpers import kv_model
from loongcollector_amd import kvsplit

pytestmark = pytest.mark.gpu
SENT = 0xA5
GUARD = 4  # guard rows before and behind every output array
OFFSETS = (15, 16, 17, 63, 64, 65, 127, 128, 129)
LOGFMT = {"Delimiter": " ", "Separator": "=", "Quote": "\""}
EDGE = {"Delimiter": "#?#", "Separator": ": ", "Quote": "'"}
Q2 = {"Delimiter": " ", "Separator": "=", "Quote": "\"\""}
LONG = {"Delimiter": "#D中文分隔#", "Separator": "#S中文分隔#"}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@functools.lru_cache(maxsize=None)
def _proc(config_json):
    return kvsplit.Processor(**json.loads(config_json))


def proc(config):
    return _proc(json.dumps(config, sort_keys=True))


def junk(config, n, shift=0):
    """n bytes the routine would react to: delimiter, separator, quote and backslash bytes"""
    d, s, q = kc.needles(config)
    pattern = bytes([d[0], s[0], (q or b'"')[0], 0x5C])
    return bytes(pattern[(i + shift) & 3] for i in range(n))


def pack(config, values, pad_front=0):
    """values back to back behind pad_front bytes -> (data uint8, padded to whole 16-byte units with bytes the routine would react to, off)"""
    blob = junk(config, pad_front) + b"".join(values)
    size = max((len(blob) + 15) // 16 * 16 + 16, 16)
    data = np.frombuffer(blob + junk(config, size - len(blob), 1), np.uint8).copy()
    off = np.zeros(len(values) + 1, np.int32)
    off[1:] = np.cumsum([len(v) for v in values])
    return data, off + pad_front


def at_residues(config, wanted):
    """wanted: [(value, residue of its first byte)] -> values with junk values between them so that every wanted one begins at its
    residue (the fillers are split and compared like every other value)"""
    values, at = [], 0
    for value, residue in wanted:
        gap = (residue - at) % 16
        if gap:
            values.append(junk(config, gap, at))
            at += gap
        values.append(value)
        at += len(value)
    return values


def device_rows(torch, config, data, off, W, with_pairs=True):
    """lc_kvsplit_device over the packed bytes; every output array is pre-filled with the sentinel and guarded on both sides"""
    n = len(off) - 1
    dev = torch.device("cuda:0")
    full, d_out, rows = {}, {}, {}
    for k, (shape, dtype) in kvsplit.out_shapes(n, W).items():  # byte buffers: (GUARD rows, the n rows, GUARD rows), all sentinel
        rows[k] = int(np.prod(shape[1:])) * np.dtype(dtype).itemsize
        full[k] = torch.full(((n + 2 * GUARD) * rows[k] + 16,), SENT, dtype=torch.uint8, device=dev)
        d_out[k] = full[k][GUARD * rows[k]:(GUARD + n) * rows[k]] if rows[k] and n else None
    d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)
    if n:
        kvsplit.split_device(proc(config), d_data, d_off, n, W, d_out["status"], d_out["npairs"], d_out["pairs"] if with_pairs else None,
                             stream=torch.cuda.current_stream().cuda_stream)
    else:  # n = 0 touches nothing: not even its pointers
        kvsplit.load().lc_kvsplit_device(proc(config).handle, None, None, 0, W, None, None, None, None)
    torch.cuda.synchronize()
    res = {}
    for k, (shape, dtype) in kvsplit.out_shapes(n, W).items():
        raw = full[k].cpu().numpy()
        assert (raw[:GUARD * rows[k]] == SENT).all() and (raw[(GUARD + n) * rows[k]:] == SENT).all(), "%s: a guard row was written" % k
        res[k] = raw[GUARD * rows[k]:(GUARD + n) * rows[k]].view(dtype).reshape(shape)
    return res


def against_model(got, config, values, W, what):
    """status, the TRUE count, the first min(count, W) rows -- and nothing written behind them.  A value the reference panics on is
    compared on its status alone (its count and rows are unspecified), never skipped."""
    untouched = np.full(4, SENT, np.uint8).view(np.int32)[0]
    panics = 0
    for i, value in enumerate(values):
        want = kc.rows_of(kc.rows_text(config, value))
        if want is None:
            assert got["status"][i] == kvsplit.LC_KV_REF_PANIC, (what, i, value[:100], "the model panics, status %d" % got["status"][i])
            panics += 1
            continue
        assert got["status"][i] == kvsplit.LC_KV_OK, (what, i, value[:100], "status %d, the model does not panic" % got["status"][i])
        assert got["npairs"][i] == len(want), (what, i, value[:100], int(got["npairs"][i]), len(want))
        k = min(len(want), W)
        assert np.array_equal(got["pairs"][i][:k], want[:k]), (what, i, value[:100], got["pairs"][i][:k].tolist(), want[:k].tolist())
        assert (got["pairs"][i][k:] == untouched).all(), (what, i, value[:100], "a row behind min(npairs, W) was written")
    return panics


def check(torch, config, values, W=16, pad_front=0, what="device"):
    data, off = pack(config, values, pad_front)
    return against_model(device_rows(torch, config, data, off, W), config, values, W, what)


def test_fixture_cases_device_and_host_entry():
    """every fixture case, one launch per configuration, and the same values through the host entry"""
    torch = _torch()
    groups = kc.cases_by_config(kc.all_cases())
    assert len(groups) >= 12 and sum(len(c) for _, c in groups) > 10000
    panics = 0
    for config, cases in groups:
        values = [v for _, _, v, _ in cases]
        for (label, _, v, rows) in cases[:50]:
            assert kc.rows_text(config, v) == rows, label  # (the model still gives what the files record)
        panics += check(torch, config, values, W=24, pad_front=len(values) % 16, what="device %r" % (config,))
        got = kvsplit.split_host(proc(config), values, W=24, fill=SENT)
        against_model(got, config, values, 24, "host entry %r" % (config,))
    assert panics > 80
    assert "kv_split_kernel" in kvsplit.binding.launched_kernels()


# (what stands before the filler, what stands behind it, index of the decision byte in the latter)
EDGE_KINDS = {
    "delimiter_first_byte": ("k: v", "#?#z: 9", 0),
    "delimiter_last_byte": ("k: v", "#?#z: 9", 2),
    "delimiter_near_miss": ("k: v", "#?x#?#z: 9", 0),
    "separator_first_byte": ("k", ": v#?#z: 9", 0),
    "separator_second_byte": ("k", ": v#?#z: 9", 1),
    "separator_near_miss": ("k", ":x: v#?#z: 9", 0),
    "opening_quote": ("k", ": 'q#?#r'#?#z: 9", 2),
    "prefix_quote": ("a: 1", "#?#'q#?#r: s'#?#z: 9", 3),
    "escape_space": ("k: 'a#?#b", " \\' c'#?#z: 9", 0),
    "escape_backslash": ("k: 'a#?#b", " \\' c'#?#z: 9", 1),
    "escaped_quote": ("k: 'a#?#b", " \\' c'#?#z: 9", 2),
    "escaped_quote_twice": ("k: 'a#?#b", " \\' \\' c'#?#z: 9", 5),
    "closing_quote": ("k: 'a#?#b", "'#?#z: 9", 0),
    "closing_quote_no_delimiter_behind": ("k: 'a#?#b", "'zzzy: 2#?#z: 9", 0),
    "no_closing_quote": ("k: 'a#?#b", "#?#z: 9#?#w: 8", 0),
}


@functools.lru_cache(maxsize=None)
def edge_values():
    """-> [(value, residue)]: the decision byte of every kind at offset p of its value, the value whole and cut right behind that byte (a
    needle that straddles the value's END), for all 16 residues of the value's first byte"""
    out = []
    for kind, (before, after, idx) in sorted(EDGE_KINDS.items()):
        for p in OFFSETS:
            whole = (before + "x" * (p - len(before) - idx) + after).encode()
            assert len(before) + idx <= p
            for residue in range(16):
                out.append((whole, residue))
                out.append((whole[:p + 1], residue))
    return out


def test_decision_bytes_on_the_borders_for_every_residue():
    """the first and last byte of a 3-byte delimiter, both bytes of a 2-byte separator, the quote, each byte of ` \\Q`, the closing quote on
    offsets 15 .. 129, the value's first byte on every residue: the quad, stage and tile borders fall on every one of them"""
    torch = _torch()
    wanted = edge_values()
    assert len(wanted) == len(EDGE_KINDS) * len(OFFSETS) * 16 * 2
    values = at_residues(EDGE, wanted)
    assert check(torch, EDGE, values, W=8, what="edges") == 0
    got = kvsplit.split_host(proc(EDGE), values[:2000], W=8, fill=SENT)
    against_model(got, EDGE, values[:2000], 8, "edges, host entry")


def test_a_15_byte_delimiter_straddles_every_border():
    torch = _torch()
    d, s, _ = kc.needles(LONG)
    assert len(d) == len(s) == 15
    wanted = []
    for needle, tail in ((d, b"z" + s + b"9"), (s, b"v" + d + b"z" + s + b"9")):
        for border in (16, 64, 128):
            for inside in range(0, 16):  # bytes of the needle before the border
                for residue in range(16):
                    p = border - inside - residue  # the needle's first byte, counted from the value's first byte
                    if p < 2:
                        continue
                    head = b"k" + (s + b"v" if needle is d else b"")
                    if p < len(head):
                        continue
                    value = head + b"y" * (p - len(head)) + needle + tail
                    wanted.append((value, residue))
                    wanted.append((value[:p + max(inside, 1)], residue))  # the value ends inside the needle
    values = at_residues(LONG, wanted)
    assert len(values) > 2000
    assert check(torch, LONG, values, W=4, what="15-byte needles") == 0
    quoted = dict(LONG, Quote="\"\"\"")
    assert check(torch, quoted, values[:1500], W=4, what="15-byte needles, 3-byte quote") == 0


def test_pair_counts_around_w_and_w_zero():
    torch = _torch()
    W = 4
    values = [" ".join("k%d=%d" % (i, i) for i in range(n)).encode() for n in (W - 1, W, W + 1, 1, 3 * W, W)] + [b'a="x y" b=2 c=3 d="4 5" e=6']
    data, off = pack(LOGFMT, values, 3)
    got = device_rows(torch, LOGFMT, data, off, W)
    against_model(got, LOGFMT, values, W, "around W")
    assert got["npairs"].tolist() == [W - 1, W, W + 1, 1, 3 * W, W, 5]
    for with_pairs in (True, False):  # W = 0: the counts alone, pairs may be NULL
        got = device_rows(torch, LOGFMT, data, off, 0, with_pairs=with_pairs)
        against_model(got, LOGFMT, values, 0, "W = 0")
    got = kvsplit.split_host(proc(LOGFMT), values, W=0, fill=SENT)
    against_model(got, LOGFMT, values, 0, "W = 0, host entry")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_short_last_wavefronts(n):
    torch = _torch()
    values = kc.random_values(LOGFMT, 900 + n, n, longest=90)
    check(torch, LOGFMT, values, W=6, pad_front=n % 16, what="n = %d" % n)
    if n:
        check(torch, {}, kc.random_values({}, 901 + n, n, longest=90), W=6, what="n = %d, no quote" % n)


def test_an_empty_value_between_two_long_ones_and_a_70000_byte_value():
    torch = _torch()
    long_a = " ".join('key%d="v %d"' % (i, i) for i in range(400)).encode()
    long_b = b'open="never closed ' + b"x=1 " * 300
    big = (" ".join("k%d=%d" % (i, i) for i in range(40)) + ' q="' + "y " * 35000 + '" tail=1 last="a \\" b" end').encode()
    assert len(big) > 70000
    values = [long_a, b"", long_b, b"", b"", big, b"a=1"]
    check(torch, LOGFMT, values, W=48, pad_front=7, what="empty between long, 70 000 bytes")
    plain = [v.replace(b'"', b"'") for v in values]
    check(torch, {"Delimiter": " ", "Separator": "="}, plain, W=48, pad_front=9, what="the same without a quote")


def test_a_panic_value_beside_normal_ones_in_one_wavefront():
    torch = _torch()
    values = [b'a=1 b=""x y"" c=3', b'a=""x ', b'k=v', b'c=1 a=""x ', b"", b'a=""x yz c=1 d=2'] * 10
    assert [kv_model.split(Q2, v)[0] for v in values[:6]] == ["ok", "panic", "ok", "panic", "ok", "ok"]
    assert len(values) < 64 and check(torch, Q2, values, W=8, pad_front=2, what="panic beside normal") == 20


def test_argument_errors():
    torch = _torch()
    dev = torch.device("cuda:0")
    values = [b"a=1 b=2"]
    data, off = pack(LOGFMT, values)
    d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)
    status = torch.zeros(16, dtype=torch.uint8, device=dev)
    npairs = torch.zeros(4, dtype=torch.int32, device=dev)
    raw = torch.full((16 * 8 + 32,), SENT, dtype=torch.uint8, device=dev)
    L, h = kvsplit.load(), proc(LOGFMT).handle
    aligned = raw.data_ptr() + (-raw.data_ptr()) % 16
    args = (h, d_data.data_ptr(), d_off.data_ptr(), 1, 8, status.data_ptr(), npairs.data_ptr())
    for shift in (4, 8, 12):  # pairs is written as 16-byte vectors
        assert L.lc_kvsplit_device(*args, aligned + shift, None) == 5
    assert L.lc_kvsplit_device(*args, None, None) == 5  # NULL pairs with W > 0
    assert L.lc_kvsplit_device(None, *args[1:], aligned, None) == 5
    assert L.lc_kvsplit_device(h, d_data.data_ptr(), d_off.data_ptr(), 1, 8, status.data_ptr(), npairs.data_ptr() + 2, aligned, None) == 5
    torch.cuda.synchronize()
    assert (raw.cpu().numpy() == SENT).all() and int(npairs.sum()) == 0
    assert L.lc_kvsplit_device(*args, aligned, None) == 0
    torch.cuda.synchronize()
    assert npairs[0].item() == 2


def test_processor_on_a_1000_log_batch_with_the_mop_up():
    """lc_kvsplit_process_logs_json on the device against the same processor code over the CPU double, and both against the model"""
    from helpers import kv_product as kp
    _torch()
    config = dict(LOGFMT, SourceKey="content", KeepSource=False)
    values = [v.decode() for v in kc.random_values(LOGFMT, 31, 990, longest=120)]
    values += [" ".join("k%d=%d" % (i, i) for i in range(n)) for n in (3, 17, 33, 40, 5, 16, 18, 2, 1, 64)]
    logs = [[("host", "h%d" % i), ("content", v)] if i % 7 else [("host", "only")] for i, v in enumerate(values)]
    on_device, on_double = kvsplit.Processor(**config), kp.processor(**config)
    for p in (on_device, on_double):
        p.set_first_trip_pairs(8)
    got, want = on_device.process_logs(logs), on_double.process_logs(logs)
    assert got == want == kp.model_logs(config, logs)[0]
    assert on_device.counters() == on_double.counters() and on_device.counters()["mop_up"] > 20
    assert on_device.collect_alarms() == on_double.collect_alarms()
