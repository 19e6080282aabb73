"""processor_anchor on the device: anchor_locate_kernel through lc_anchor_locate_device and lc_anchor_locate_host against
tests/helpers/anchor_model.py (anchor.go restated on bytes) -- every fixture case, the first and last byte of Start and of Stop on
chosen tile offsets for every residue of the value's first byte, needles across the quad / stage / tile borders, near misses and
needles cut by the value's end there, value lengths 0-65, short last wavefronts, one long value in a wavefront, the early exit,
sentinel rows around the output, argument errors -- and the processor on a 1000-log batch against the CPU double."""
import functools
import json

import numpy as np
import pytest

from helpers import anchor_cases as ac
from loongcollector_amd import anchor

pytestmark = pytest.mark.gpu
SENT = 0xA5
GUARD = 4  # sentinel rows before and behind the span rows
OFFSETS = (15, 16, 17, 63, 64, 65, 127, 128, 129)
EDGE = ac.config_of([("abc:", "#?#"), ("#?#", "abc:"), ("c", "#"), ("", "?#a"), ("zz", "")])
LOGLINE = ac.config_of([("time:", "\t"), ("level:", "\t")])
FILL = b"."  # no needle holds it


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@functools.lru_cache(maxsize=None)
def _proc(config_json):
    return anchor.Processor(**json.loads(config_json))


def proc(config):
    return _proc(json.dumps(config, sort_keys=True))


def junk(config, n, shift=0):
    """n bytes the routine would react to: the needles' first bytes"""
    firsts = b"".join((a["Start"] or ":")[:1].encode() + (a["Stop"] or "\t")[:1].encode() for a in config["Anchors"])
    return bytes(firsts[(i + shift) % len(firsts)] for i in range(n))


def pack(config, values, pad_front=0):
    """values back to back behind pad_front bytes -> (data uint8, padded to whole 16-byte units with bytes the routine would react to, off)"""
    blob = junk(config, pad_front) + b"".join(values)
    size = max((len(blob) + 15) // 16 * 16 + 16, 16)
    data = np.frombuffer(blob + junk(config, size - len(blob), 1), np.uint8).copy()
    off = np.zeros(len(values) + 1, np.int32)
    off[1:] = np.cumsum([len(v) for v in values])
    return data, off + pad_front


def at_residues(wanted):
    """wanted: [(value, residue of its first byte)] -> values with filler values between them so that every wanted one begins at its
    residue (the fillers are located and compared like every other value)"""
    values, at = [], 0
    for value, residue in wanted:
        gap = (residue - at) % 16
        if gap:
            values.append(FILL * gap)
            at += gap
        values.append(value)
        at += len(value)
    return values


def device_spans(torch, config, data, off):
    """lc_anchor_locate_device over the packed bytes; the span array is pre-filled with the sentinel and has sentinel rows on both sides"""
    n = len(off) - 1
    dev = torch.device("cuda:0")
    p = proc(config)
    row = p.stride * 8
    full = torch.full(((n + 2 * GUARD) * row + 16,), SENT, dtype=torch.uint8, device=dev)
    assert full.data_ptr() % 16 == 0 and (GUARD * row) % 16 == 0
    d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)
    if n:
        anchor.locate_device(p, d_data, d_off, n, full[GUARD * row:], stream=torch.cuda.current_stream().cuda_stream)
    else:  # n = 0 touches nothing: not even its pointers
        assert anchor.load().lc_anchor_locate_device(p.handle, None, None, 0, None, None) == 0
    torch.cuda.synchronize()
    raw = full.cpu().numpy()
    assert (raw[:GUARD * row] == SENT).all() and (raw[(GUARD + n) * row:] == SENT).all(), "a sentinel row was written"
    return raw[GUARD * row:(GUARD + n) * row].view(np.int32).reshape(n, p.stride, 2)


def against_model(got, config, values, what):
    """every entry of every value, the pad entry of an odd count included"""
    stride = got.shape[1]
    assert stride == (len(config["Anchors"]) + 1) // 2 * 2
    for i, value in enumerate(values):
        want = ac.rows_of(ac.rows_text(config, value), stride)
        assert np.array_equal(got[i], want), (what, i, value[:120], got[i].tolist(), want.tolist())


def check(torch, config, values, pad_front=0, what="device"):
    data, off = pack(config, values, pad_front)
    against_model(device_spans(torch, config, data, off), config, values, what)


def test_fixture_cases_device_and_host_entry():
    """every fixture case, one launch per configuration, and the same values through the host entry"""
    torch = _torch()
    groups = ac.cases_by_config(ac.all_cases())
    assert len(groups) >= 30 and sum(len(c) for _, c in groups) > 6000
    anchor.binding.launched_kernels()
    for config, cases in groups:
        values = []
        for (label, _, v, tail, rows) in cases:  # (a named case's tail follows it as a value of its own, as in the packed buffer it means)
            values.append(v)
            if label.startswith("named:"):
                assert ac.rows_text(config, v) == rows, label  # (the model still gives what the files record)
                values.append(tail)
        check(torch, config, values, pad_front=len(values) % 16, what="device %r" % (config,))
        against_model(anchor.locate_host(proc(config), values, fill=SENT), config, values, "host entry %r" % (config,))
    assert "anchor_locate_kernel" in anchor.binding.launched_kernels()


@functools.lru_cache(maxsize=None)
def edge_values():
    """-> [(value, residue)]: for the needles abc: (Start of anchor 0, Stop of anchor 1) and #?# (the other way round), the first and the
    last byte on tile offset p -- so the needle straddles every border from both sides --, the needle's near miss (less its last byte) in
    front of it, the value cut behind the needle's last byte but one (its tail is then the NEXT value's head: the cut-off byte), for all
    16 residues of the value's first byte"""
    out = []
    for first, second in (("abc:", "#?#"), ("#?#", "abc:")):
        for p in OFFSETS:
            for residue in range(16):
                for on_last in (False, True):
                    at = p - residue - (len(first) - 1 if on_last else 0)  # first's first byte, counted from the value's first byte
                    if at >= 0:
                        whole = "." * at + first + "field" + second + "tail"
                        out.append((whole.encode(), residue))
                        out.append((whole[:at + len(first) - 1].encode(), residue))   # cut inside Start ...
                        out.append((whole[at + len(first) - 1:].encode(), (residue + at + len(first) - 1) % 16))  # ... the rest: the next value
                    if at >= len(first):
                        near = "." * (at - len(first)) + first[:-1] + "." + first + "field" + second
                        out.append((near.encode(), residue))
                    at2 = p - residue - (len(second) - 1 if on_last else 0) - len(first) - 2  # the same for second, behind first
                    if at2 >= 0:
                        whole = "." * at2 + first + "fd" + second + "tail"
                        out.append((whole.encode(), residue))
                        out.append((whole[:-5].encode(), residue))                          # cut inside Stop ...
                        out.append((whole[-5:].encode(), (residue + len(whole) - 5) % 16))  # ... the rest: the next value
                        near = "." * at2 + first + second[:-1] + second + "x"
                        out.append((near.encode(), residue))
    return out


def test_needle_bytes_on_the_borders_for_every_residue():
    """offsets 15 .. 129 x 16 residues: the quad, stage and tile borders fall on the first and on the last byte of Start and of Stop"""
    torch = _torch()
    wanted = edge_values()
    assert len(wanted) > 4000
    values = at_residues(wanted)
    check(torch, EDGE, values, what="edges")
    against_model(anchor.locate_host(proc(EDGE), values[:1500], fill=SENT), EDGE, values[:1500], "edges, host entry")


def test_a_32_byte_needle_straddles_every_border():
    torch = _torch()
    s32, p31 = "0123456789abcdefghijklmnopqrstuv", "VUTSRQPONMLKJIHGFEDCBA987654321"
    config = ac.config_of([(s32, p31), (p31, s32), (s32[:5], p31[:4])])
    wanted = []
    for border in (16, 64, 128):
        for inside in range(0, 32, 3):  # bytes of the needle before the border
            for residue in range(16):
                at = border - inside - residue
                if at < 0:
                    continue
                value = "." * at + s32 + "mid" + p31 + "x"
                wanted.append((value.encode(), residue))
                wanted.append((value[:at + 31].encode(), residue))  # the value ends inside the needle; the next value begins with its last byte
                wanted.append((value[at + 31:].encode(), (residue + at + 31) % 16))
                wanted.append((("." * at + p31 + s32[:31] + s32 + "end").encode(), residue))
    values = at_residues(wanted)
    assert len(values) > 1500
    check(torch, config, values, what="32-byte needles")


def test_value_lengths_0_to_65_and_odd_anchor_counts():
    torch = _torch()
    for count in (1, 3, 15):
        config = ac.config_of([("k%d=" % (i % 4), ";" if i % 2 else "") for i in range(count)])
        values = []
        for n in range(66):
            body = ("k1=a;k2=bc;k3=;k0=" + "v" * 70)[:n]
            values += [body.encode(), (("." * 70)[:max(n - 5, 0)] + "k0=1;")[:n].encode()]
        check(torch, config, values, pad_front=count, what="lengths 0-65, %d anchors" % count)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_short_last_wavefronts(n):
    torch = _torch()
    symbols = [b"time:", b"level:", b"\t", b"x", b"tim", b"leve", b":"]
    values = ac.random_values(symbols, 900 + n, n, longest=90)
    check(torch, LOGLINE, values, pad_front=n % 16, what="n = %d" % n)
    if n:
        against_model(anchor.locate_host(proc(LOGLINE), values, fill=SENT), LOGLINE, values, "n = %d, host entry" % n)


@pytest.mark.parametrize("where", ["lane0", "lane63", "wave3"])
def test_one_4096_byte_value(where):
    """one long value among short ones: in lane 0, in lane 63, and as the only value of wave 3 that has bytes"""
    torch = _torch()
    big = (b"." * 1000 + b"level:late\t" + b"." * 2000 + b"time:later\t").ljust(4095, b".") + b"\t"
    assert len(big) == 4096
    short = [b"time:%d\tlevel:l%d\t" % (i, i) for i in range(256)]
    if where == "lane0":
        values = [big] + short[1:]
    elif where == "lane63":
        values = short[:63] + [big] + short[64:]
    else:
        values = short[:192] + [b""] * 20 + [big] + [b""] * 43
    check(torch, LOGLINE, values, pad_front=5, what=where)


def test_the_early_exit():
    """a wavefront of 4096-byte values whose anchors all resolve in stage 0; the same with ONE lane whose Stop is the value's last byte; a
    wavefront in which every lane is "no start" and so walks to the end.  (What the exit saves is measured by tools/anchor_bench.py; here
    the results must not depend on it.)"""
    torch = _torch()
    front = [(b"time:%d\tlevel:l%d\t" % (i, i)).ljust(4096, b"x") for i in range(64)]
    check(torch, LOGLINE, front, what="all resolved in stage 0")
    one = list(front)
    one[37] = (b"time:37\tlevel:open").ljust(4095, b"x") + b"\t"
    assert ac.rows_text(LOGLINE, one[37]) == "5 7 14 4095"
    check(torch, LOGLINE, one, pad_front=9, what="one lane's Stop is the last byte")
    none = [(b"tim:%d level %d " % (i, i)).ljust(4096, b"x") for i in range(64)]
    none[5] = none[5][:-6] + b"time:\t"
    check(torch, LOGLINE, none, pad_front=3, what="no start anywhere")
    # a resolved wavefront beside one that has to walk, in one workgroup
    check(torch, LOGLINE, front + none + one + front, pad_front=1, what="four wavefronts")


def test_argument_errors():
    torch = _torch()
    dev = torch.device("cuda:0")
    values = [b"time:1\tlevel:2\t"]
    data, off = pack(LOGLINE, values)
    d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)
    raw = torch.full((16 * 4 + 32,), SENT, dtype=torch.uint8, device=dev)
    L, h = anchor.load(), proc(LOGLINE).handle
    aligned = raw.data_ptr() + (-raw.data_ptr()) % 16
    args = (h, d_data.data_ptr(), d_off.data_ptr(), 1)
    for shift in (4, 8, 12):  # a row is whole 16-byte units
        assert L.lc_anchor_locate_device(*args, aligned + shift, None) == 5
    assert L.lc_anchor_locate_device(*args, None, None) == 5
    assert L.lc_anchor_locate_device(None, *args[1:], aligned, None) == 5
    assert L.lc_anchor_locate_device(h, None, d_off.data_ptr(), 1, aligned, None) == 5
    torch.cuda.synchronize()
    assert (raw.cpu().numpy() == SENT).all()
    assert L.lc_anchor_locate_device(*args, aligned, None) == 0
    torch.cuda.synchronize()
    got = raw.cpu().numpy()[aligned - raw.data_ptr():][:16].view(np.int32)
    assert got.tolist() == [5, 6, 13, 14]


def test_a_tensor_on_another_device_is_refused():
    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    data, off = pack(LOGLINE, [b"time:1\tlevel:2\t"])
    other = torch.device("cuda:1")
    d_data, d_off = torch.from_numpy(data).to(other), torch.from_numpy(off).to(other)
    spans = torch.zeros(4, dtype=torch.int32, device=other)
    torch.cuda.set_device(0)
    assert anchor.load().lc_anchor_locate_device(proc(LOGLINE).handle, d_data.data_ptr(), d_off.data_ptr(), 1, spans.data_ptr(), None) != 0


def test_processor_on_a_1000_log_batch():
    """lc_anchor_process_logs_json on the device against the same processor code over the CPU double, and both against the model"""
    from helpers import anchor_product as ap
    _torch()
    config = {"Anchors": [{"Start": "time:", "Stop": "\t", "FieldName": "time"}, {"Start": "level:", "Stop": "\t", "FieldName": "level"},
                          {"Start": "msg:", "Stop": "", "FieldName": "msg"}], "SourceKey": "content", "NoKeyError": True, "NoAnchorError": True}
    symbols = [b"time:", b"level:", b"msg:", b"\t", b"x", b"tim", b"leve", b":", b"y z"]
    values = [v.decode() for v in ac.random_values(symbols, 31, 1000, longest=120)]
    logs = [[("host", "h%d" % i), ("content", v)] if i % 7 else [("host", "only")] for i, v in enumerate(values)]
    on_device, on_double = anchor.Processor(**config), ap.processor(**config)
    anchor.binding.launched_kernels()
    got, want = on_device.process_logs(logs), on_double.process_logs(logs)
    assert "anchor_locate_kernel" in anchor.binding.launched_kernels()
    model, alarms, metric = ap.model_logs(config, logs)
    assert got == want == model
    assert on_device.counters() == on_double.counters() and on_device.counters()["pairs_per_log"] == metric
    assert on_device.counters()["fields"] > 300 and on_device.counters()["no_start"] > 300 and on_device.counters()["no_stop"] > 50
    assert on_device.collect_alarms() == on_double.collect_alarms() == alarms
