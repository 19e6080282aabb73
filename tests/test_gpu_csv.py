"""processor_csv on the device: csv_split_kernel through lc_csv_device and lc_csv_host against tests/helpers/csv_model.py (the reader
rules restated line by line) -- every fixture case in batches of 1, 63, 64, 65 and 257 values, every decision byte on chosen offsets for
every alignment of the value's first byte, field counts around W, sentinel-filled and guarded outputs, argument errors -- and the
processor against the CPU double and the model."""
import functools
import json

import numpy as np
import pytest

from helpers import csv_cases as cc
from loongcollector_amd import csv_decode

pytestmark = pytest.mark.gpu
SENT = 0xA5
GUARD = 4  # guard rows before and behind every output array
OFFSETS = (15, 16, 17, 63, 64, 65, 127, 128)
BATCHES = (1, 63, 64, 65, 257)
WIDE = cc.WIDE.encode("utf-8")


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@functools.lru_cache(maxsize=None)
def _proc(config_json):
    return csv_decode.Processor(**json.loads(config_json))


def proc(config):
    sep, trim = cc.reader_config(config)
    return _proc(json.dumps({"SplitSep": sep.decode("utf-8"), "TrimLeadingSpace": trim}, sort_keys=True))


def junk(config, n, shift=0):
    """n bytes the routine would react to: separator, quote and line-end bytes"""
    sep, _ = cc.reader_config(config)
    pattern = bytes([sep[0], 0x22, 0x0A, 0x0D])
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
    residue (the fillers are read and compared like every other value)"""
    values, at = [], 0
    for value, residue in wanted:
        gap = (residue - at) % 16
        if gap:
            values.append(junk(config, gap, at))
            at += gap
        values.append(value)
        at += len(value)
    return values


def device_rows(torch, config, data, off, W, with_fields=True):
    """lc_csv_device over the packed bytes; every output array is pre-filled with the sentinel and guarded on both sides"""
    n = len(off) - 1
    dev = torch.device("cuda:0")
    full, d_out, rows = {}, {}, {}
    for k, (shape, dtype) in csv_decode.out_shapes(n, W).items():  # byte buffers: (GUARD rows, the n rows, GUARD rows), all sentinel
        rows[k] = int(np.prod(shape[1:])) * np.dtype(dtype).itemsize
        full[k] = torch.full(((n + 2 * GUARD) * rows[k] + 16,), SENT, dtype=torch.uint8, device=dev)
        d_out[k] = full[k][GUARD * rows[k]:(GUARD + n) * rows[k]] if rows[k] and n else None
    d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)
    csv_decode.read_device(proc(config), d_data, d_off, n, W, d_out["status"], d_out["count"], d_out["fields"] if with_fields else None,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = {}
    for k, (shape, dtype) in csv_decode.out_shapes(n, W).items():
        raw = full[k].cpu().numpy()
        assert (raw[:GUARD * rows[k]] == SENT).all() and (raw[(GUARD + n) * rows[k]:] == SENT).all(), "%s: a guard row was written" % k
        res[k] = raw[GUARD * rows[k]:(GUARD + n) * rows[k]].view(dtype).reshape(shape)
    return res


@functools.lru_cache(maxsize=None)
def model_answer(sep, trim, value):
    return cc.fields_of(cc.result_text({"SplitSep": sep.decode("utf-8"), "TrimLeadingSpace": trim}, value))


def against_model(got, config, values, W, what):
    """status, the TRUE count, the texts of the first min(count, W) fields -- and nothing written behind them.  An error value is compared
    on its status alone (its count and rows are unspecified), never skipped.  -> {status code: values}"""
    untouched = np.full(4, SENT, np.uint8).view(np.int32)[0]
    sep, trim = cc.reader_config(config)
    seen = {0: 0, 1: 0, 2: 0, 3: 0}
    for i, value in enumerate(values):
        code, fields = model_answer(sep, trim, value)
        seen[code] += 1
        assert got["status"][i] == code, (what, i, value[:100], "status %d, the model says %d" % (got["status"][i], code))
        if code >= 2:
            continue
        if code == 1:
            assert got["count"][i] == 0 and (got["fields"][i] == untouched).all(), (what, i, value[:100], "io.EOF with a count or a row")
            continue
        assert got["count"][i] == len(fields), (what, i, value[:100], int(got["count"][i]), len(fields))
        k = min(len(fields), W)
        texts = csv_decode.field_texts(value, got["fields"][i], k)
        assert texts == fields[:k], (what, i, value[:100], texts, fields[:k])
        assert (got["fields"][i][k:] == untouched).all(), (what, i, value[:100], "a row behind min(count, W) was written")
    return seen


def check(torch, config, values, W=8, pad_front=0, what="device"):
    data, off = pack(config, values, pad_front)
    return against_model(device_rows(torch, config, data, off, W), config, values, W, what)


def test_fixture_cases_in_batches_device_and_host_entry():
    """every named, unit and random case: per configuration one launch over all of them and the same values through the host entry, then
    the same list again in batches of n = 1, 63, 64, 65 and 257 -- a partial wavefront, a full one, one lane over, a second workgroup
    with one live lane"""
    torch = _torch()
    groups = cc.cases_by_config(cc.all_cases())
    assert len(groups) >= 5 and sum(len(c) for _, c in groups) > 10000
    seen = {0: 0, 1: 0, 2: 0, 3: 0}
    for config, cases in groups:
        values = [v for _, _, v, _ in cases]
        for (label, _, v, result) in cases[:60]:
            assert cc.result_text(config, v) == result, label  # (the model still gives what the files record)
        for code, k in check(torch, config, values, W=8, pad_front=len(values) % 16, what="device %r" % (config,)).items():
            seen[code] += k
        got = csv_decode.read_host(proc(config), values, W=8, fill=SENT)
        against_model(got, config, values, 8, "host entry %r" % (config,))
        at = round_ = 0
        while at < len(values):  # the whole list again, cut into batches of 1, 63, 64, 65, 257, 1, ... values (the last one as it falls)
            n = BATCHES[round_ % len(BATCHES)]
            check(torch, config, values[at:at + n], W=3, pad_front=(at + round_) % 16, what="n = %d at %d of %r" % (n, at, config))
            at += n
            round_ += 1
        assert round_ >= 2 * len(BATCHES)
    assert seen[0] > 4000 and seen[2] > 1000 and seen[3] > 1000 and seen[1] > 100, seen
    assert "csv_split_kernel" in csv_decode.binding.launched_kernels()


# the event byte of each kind stands on byte p of its value: (what stands before the filler, what stands from p on, config, filler)
COMMA, COMMA_TRIM, WIDE_SEP = {"SplitSep": ","}, {"SplitSep": ",", "TrimLeadingSpace": True}, {"SplitSep": cc.WIDE}
BORDER_KINDS = {
    "separator": (b"a,b", b",c,d", COMMA, b"x"),
    "three_byte_separator_first_byte": (b"a" + WIDE + b"b", WIDE + b"c" + WIDE + b"d", WIDE_SEP, b"x"),
    "three_byte_separator_second_byte": (b"a" + WIDE + b"b", WIDE[1:] + b"c" + WIDE + b"d", WIDE_SEP, b"x"),
    "three_byte_separator_third_byte": (b"a" + WIDE + b"b", WIDE[2:] + b"c" + WIDE + b"d", WIDE_SEP, b"x"),
    "three_byte_separator_behind_a_closing_quote": (b'a' + WIDE + b'"b', WIDE + b"c", WIDE_SEP, b"x"),
    "second_quote_of_a_doubled_quote": (b'a,"b', b'"c",d', COMMA, b"x"),
    "lf_of_crlf_inside_quotes": (b'a,"b', b'\nc",d\ne', COMMA, b"x"),
    "closing_quote": (b'a,"b', b'",c', COMMA, b"x"),
    "closing_quote_then_crlf": (b'a,"b', b'"\r\nc', COMMA, b"x"),
    "lf_behind_cr_unquoted": (b"a,b", b"\nc,d", COMMA, b"x"),
    "first_byte_behind_a_trim": (b"a,", b'b,"c"', COMMA_TRIM, b" "),
    "quote_behind_a_trim": (b"a,", b'"b ""c",d', COMMA_TRIM, b"\t"),
    "last_byte_of_a_trimmed_rune": (b"a,", b"\x80b,c", COMMA_TRIM, b" "),
}


@functools.lru_cache(maxsize=None)
def border_values(kind):
    """-> [(value, residue)]: the kind's event byte on offset p of its value, the value whole and cut right behind that byte, for all 16
    residues of the value's first byte"""
    before, after, _, filler = BORDER_KINDS[kind]
    out = []
    for p in OFFSETS:
        fill = filler * (p - len(before))
        if kind in ("second_quote_of_a_doubled_quote", "three_byte_separator_behind_a_closing_quote"):
            fill = fill[:-1] + b'"'
        elif kind in ("lf_of_crlf_inside_quotes", "lf_behind_cr_unquoted"):
            fill = fill[:-1] + b"\r"
        elif kind == "three_byte_separator_second_byte":
            fill = fill[:-1] + WIDE[:1]
        elif kind == "three_byte_separator_third_byte":
            fill = fill[:-2] + WIDE[:2]
        elif kind == "last_byte_of_a_trimmed_rune":
            fill = fill[:-2] + b"\xe2\x80"
        whole = before + fill + after
        assert len(before) + len(fill) == p
        for residue in range(16):
            out.append((whole, residue))
            out.append((whole[:p + 1], residue))
    return out


@pytest.mark.parametrize("kind", sorted(BORDER_KINDS))
def test_event_bytes_on_the_borders_for_every_alignment(kind):
    """a separator, each byte of a three-byte separator, the second quote of `""`, the `\\n` of `\\r\\n` inside quotes, a closing quote, the
    first byte behind a trim on offsets 15 .. 128, the value's first byte on every residue: the quad and the 64-byte stage fall on each"""
    torch = _torch()
    config = BORDER_KINDS[kind][2]
    wanted = border_values(kind)
    assert len(wanted) == len(OFFSETS) * 16 * 2
    values = at_residues(config, wanted)
    seen = check(torch, config, values, W=6, what=kind)
    assert seen[0] >= len(wanted) // 2
    got = csv_decode.read_host(proc(config), values[:300], W=6, fill=SENT)
    against_model(got, config, values[:300], 6, kind + ", host entry")


def test_field_counts_around_w_and_w_zero():
    torch = _torch()
    W = 4
    values = [",".join('"v""%d"' % i if i % 3 == 2 else "v%d" % i for i in range(n)).encode() for n in (W - 1, W, W + 1, 1, 3 * W, W)] + [b"", b'a"b', b'"a']
    data, off = pack(COMMA, values, 3)
    got = device_rows(torch, COMMA, data, off, W)
    against_model(got, COMMA, values, W, "around W")
    assert got["count"][:7].tolist() == [W - 1, W, W + 1, 1, 3 * W, W, 0] and got["status"].tolist() == [0] * 6 + [1, 2, 3]
    for with_fields in (True, False):  # W = 0: the counts alone, fields may be NULL
        got = device_rows(torch, COMMA, data, off, 0, with_fields=with_fields)
        against_model(got, COMMA, values, 0, "W = 0")
    got = csv_decode.read_host(proc(COMMA), values, W=0, fill=SENT)
    against_model(got, COMMA, values, 0, "W = 0, host entry")


def test_an_empty_value_between_two_long_ones_and_a_70000_byte_value():
    torch = _torch()
    long_a = ",".join('"v ""%d"""' % i if i % 2 else "v%d" % i for i in range(400)).encode()
    long_b = b'a,"never closed ' + b"x,y\r\n" * 300
    big = (",".join("k%d" % i for i in range(40)) + ',"' + "y\r\n" * 24000 + '",tail,"a ""b"""\r\nsecond,record').encode()
    assert len(big) > 70000
    values = [long_a, b"", long_b, b"", b"", big, b"a,1"]
    seen = check(torch, COMMA, values, W=48, pad_front=7, what="empty between long, 70 000 bytes")
    assert seen == {0: 3, 1: 3, 2: 0, 3: 1}


def test_argument_errors():
    torch = _torch()
    dev = torch.device("cuda:0")
    data, off = pack(COMMA, [b"a,b"])
    d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)
    status = torch.zeros(16, dtype=torch.uint8, device=dev)
    count = torch.zeros(4, dtype=torch.int32, device=dev)
    raw = torch.full((8 * 8 + 32,), SENT, dtype=torch.uint8, device=dev)
    L, h = csv_decode.load(), proc(COMMA).handle
    aligned = raw.data_ptr() + (-raw.data_ptr()) % 16
    args = (h, d_data.data_ptr(), d_off.data_ptr(), 1, 8, status.data_ptr(), count.data_ptr())
    for shift in (2, 4, 12):  # fields is written as 8-byte vectors
        assert L.lc_csv_device(*args, aligned + shift, None) == 5
    assert L.lc_csv_device(*args, None, None) == 5  # NULL fields with W > 0
    assert L.lc_csv_device(None, *args[1:], aligned, None) == 5
    assert L.lc_csv_device(h, d_data.data_ptr(), d_off.data_ptr(), 1, 8, status.data_ptr(), count.data_ptr() + 2, aligned, None) == 5
    assert L.lc_csv_device(h, None, None, 0, 8, None, None, None, None) == 0  # n = 0 touches nothing: not even its pointers
    invalid = csv_decode.Processor(SplitSep='"', SplitKeys=["a"])
    assert L.lc_csv_device(invalid.handle, *args[1:], aligned, None) == 2  # LC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (raw.cpu().numpy() == SENT).all() and int(count.sum()) == 0
    assert L.lc_csv_device(*args, aligned + 8, None) == 0
    torch.cuda.synchronize()
    assert count[0].item() == 2
    logs = [[("c", "a,b")]]
    assert invalid.process_logs(logs) == logs and invalid.counters()["decode_errors"] == 1 and invalid.counters()["values"] == 0
    assert invalid.collect_alarms() == [(csv_decode.LC_CSV_ALARM_DECODE, b"cannot decode log:csv: invalid field or comment delimiter\tlog:a,b\t")]


def test_the_unit_tests_cases_through_the_processor():
    _torch()
    unit, _ = cc.load_fixtures()
    for e in unit["cases"]:  # (KeepSource: the test calls decodeCSV directly, so its source stays)
        p = csv_decode.Processor(**dict(e["config"], SourceKey="content", KeepSource=True))
        got = p.process_logs([[("content", e["value"])]])[0]
        assert got[0] == ("content", e["value"]) and [list(kv) for kv in got[1:]] == e["appended"], e["case"]
        assert e["contents"] is None or len(got) == e["contents"], e["case"]
        for i, v in e["values"].items():
            assert got[int(i)][1] == v, (e["case"], i)


@pytest.mark.parametrize("preserve,expand", [(False, False), (True, False), (True, True)])
def test_processor_on_a_1000_log_batch_with_the_mop_up(preserve, expand):
    """lc_csv_process_logs_json on the device against the same processor code over the CPU double, and both against the model; the mop-up
    trip forced by lc_csv_set_first_trip_fields(1)"""
    _torch()
    config = dict(SplitKeys=["f1", "f2", "f3"], SourceKey="content", KeepSource=False, PreserveOthers=preserve, ExpandOthers=expand, ExpandKeyPrefix="x_",
                  TrimLeadingSpace=True, NoKeyError=True)
    values = [v.decode("utf-8") for v in cc.random_values(config, 31, 980, longest=60)]
    values += [",".join('"v,""%d"' % i if i % 4 == 1 else " v%d" % i for i in range(n)) for n in (3, 17, 33, 40, 5, 2, 1, 64)] + ["", "\n", '"a\r\nb",c']
    logs = [[("host", "h%d" % i), ("content", v)] if i % 7 else [("host", "only")] for i, v in enumerate(values)]
    on_device, on_double = csv_decode.Processor(**config), cc.processor(**config)
    for p in (on_device, on_double):
        p.set_first_trip_fields(1)
    got, want = on_device.process_logs(logs), on_double.process_logs(logs)
    assert got == want == cc.model_logs(config, logs)[0]
    c = on_device.counters()
    assert c == on_double.counters() and c["mop_up"] > 100 and c["decode_errors"] > 100 and c["eof_values"] > 2 and c["key_count"] > 100
    assert c["no_source_key"] == len([1 for i in range(len(values)) if i % 7 == 0]) and c["values"] == len(values) - c["no_source_key"]
    alarms = on_device.collect_alarms()
    assert alarms == on_double.collect_alarms() == cc.model_logs(config, logs)[1]
    texts = [t for _, t in alarms]
    assert any(t.startswith(b'cannot decode log:bare " in non-quoted-field\tlog:') for t in texts)
    assert any(t.startswith(b'cannot decode log:extraneous or missing " in quoted-field\tlog:') for t in texts)
    assert any(t.startswith(b"decode keys not match, split len:40\tlog:") for t in texts) and b"cannot find key:content\t" in texts
    assert got[-1] == [("host", "h%d" % (len(values) - 1)), ("f1", "a\nb"), ("f2", "c")]
