"""The field codecs on the CPU: the per-unit routines of csrc/codec_vm.hpp compiled for the host (a stand-alone program,
tests/native/codec_host_check.cpp, plain and under AddressSanitizer + UBSan, each run as its own process) and the product's processor
code over the host double of the device trip (tests/native/codec_double.cpp), both against tests/helpers/codec_model.py.  The routines
are never their own reference.  Fixtures: tests/golden/README_codec.md."""
import ctypes

import pytest

from helpers import codec_cases as cc
from helpers import codec_model as model
from helpers import codec_product as cp
from loongcollector_amd import codec


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return cc.build_host_check(tmp_path_factory.mktemp("codec_host_check"))


def _differences(exe, path, pairs):
    got = cc.run_host_check(exe, path, pairs)
    return [(op, value[:80], g[:120]) for (op, value), g in zip(pairs, got) if g != cc.expected_text(op, value)]


def test_host_routines_equal_the_model_on_the_whole_corpus(program, tmp_path):
    """encode, MD5, and the decode's size pass at all 16 alignments of the first byte (the program compares them among themselves) with
    the write pass behind it, clean values through the compacting path as well"""
    pairs = [(op, v) for op in model.OPS for _, v in cc.cases(op)]
    assert len(pairs) > 10000
    bad = _differences(program, tmp_path / "cases.bin", pairs)
    assert not bad, bad[:10]
    outcomes = {cc.expected_text("base64_decode", v).split()[0] for _, v in cc.decode_cases()}
    assert outcomes == {"1", "2"}


def test_sanitized_host_check_program(tmp_path):
    """the same stand-alone program under AddressSanitizer + UBSan, as a child process, once: every value from an exactly-sized heap copy,
    the output in an exactly-sized block"""
    exe = cc.build_host_check(tmp_path, sanitize=True)
    pairs = [(op, v) for op in model.OPS for _, v in cc.cases(op)[::3]]
    bad = _differences(exe, tmp_path / "cases.bin", pairs)
    assert not bad, bad[:5]


# ---------------------------------------------------------------------------------------------- the processor
TEXT = "a NUL \x00, 啊 and 🙂"
BATCH = [
    [("src", "123")],
    [("host", "h"), ("src", "MTIz"), ("src", "second: never visited"), ("tail", "t")],   # the FIRST content with the key only
    [("other", "no source here")],
    [("src", "")],
    [("src", "test_value"), ("src", "MTIz")],                                            # the first one fails: nothing is appended
    [],
    [("src", model.encode(TEXT.encode("utf-8")).decode())],
    [("src", "QUJD\r\nREU=\r\n")],
    [("src", TEXT)],
    [("src", "QUJDRE=x")],
]
CONFIGS = [
    {"Op": "base64_encode", "SourceKey": "src", "NewKey": "dest"},
    {"Op": "base64_encode", "SourceKey": "src", "NewKey": "", "NoKeyError": True},
    {"Op": "base64_encode", "SourceKey": "src", "NewKey": "src"},
    {"Op": "base64_decode", "SourceKey": "src", "NewKey": "dest", "DecodeError": True, "NoKeyError": True},
    {"Op": "base64_decode", "SourceKey": "src", "NewKey": "", "DecodeError": False, "NoKeyError": False},
    {"Op": "md5", "SourceKey": "src", "MD5Key": "digest", "NoKeyError": True},
    {"Op": "md5", "SourceKey": "", "MD5Key": "digest"},                                  # an empty SourceKey matches an empty key
]


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "%s-%s" % (c["Op"], c.get("NewKey", c.get("MD5Key")) or "nokey"))
def test_processor_equals_the_models_process_logs(config):
    batch = BATCH + [[("", "the empty key")]]
    p = cp.processor(**config)
    want, alarms, counters = model.process_logs(config, batch)
    assert p.process_logs(batch) == want
    assert p.collect_alarms() == alarms
    assert p.counters() == counters and counters["failed_trips"] == 0
    if config["SourceKey"] == "":
        assert counters["values"] == 1 and want[-1] == [("", "the empty key"), ("digest", model.md5_hex(b"the empty key").decode())]
        return
    assert counters["values"] == 8 and counters["no_key"] == 3
    assert want[2] == batch[2] and want[5] == []
    no_key = (codec.LC_CODEC_ALARM_NO_KEY, b"cannot find key:src\t")
    if config["Op"] == "base64_encode":
        assert counters["out"] == 8 and alarms == ([no_key] * 3 if config.get("NoKeyError") else [])
        if config["NewKey"] == "":
            assert want[0] == [("src", "MTIz")] and want[3] == [("src", "")]             # replaced in place
            assert want[1] == [("host", "h"), ("src", "TVRJeg=="), ("src", "second: never visited"), ("tail", "t")]
        else:
            assert want[0] == [("src", "123"), (config["NewKey"], "MTIz")] and want[3] == [("src", ""), (config["NewKey"], "")]
            assert want[1] == batch[1] + [(config["NewKey"], "TVRJeg==")]
    elif config["Op"] == "base64_decode":
        assert counters["out"] == 4 and counters["decode_errors"] == 4
        assert want[1] == batch[1] + [(config["NewKey"], "123")]                         # appended, also under the empty key
        assert want[4] == batch[4] and want[0] == batch[0]                               # a failure appends nothing
        assert want[6] == batch[6] + [(config["NewKey"], TEXT)] and want[7] == batch[7] + [(config["NewKey"], "ABCDE")]
        assert want[3] == [("src", ""), (config["NewKey"], "")]
        if config["DecodeError"]:
            decode = [a for a in alarms if a[0] == codec.LC_CODEC_ALARM_DECODE]
            assert decode == [(1, b"decode base64 error:illegal base64 data at input byte 0\t"),
                              (1, b"decode base64 error:illegal base64 data at input byte 4\t"),
                              (1, b"decode base64 error:illegal base64 data at input byte 1\t"),
                              (1, b"decode base64 error:illegal base64 data at input byte 6\t")]
            assert alarms.count(no_key) == 3
        else:
            assert alarms == []
    else:
        assert counters["out"] == 8 and alarms == [no_key] * 3
        assert want[0] == [("src", "123"), ("digest", "202cb962ac59075b964b07152d234b70")]
        assert want[3] == [("src", ""), ("digest", "d41d8cd98f00b204e9800998ecf8427e")]


def test_unit_test_vectors_through_the_processor():
    for e in cc.load_vectors()["cases"]:
        p = cp.processor(**e["config"])
        assert [list(kv) for kv in p.process_logs([[tuple(kv) for kv in e["log"]]])[0]] == e["contents"], e["case"]
        assert p.collect_alarms() == [(a["kind"], a["text"].encode()) for a in e["alarms"]], e["case"]
        for a in e["alarms"]:
            assert a["text"].startswith(a.get("text_begins", a["text"]))


def test_apply_equals_the_model_on_a_slice_of_the_corpus():
    """Processor.apply over the double: flags, bytes, lengths and error offsets of one trip"""
    for op in model.OPS:
        values = [v for _, v in cc.cases(op)[::7]]
        assert cp.processor(Op=op).apply(values) == [model.apply(op, v) for v in values], op


def test_one_trip_per_batch_and_none_without_a_source():
    L = cp.double()
    p = cp.processor(**CONFIGS[0])
    before = cp.trip_stats(L)
    p.process_logs(BATCH)
    after = cp.trip_stats(L)
    assert after["trips"] - before["trips"] == 1 and after["values"] - before["values"] == 8
    assert p.process_logs([[("x", "y")], []]) == [[("x", "y")], []] and cp.trip_stats(L)["trips"] == after["trips"]
    assert p.counters()["values"] == 8 and p.counters()["no_key"] == 4


def test_failed_trip_leaves_every_log_unchanged_and_is_reported():
    L = cp.double()
    p = cp.processor(**CONFIGS[3])
    logs = [[("src", "MTIz")], [("other", "x")], [("src", "bad!")]]
    L.cd_fail_next_trips(1)
    with pytest.raises(RuntimeError):
        p.process_logs(logs)
    assert p.counters() == {"values": 0, "out": 0, "decode_errors": 0, "no_key": 0, "failed_trips": 1}
    heard = p.collect_alarms()
    assert [k for k, _ in heard] == [codec.LC_CODEC_ALARM_TRIP_FAILED] and b"3 logs left unchanged" in heard[0][1]
    assert p.process_logs(logs) == model.process_logs(CONFIGS[3], logs)[0] and p.counters()["failed_trips"] == 1


def _create(text):
    handle, err = ctypes.c_void_p(), ctypes.create_string_buffer(256)
    rc = cp.double().lc_codec_create(text, len(text), ctypes.byref(handle), err, 256)
    assert (rc == 0) == bool(handle.value)
    if handle.value:
        cp.double().lc_codec_free(handle)
    return rc, err.value


def test_create_refusals_through_the_double():
    for text in (b"{}", b'{"SourceKey": "src"}', b'{"Op": "base32"}', b'{"Op": 7}', b'{"Op": "MD5"}', b'{"Op": ""}'):
        rc, err = _create(text)
        assert rc == 5 and b"Op" in err and b"base64_encode" in err, text
    rc, err = _create(b"[1, 2]")
    assert rc == 5 and b"JSON object" in err
    for op in model.OPS:  # nothing else is refused: no key at all, keys of other plugins
        assert _create(b'{"Op": "%s"}' % op.encode()) == (0, b"")
        assert _create(b'{"Op": "%s", "SourceKey": "", "NewKey": "", "MD5Key": "", "Match": "x", "NoKeyError": 1}' % op.encode())[0] == 0
    with pytest.raises(codec.CodecInitError) as e:
        cp.processor(Op="rot13")
    assert e.value.code == 5 and "rot13" in str(e.value)
