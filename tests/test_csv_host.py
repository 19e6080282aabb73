"""processor_csv on the CPU: the per-value routine of csrc/csv_vm.hpp compiled for the host (a stand-alone program,
tests/native/csv_host_check.cpp, plain and under AddressSanitizer + UBSan) and the product's processor code over the host double of the
device trip (tests/native/csv_double.cpp), both against tests/helpers/csv_model.py -- the reader rules restated line by line.  The
routine is never its own reference.  Fixtures: tests/golden/README_csv.md."""
import ctypes
import itertools

import pytest

from helpers import csv_cases as cc
from helpers import csv_model
from loongcollector_amd import csv_decode

RANDOM_CONFIGS = [{"SplitSep": ","}, {"SplitSep": ",", "TrimLeadingSpace": True}, {"SplitSep": cc.WIDE}, {"SplitSep": cc.WIDE, "TrimLeadingSpace": True},
                  {"SplitSep": "\t", "TrimLeadingSpace": True}, {"SplitSep": "é"}, {"SplitSep": "\U0001F600", "TrimLeadingSpace": True},
                  {"SplitSep": "a"}, {"SplitSep": " ", "TrimLeadingSpace": True}]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return cc.build_host_check(tmp_path_factory.mktemp("csv_host_check"))


def _differences(exe, cases):
    got = cc.run_host_check(exe, [(config, value) for _, config, value, _ in cases])
    return [(label, value, result, g) for (label, _, value, result), g in zip(cases, got) if g != result]


def _random_cases(longest, per_config, seed):
    out = []
    for i, config in enumerate(RANDOM_CONFIGS):
        values = cc.random_values(config, seed + i, per_config, longest=longest)
        out += [("random:%d:%d" % (i, k), config, v, cc.result_text(config, v)) for k, v in enumerate(values)]
    return out


def test_host_routine_equals_the_model_on_every_fixture(program):
    """status, the true count and every field's text, at all 16 alignments of the first byte (the program compares them among themselves),
    through a source that answers separator, quote and line-end bytes outside the value and traps a read of the routine's own there"""
    bad = _differences(program, cc.all_cases())
    assert not bad, bad[:10]


def test_host_routine_equals_the_model_on_9000_random_values(program):
    """1000 seeded values of up to 200 bytes per configuration -- several stages, separators and runes across their borders, separators of
    1 to 4 bytes, a separator that is a white-space rune or a letter of the alphabet -- the model run live"""
    cases = _random_cases(200, 1000, 4000)
    bad = _differences(program, cases)
    assert not bad, bad[:5]
    errors = sum(1 for c in cases if c[3] in ("2", "3"))
    assert len(cases) == 9000 and 900 < errors < 8100


def test_sanitized_host_check_program(tmp_path):
    """the same stand-alone program under AddressSanitizer + UBSan, as a child process, once: every value from an exactly-sized heap copy,
    exactly count rows to write into"""
    exe = cc.build_host_check(tmp_path, sanitize=True)
    cases = cc.all_cases()
    named = [c for c in cases if not c[0].startswith("random:")]
    sample = named + [c for c in cases if c[0].startswith("random:")][::4] + _random_cases(300, 40, 77)
    bad = _differences(exe, sample)
    assert not bad, bad[:5]


# value-only mutations of csrc/csv_vm.hpp, each rebuilt from a mutated copy in a scratch tree; each must fail the check named beside it
MUTATIONS = {
    "crlf_fold_inside_quotes_removed": ("else if (raw[i] == '\\r' && i + 1 < n && raw[i + 1] == '\\n') continue;", "", "named:crlf_inside_quotes:1"),
    "empty_line_test_behind_the_trim": ("    if (w.phase == kCsvLine) {  // empty lines, before any trimming",
                                        "    if (w.phase == kCsvLine && Trim && (c == ' ' || c == '\\t')) return;\n    if (w.phase == kCsvLine) {",
                                        "named:trim_blanks_only_line:1"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutations_are_caught(name, program, tmp_path):
    old, new, caught_by = MUTATIONS[name]
    cases = [c for c in cc.all_cases() if not c[0].startswith("random:wide") and not c[0].startswith("random:semicolon")]
    bad = _differences(cc.mutated_host_check(tmp_path, old, new), cases)
    labels = {b[0] for b in bad}
    assert caught_by in labels and len(labels) >= 3, sorted(labels)[:10]
    if name == "crlf_fold_inside_quotes_removed":
        assert "named:quoted_field_over_three_lines:1" in labels and all(b"\r\n" in b[1] for b in bad)
    else:  # (only trimming configurations, only values with a line of blanks or tabs before the record)
        config_of = {c[0]: c[1] for c in cases}
        assert "named:trim_empty_line_test_comes_first:1" in labels and all(config_of[b[0]].get("TrimLeadingSpace") for b in bad)
    assert not _differences(program, cases[:80])  # (the unmutated routine, same walk)


# ---------------------------------------------------------------------------------------------- the processor
KEYS = ["f1", "f2", "f3"]
BATCH = [
    [("content", '12,34,56')],
    [("time", "12:00"), ("content", '"normal","""quote""",",",more,"x\r\ny"'), ("content", "second,source")],  # only the first source
    [("other", "no source here")],
    [("content", "")],
    [("content", '  12,  ,"  34",  78,  ,"  90", tail')],
    [("content", '12",34,56')],
    [("content", '"12"  ,34,56')],
    [("f1", "pre-existing"), ("content", "a,b"), ("tail", "t")],
    [("content", "\n\r\n")],
    [("content", 'a,b,c,\\.,d e,"", x')],
    [],
]


@pytest.mark.parametrize("keep,preserve,expand,trim", list(itertools.product([False, True], repeat=4)))
def test_processor_equals_the_models_process_log(keep, preserve, expand, trim):
    config = dict(SplitKeys=KEYS, SourceKey="content", KeepSource=keep, PreserveOthers=preserve, ExpandOthers=expand, ExpandKeyPrefix="expand_",
                  TrimLeadingSpace=trim, NoKeyError=True)
    p = cc.processor(**config)
    want, alarms = cc.model_logs(config, BATCH)
    got = p.process_logs(BATCH)
    assert got == want
    assert p.collect_alarms() == alarms
    kinds = [k for k, _ in alarms]
    c = p.counters()
    assert c["no_source_key"] == kinds.count(csv_decode.LC_CSV_ALARM_NO_SOURCE_KEY) == 2
    assert c["decode_errors"] == kinds.count(csv_decode.LC_CSV_ALARM_DECODE) == 2 and c["key_count"] == kinds.count(csv_decode.LC_CSV_ALARM_KEY_COUNT) == 6
    assert c["values"] == 9 and c["eof_values"] == 2 and c["failed_trips"] == 0
    removed = 0 if keep else 7  # sources taken out: every value that decoded
    assert c["fields"] == sum(len(w) - len(b) for w, b in zip(want, BATCH)) + removed
    assert got[5] == BATCH[5] and got[6] == BATCH[6]  # an error value keeps its source whatever KeepSource says
    assert (csv_decode.LC_CSV_ALARM_DECODE, b'cannot decode log:bare " in non-quoted-field\tlog:12",34,56\t') in alarms
    assert (csv_decode.LC_CSV_ALARM_DECODE, b'cannot decode log:extraneous or missing " in quoted-field\tlog:"12"  ,34,56\t') in alarms
    assert (csv_decode.LC_CSV_ALARM_KEY_COUNT, b"decode keys not match, split len:1\tlog:\t") in alarms
    assert (csv_decode.LC_CSV_ALARM_NO_SOURCE_KEY, b"cannot find key:content\t") in alarms
    tail = got[1][len(BATCH[1]) - (0 if keep else 1):]
    assert tail[:3] == [("f1", "normal"), ("f2", '"quote"'), ("f3", ",")]
    if preserve and expand:
        assert tail[3:] == [("expand_1", "more"), ("expand_2", "x\ny")]
    elif preserve:
        assert tail[3:] == [("_decode_preserve_", 'more,"x\ny"')]
        assert got[9][-1] == ("_decode_preserve_", '"\\.",d e,," x"' if not trim else '"\\.",d e,,x')
    else:
        assert tail[3:] == []


def test_the_unit_tests_cases_through_the_processor():
    unit, _ = cc.load_fixtures()
    for e in unit["cases"]:  # (KeepSource: the test calls decodeCSV directly, so its source stays)
        p = cc.processor(**dict(e["config"], SourceKey="content", KeepSource=True))
        got = p.process_logs([[("content", e["value"])]])[0]
        assert got[0] == ("content", e["value"]) and [list(kv) for kv in got[1:]] == e["appended"], e["case"]
        assert e["contents"] is None or len(got) == e["contents"], e["case"]
        assert (p.counters()["decode_errors"] == 1) == (not e["res"]), e["case"]


def test_empty_split_keys_never_reach_the_trip_and_nokeyerror_guards_the_alarm():
    L = cc.double()
    before = cc.trip_stats(L)
    logs = [[("content", 'a"b,c')], [("x", "y")]]
    for keep, preserve in itertools.product([False, True], repeat=2):
        config = dict(SplitKeys=[], SourceKey="content", KeepSource=keep, PreserveOthers=preserve)
        p = cc.processor(**config)
        want, alarms = cc.model_logs(config, logs)
        assert p.process_logs(logs) == want and p.collect_alarms() == alarms == []
        assert want[0] == ([("content", 'a"b,c')] if keep else []) + ([("_decode_preserve_", 'a"b,c')] if preserve else [])
        assert p.counters()["values"] == 0 and p.counters()["fields"] == int(preserve) and p.counters()["no_source_key"] == 1
    assert cc.trip_stats(L) == before
    p = cc.processor(SplitKeys=KEYS, SourceKey="content", NoKeyError=False)
    assert p.process_logs([[("x", "y")]]) == [[("x", "y")]] and p.collect_alarms() == [] and p.counters()["no_source_key"] == 1
    p = cc.processor(SplitKeys=KEYS)  # an empty SourceKey takes a log's first content
    assert p.process_logs([[("x", "1,2,3"), ("y", "4,5,6")]]) == [[("y", "4,5,6"), ("f1", "1"), ("f2", "2"), ("f3", "3")]]


@pytest.mark.parametrize("sep", ['"', "\r", "\n", "\0", "�"])
def test_an_invalid_delimiter_fails_every_value_without_a_trip(sep):
    L = cc.double()
    before = cc.trip_stats(L)
    config = dict(SplitKeys=KEYS, SplitSep=sep, SourceKey="content", KeepSource=False)
    logs = [[("content", "a,b,c")], [("content", "x" * 2000)], [("other", "o")]]
    p = cc.processor(**config)
    want, alarms = cc.model_logs(config, logs)
    assert p.process_logs(logs) == want == logs and p.collect_alarms() == alarms
    assert alarms[0] == (csv_decode.LC_CSV_ALARM_DECODE, b"cannot decode log:csv: invalid field or comment delimiter\tlog:a,b,c\t")
    assert alarms[1][1].endswith(b"\tlog:" + b"x" * 1024 + b"\t")  # util.CutString(value, 1024)
    assert p.counters()["decode_errors"] == 2 and p.counters()["values"] == 0 and cc.trip_stats(L) == before
    status, count = (ctypes.c_uint8 * 1)(), (ctypes.c_uint32 * 1)()
    line, length = (ctypes.c_char_p * 1)(b"a"), (ctypes.c_uint32 * 1)(1)
    assert L.lc_csv_host(p.handle, line, length, 1, 0, status, count, None) == 2  # LC_ERR_UNSUPPORTED
    # ... and with SplitKeys empty the reader is never asked
    q = cc.processor(SplitKeys=[], SplitSep=sep, PreserveOthers=True)
    assert q.process_logs([[("c", "v")]]) == [[("_decode_preserve_", "v")]] and q.collect_alarms() == []


def test_init_refuses_a_separator_that_is_not_one_rune():
    for sep in ("", ",,", "ab", "，，"):
        with pytest.raises(csv_decode.CsvInitError, match="invalid separator: " + sep):
            cc.processor(SplitKeys=KEYS, SplitSep=sep)
    for sep in ("é", cc.WIDE, "\U0001F600"):
        p = cc.processor(SplitKeys=KEYS, SplitSep=sep)
        assert p.process_logs([[("c", sep.join('1 "2" 3'.split()))]]) == [[("f1", "1"), ("f2", "2"), ("f3", "3")]]
    handle, err = ctypes.c_void_p(), ctypes.create_string_buffer(256)
    assert cc.double().lc_csv_create(b"[1, 2]", 6, ctypes.byref(handle), err, 256) != 0 and not handle.value and b"JSON object" in err.value
    p = cc.processor(SplitKeys=KEYS)  # SplitSep defaults to `,`
    assert p.process_logs([[("c", "1,2,3")]]) == [[("f1", "1"), ("f2", "2"), ("f3", "3")]]


@pytest.mark.parametrize("preserve,W", [(True, 1), (True, 4), (False, 1), (False, 2)])
def test_mop_up_is_one_trip_at_the_largest_count_needed(preserve, W):
    L = cc.double()
    counts = [1, W, W + 1, 3, 25, 2, 40]
    logs = [[("content", ",".join('"v""%d"' % i if i % 5 == 4 else "v%d" % i for i in range(n)))] for n in counts]
    config = dict(SplitKeys=KEYS, SourceKey="content", PreserveOthers=preserve)
    p = cc.processor(**config)
    p.set_first_trip_fields(W)
    before = cc.trip_stats(L)
    assert p.process_logs(logs) == cc.model_logs(config, logs)[0]
    after = cc.trip_stats(L)
    needed = [n if preserve else min(n, 3) for n in counts]
    wide = sum(1 for n in needed if n > W)
    assert after["trips"] - before["trips"] == 2 and after["values"] - before["values"] == len(logs) + wide and after["last_W"] == max(needed)
    assert p.counters()["mop_up"] == wide and p.counters()["key_count"] == sum(1 for n in counts if n != 3)
    # the default sizes: len(SplitKeys), + 16 with PreserveOthers -- one trip unless a value holds more
    q = cc.processor(**config)
    q.process_logs(logs[:4])
    assert cc.trip_stats(L)["trips"] - after["trips"] == 1 and cc.trip_stats(L)["last_W"] == 3 + (16 if preserve else 0) and q.counters()["mop_up"] == 0
    q.process_logs(logs)
    assert q.counters()["mop_up"] == (2 if preserve else 0)
    # no source value at all: no trip
    trips = cc.trip_stats(L)["trips"]
    assert q.process_logs([[("x", "y")], []]) == [[("x", "y")], []] and cc.trip_stats(L)["trips"] == trips


def test_failed_trip_leaves_every_log_unchanged_and_is_reported():
    L = cc.double()
    p = cc.processor(SplitKeys=KEYS, SourceKey="content")
    logs = [[("content", "a,b,c")], [("other", "x")]]
    L.cd_fail_next_trips(1)
    with pytest.raises(RuntimeError):
        p.process_logs(logs)
    c = p.counters()
    assert c["failed_trips"] == 1 and c["values"] == c["fields"] == c["no_source_key"] == 0
    assert [k for k, _ in p.collect_alarms()] == [csv_decode.LC_CSV_ALARM_TRIP_FAILED]
    assert p.process_logs(logs) == [[("f1", "a"), ("f2", "b"), ("f3", "c")], [("other", "x")]] and p.counters()["failed_trips"] == 1
