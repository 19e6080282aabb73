"""processor_split_key_value on the CPU: the per-value routine of csrc/kv_vm.hpp compiled for the host (a stand-alone program,
tests/native/kv_host_check.cpp, plain and under AddressSanitizer + UBSan) and the product's processor code over the host double of the
device trip (tests/native/kv_double.cpp), both against tests/helpers/kv_model.py -- the Go restated line by line.  The routine is never
its own reference.  Fixtures: tests/golden/README_kv.md."""
import itertools

import pytest

from helpers import kv_cases as kc
from helpers import kv_model
from helpers import kv_product as kp
from loongcollector_amd import kvsplit

LOGFMT = {"Delimiter": " ", "Separator": "=", "Quote": "\""}
Q2 = {"Delimiter": " ", "Separator": "=", "Quote": "\"\""}
RANDOM_CONFIGS = [{}, LOGFMT, {"Delimiter": "#?#", "Separator": ": ", "Quote": "'"}, Q2, {"Delimiter": ",", "Separator": "=>", "Quote": "''"},
                  {"Delimiter": ":", "Separator": ":", "Quote": "\""}, {"Delimiter": "ab", "Separator": "ba", "Quote": "aba"},
                  {"Delimiter": "aa", "Separator": "a", "Quote": "a"}, {"Delimiter": "#D中文分隔#", "Separator": "#S中文分隔#", "Quote": "\"\"\""}]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return kc.build_host_check(tmp_path_factory.mktemp("kv_host_check"))


def _differences(exe, cases):
    got = kc.run_host_check(exe, [(config, value) for _, config, value, _ in cases])
    return [(label, value, rows, g) for (label, _, value, rows), g in zip(cases, got) if g != rows]


def test_host_routine_equals_the_model_on_every_fixture(program):
    """status, the true count and every span, at all 16 alignments of the first byte (the program compares them among themselves), through
    a source that answers delimiter, separator, quote and backslash bytes outside the value"""
    bad = _differences(program, kc.all_cases())
    assert not bad, bad[:10]


def test_host_routine_equals_the_model_on_9000_random_values(program):
    """1000 seeded values of up to 200 bytes per configuration -- several stages, needles across their borders -- the model run live"""
    total = panics = 0
    for i, config in enumerate(RANDOM_CONFIGS):
        values = kc.random_values(config, 4000 + i, 1000, longest=200)
        cases = [("random:%d:%d" % (i, k), config, v, kc.rows_text(config, v)) for k, v in enumerate(values)]
        bad = _differences(program, cases)
        assert not bad, bad[:5]
        total += len(cases)
        panics += sum(1 for c in cases if c[3] == kc.PANIC)
    assert total == 9000 and 0 < panics < 900


def test_sanitized_host_check_program(tmp_path):
    """the same stand-alone program under AddressSanitizer + UBSan, as a child process, once: every value from an exactly-sized heap copy,
    exactly npairs rows to write into"""
    exe = kc.build_host_check(tmp_path, sanitize=True)
    cases = kc.all_cases()
    named = [c for c in cases if not c[0].startswith("random:")]
    sample = named + [c for c in cases if c[0].startswith("random:")][::4]
    sample += [("long:%d" % k, RANDOM_CONFIGS[k % 5], v, kc.rows_text(RANDOM_CONFIGS[k % 5], v))
               for k, v in enumerate(v for i in range(5) for v in kc.random_values(RANDOM_CONFIGS[i], 77 + i, 60, longest=300))]
    bad = _differences(exe, sample)
    assert not bad, bad[:5]


# value-only mutations of csrc/kv_vm.hpp, each rebuilt from a mutated copy in a scratch tree; each must fail the check named beside it
MUTATIONS = {
    "separator_quote_at_zero_counts": ("return w.sqPos != kKvNone && w.sqPos > w.b &&", "return w.sqPos != kKvNone && w.sqPos >= w.b &&",
                                       "named:separator_quote_at_zero_is_not_above_zero"),
    "escaped_quote_not_skipped": ("if (pos >= w.sp + 2 && src.byteAt(head + pos - 2) == ' ' && src.byteAt(head + pos - 1) == '\\\\') {",
                                  "if (false && pos >= w.sp + 2 && src.byteAt(head + pos - 2) == ' ' && src.byteAt(head + pos - 1) == '\\\\') {",
                                  "named:escaped_once"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutations_are_caught(name, program, tmp_path):
    old, new, caught_by = MUTATIONS[name]
    cases = [c for c in kc.all_cases() if not c[0].startswith("random:wide") and not c[0].startswith("random:default")]
    bad = _differences(kp.mutated_host_check(tmp_path, old, new), cases)
    labels = {b[0] for b in bad}
    assert caught_by in labels and len(labels) >= 5, sorted(labels)[:10]
    if name == "escaped_quote_not_skipped":
        assert "unit:TestSplitWithQuote/1" in labels and all(b"\\" in b[1] for b in bad)  # (only values that hold a backslash)
    else:
        config_of = {c[0]: c[1] for c in cases}
        for label, value, _, _ in bad:  # (only values that hold Separator+Quote)
            _, separator, quote = kc.needles(config_of[label])
            assert separator + quote in value, label
    assert not _differences(program, cases[:80])  # (the unmutated routine, same walk)


# ---------------------------------------------------------------------------------------------- the processor
BATCH = [
    [("content", 'a=1 b="x y" c=3')],
    [("time", "12:00"), ("content", "k=v k=w k=v"), ("content", "second=source")],          # duplicates kept; only the first source
    [("other", "no source here")],
    [("content", "")],
    [("content", 'nosep =empty "quoted nosep" x="unterminated y=2 z=3')],
    [("content", "trailing=delimiter ")],
    [("k", "pre-existing"), ("content", "k=new =1 =2 lone lone2"), ("tail", "t")],
    [],
]


@pytest.mark.parametrize("keep,discard,empty_source", list(itertools.product([False, True], repeat=3)))
def test_processor_equals_the_models_process_log(keep, discard, empty_source):
    config = dict(LOGFMT, KeepSource=keep, DiscardWhenSeparatorNotFound=discard, SourceKey="" if empty_source else "content")
    p = kp.processor(**config)
    want, alarms = kp.model_logs(config, BATCH)
    assert p.process_logs(BATCH) == want
    assert p.collect_alarms() == alarms
    kinds = [k for k, _ in alarms]
    c = p.counters()
    assert c["no_source_key"] == kinds.count(kvsplit.LC_KV_ALARM_NO_SOURCE_KEY) == (1 if empty_source else 2)
    assert c["no_separator"] == kinds.count(kvsplit.LC_KV_ALARM_NO_SEPARATOR) > 0 and c["empty_keys"] == kinds.count(kvsplit.LC_KV_ALARM_EMPTY_KEY) > 0
    assert c["values"] == len(BATCH) - c["no_source_key"] and c["ref_panic"] == c["failed_trips"] == 0
    removed = 0 if keep else sum(1 for log in BATCH if any(empty_source or k == "content" for k, _ in log))  # sources taken out
    assert c["pairs"] == sum(len(w) - len(b) for w, b in zip(want, BATCH)) + removed
    if not empty_source and keep and not discard:
        assert want[1] == BATCH[1] + [("k", "v"), ("k", "w"), ("k", "v")]
        assert want[4][1:] == [("no_separator_key_0", "nosep"), ("empty_key_0", "empty"), ("no_separator_key_1", "quoted nosep"), ("x", "\"unterminated "),
                               ("empty_key_1", "2"), ("z", "3")]  # (one byte behind the delimiter, one more skipped: the y is lost, as in the Go)
        assert (kvsplit.LC_KV_ALARM_NO_SEPARATOR, b'can not find separator in "quoted nosep"') in alarms
        assert (kvsplit.LC_KV_ALARM_EMPTY_KEY, b"the key of pair with value (empty) is empty") in alarms
        assert (kvsplit.LC_KV_ALARM_NO_SOURCE_KEY, b"can not find key: content") in alarms


def test_alarm_switches_silence_their_sites():
    config = dict(LOGFMT, SourceKey="content", ErrIfSourceKeyNotFound=False, ErrIfSeparatorNotFound=False, ErrIfKeyIsEmpty=False)
    p = kp.processor(**config)
    want, alarms = kp.model_logs(config, BATCH)
    assert p.process_logs(BATCH) == want and alarms == [] and p.collect_alarms() == []
    assert p.counters()["no_separator"] > 0 and p.counters()["empty_keys"] > 0 and p.counters()["no_source_key"] == 2


def test_reference_panic_values_leave_their_log_unchanged():
    values = ['a=""x ', 'a=""x y"" b=2', 'c=1 a=""x ', 'plain=1']
    assert [kv_model.split(Q2, v.encode())[0] for v in values] == ["panic", "ok", "panic", "ok"]
    for keep in (False, True):
        config = dict(Q2, SourceKey="content", KeepSource=keep)
        logs = [[("host", "h"), ("content", v)] for v in values]
        p = kp.processor(**config)
        want, alarms = kp.model_logs(config, logs)
        got = p.process_logs(logs)
        assert got == want and got[0] == logs[0] and got[2] == logs[2] and got[1] != logs[1]
        heard = p.collect_alarms()
        assert [k for k, _ in heard] == [k for k, _ in alarms] and [k for k, _ in heard].count(kvsplit.LC_KV_ALARM_REF_PANIC) == 2
        assert p.counters()["ref_panic"] == 2 and p.counters()["values"] == 4


@pytest.mark.parametrize("W", [1, 2, 16])
def test_mop_up_is_one_trip_at_the_largest_count(W):
    L = kp.double()
    counts = [0, 1, W - 1, W, W + 1, 3 * W + 2, 40, 2]
    logs = [[("content", " ".join("k%d=v%d" % (i, i) for i in range(n)))] for n in counts]
    true_counts = [max(n, 1) for n in counts]  # (the empty value is one empty pair)
    config = dict(LOGFMT, SourceKey="content")
    p = kp.processor(**config)
    p.set_first_trip_pairs(W)
    before = kp.trip_stats(L)
    assert p.process_logs(logs) == kp.model_logs(config, logs)[0]
    after = kp.trip_stats(L)
    wide = sum(1 for n in true_counts if n > W)
    assert after["trips"] - before["trips"] == 2 and after["values"] - before["values"] == len(logs) + wide and after["last_W"] == max(true_counts)
    assert p.counters()["mop_up"] == wide and p.counters()["pairs"] == sum(true_counts)
    # nothing above W: one trip
    small = kp.processor(**config)
    small.set_first_trip_pairs(64)
    small.process_logs(logs)
    assert kp.trip_stats(L)["trips"] - after["trips"] == 1 and small.counters()["mop_up"] == 0
    # no source value at all: no trip
    assert small.process_logs([[("x", "y")], []]) == [[("x", "y")], []] and kp.trip_stats(L)["trips"] - after["trips"] == 1


def test_failed_trip_leaves_every_log_unchanged_and_is_reported():
    L = kp.double()
    p = kp.processor(**dict(LOGFMT, SourceKey="content", KeepSource=False))
    logs = [[("content", "a=1 b=2")], [("other", "x")]]
    L.kd_fail_next_trips(1)
    with pytest.raises(RuntimeError):
        p.process_logs(logs)
    c = p.counters()
    assert c["failed_trips"] == 1 and c["values"] == c["pairs"] == c["no_source_key"] == 0
    assert [k for k, _ in p.collect_alarms()] == [kvsplit.LC_KV_ALARM_TRIP_FAILED]
    assert p.process_logs(logs) == [[("a", "1"), ("b", "2")], [("other", "x")]] and p.counters()["failed_trips"] == 1


def test_init_defaults_and_needle_bounds():
    unit, _ = kc.load_fixtures()
    for e in unit["cases"]:  # the reference's own configurations, through Init's defaults
        p = kp.processor(**e["config"])
        source = e["config"]["SourceKey"]
        got = p.process_logs([[(source, e["value"])]])[0]
        assert got[0] == (source, e["value"]) and [list(kv) for kv in got[1:]] == e["pairs"], e["case"]
    # empty strings are replaced (Init :56-67), newKeyValueSplitter's switches are on
    p = kp.processor(Delimiter="", Separator="", EmptyKeyPrefix="", NoSeparatorKeyPrefix="")
    assert p.process_logs([[("c", "a:1\t:2\tlone")]]) == [[("c", "a:1\t:2\tlone"), ("a", "1"), ("empty_key_0", "2"), ("no_separator_key_0", "lone")]]
    assert [k for k, _ in p.collect_alarms()] == [kvsplit.LC_KV_ALARM_EMPTY_KEY, kvsplit.LC_KV_ALARM_NO_SEPARATOR]
    for field in ("Delimiter", "Separator", "Quote"):
        ok = kp.processor(**{field: "x" * 32})
        assert ok.process_logs([[("c", "v")]])[0][0] == ("c", "v")
        with pytest.raises(kvsplit.KvSplitInitError, match=field + " is 33 bytes long"):
            kp.processor(**{field: "x" * 33})
    import ctypes
    handle, err = ctypes.c_void_p(), ctypes.create_string_buffer(256)
    assert kp.double().lc_kvsplit_create(b"[1, 2]", 6, ctypes.byref(handle), err, 256) != 0 and not handle.value and b"JSON object" in err.value
