"""processor_parse_delimiter_gpu on a machine without a GPU: the product's HOST code (csrc/processor_parse_delimiter_gpu.cpp: Init, the
gather, the mop-up rule, the stitch, the source-key rules, counters, alarms) and the product's PER-LINE ROUTINE (delimSplitLine of
csrc/delim_vm.hpp, what delim_split_kernel runs per lane, compiled for the host) over every case of
tests/golden/delimiter_reference_outputs.json -- the reference's own output.  tests/native/delimiter_double.cpp stands in for the device
trip.  Events, contents, counters and alarm texts must equal the fixture's."""
import ctypes
import json
import os
import random

import pytest

from helpers import plugin_double
from helpers.delimiter_model import Engine
from helpers.native_build import load_double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _double():
    vp, cp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    return load_double("delimiter_double", ("delimiter_double.cpp", "processor_parse_delimiter_gpu.cpp", "processor_parse_regex_gpu.cpp", "event_model.cpp"), {
        "dd_process_json": (vp, [vp, cp, cp, sz]),
        "dd_process_json_rc": (vp, [vp, cp, ctypes.POINTER(i32), cp, sz]),
        "dd_fail_next_trips": (i32, [i32]),
        "dd_fail_after": (i32, [i32]),
        "dd_free": (i32, [vp]),
        "dd_split_line": (None, [vp, cp, u32, u32, u32, vp, vp, vp]),
        "dd_split_stats": (i32, [ctypes.POINTER(ctypes.c_uint64)]),
    })


class Product(plugin_double.Product):
    PREFIX, FREE = "lc_delimiter_processor", "dd_free"

    def __init__(self, config, first_trip_columns=0):
        plugin_double.Product.__init__(self, config, _double())
        if first_trip_columns:
            self.L.lc_delimiter_processor_set_first_trip_columns(self.h, first_trip_columns)

    def process_group(self, group):
        """fixture group in -> the events that are left, each a dict with its contents as an ordered list of pairs"""
        err = ctypes.create_string_buffer(512)
        p = self.L.dd_process_json(self.h, json.dumps(group, ensure_ascii=False).encode("latin-1"), err, 512)
        assert p, err.value
        try:
            d = json.loads(ctypes.string_at(p).decode("latin-1"), object_pairs_hook=list)
        finally:
            self.L.dd_free(p)
        out = []
        for ev in dict(d or []).get("events", []):
            ev = dict(ev)
            ev["contents"] = [list(kv) for kv in ev.get("contents", [])]
            out.append(ev)
        return out

    def process_group_rc(self, group):
        """fixture group in -> (the processor's return code, the group's events as ToJsonString prints them)"""
        err = ctypes.create_string_buffer(512)
        rc = ctypes.c_int(0)
        p = self.L.dd_process_json_rc(self.h, json.dumps(group, ensure_ascii=False).encode("latin-1"), ctypes.byref(rc), err, 512)
        assert p, err.value
        try:
            return rc.value, (json.loads(ctypes.string_at(p).decode("latin-1")) or {}).get("events", [])
        finally:
            self.L.dd_free(p)

    def process_lines(self, lines):
        events = [{"contents": [["content", ln]], "timestamp": 1, "type": 1} for ln in lines]
        events.append({"contents": [["other", "x"]], "timestamp": 1, "type": 1})
        return [ev["contents"] for ev in self.process_group({"events": events})]

    def counters(self):
        return self.counter_values()


def _cases(golden_dir):
    with open(os.path.join(golden_dir, "delimiter_reference_outputs.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


def test_the_product_s_host_code_and_per_line_routine_equal_the_reference_on_every_case(golden_dir):
    for k, case in enumerate(_cases(golden_dir)):
        p = Product(case["config"])
        assert p.process_lines(case["lines"]) == case["out"], (k, case["config"])
        c = p.counters()
        assert c[:4] == case["counters"], (k, case["config"])
        assert c[4] == len(case["lines"]) + 1 and c[5] == len(case["out"]) and c[11] == 0
        assert [m for _, m in p.alarms] == case["alarms"], (k, case["config"])
        assert all(kind == (2 if m.startswith("keys count") else 0) for kind, m in p.alarms)


def test_the_mop_up_rule_a_small_first_trip_gives_the_same_events_as_a_huge_one(golden_dir):
    """a group whose widest line has more columns than the first trip kept: the lines that did not fit take ONE second trip"""
    L = _double()
    stats = (ctypes.c_uint64 * 2)()
    for k, case in enumerate(_cases(golden_dir)):
        widest = max(len(ln) for ln in case["lines"]) + 2
        for w in (1, 2, 4):
            small = Product(case["config"], first_trip_columns=w)
            huge = Product(case["config"], first_trip_columns=widest)
            L.dd_split_stats(stats)
            calls0 = stats[0]
            got = small.process_lines(case["lines"])
            L.dd_split_stats(stats)
            assert stats[0] - calls0 <= 2                      # one trip, and at most one mop-up
            assert got == huge.process_lines(case["lines"]) == case["out"], (k, w, case["config"])
            assert small.counters()[:4] == case["counters"] and [m for _, m in small.alarms] == case["alarms"]


RAW = {"content": "no log event", "timestamp": 1, "type": 4}      # (the fixture's one event type besides the log event)


def _log(contents):
    return {"contents": contents, "timestamp": 1, "type": 1}


def test_a_failed_first_trip_is_reported_counted_and_a_healthy_call_behind_it_parses(capfd):
    """one parsable event, one without the key, one that is no log event; counters as [discarded, out_failed, out_key_not_found,
    out_successful, in_events, out_events]: the gather's out_failed (the raw event) and key_not_found are added behind a failed trip"""
    L = _double()
    events = [_log({"content": "x,y"}), _log({"other": "y"}), RAW]
    text = "GPU split failed (rc=4: the delimiter double has no device); 1 events left unparsed"
    p = Product({"SourceKey": "content", "Separator": ",", "Keys": ["a", "b"]})
    L.dd_fail_next_trips(1)
    assert p.process_group_rc({"events": events}) == (4, events)
    assert p.alarms == [(3, text)]
    c = p.counters()
    assert c[:6] == [0, 1, 1, 0, 3, 3] and c[11] == 1
    # no sink: exactly one line on stderr
    L.lc_delimiter_processor_set_alarm_sink(p.h, None, None)
    capfd.readouterr()
    L.dd_fail_next_trips(1)
    assert p.process_group_rc({"events": events}) == (4, events)
    assert capfd.readouterr().err == "[processor_parse_delimiter_gpu] " + text + "\n"
    assert len(p.alarms) == 1 and p.counters()[11] == 2
    assert p.process_group_rc({"events": events}) == (0, [_log({"a": "x", "b": "y"}), _log({"other": "y"}), RAW])
    c = p.counters()
    assert c[:6] == [0, 3, 3, 1, 9, 9] and c[11] == 2


def test_a_failed_second_trip_leaves_the_group_untouched_and_counts_the_first_trip_s_lines():
    L = _double()
    stats = (ctypes.c_uint64 * 2)()
    events = [_log({"content": "x,y,z"}), _log({"content": "x"}), _log({"other": "y"})]
    p = Product({"SourceKey": "content", "Separator": ",", "Keys": ["a", "b"], "AllowingShortenedFields": True}, first_trip_columns=1)
    L.dd_split_stats(stats)
    calls0 = stats[0]
    L.dd_fail_after(1)
    assert p.process_group_rc({"events": events}) == (4, events)
    L.dd_split_stats(stats)
    assert stats[0] - calls0 == 1          # the first trip went through; the mop-up is the call that failed
    assert p.alarms == [(3, "GPU split failed (rc=4: the delimiter double has no device); 2 events left unparsed")]
    c = p.counters()
    assert c[:6] == [0, 0, 1, 0, 3, 3] and c[11] == 2
    assert p.process_group_rc({"events": events}) == (0, [_log({"a": "x", "b": "y", "__column2__": "z"}), _log({"a": "x"}), _log({"other": "y"})])
    assert p.counters()[:4] == [0, 0, 2, 2] and p.counters()[11] == 2


def _unit(golden_dir):
    with open(os.path.join(golden_dir, "delimiter_unittest_vectors.json"), encoding="utf-8") as f:
        return json.load(f)


def same_events(got, expect):
    """the unit test compares ToJsonString texts, whose contents are an object: keys and values, timestamps and type"""
    def norm(ev):
        return (dict(ev.get("contents", [])), ev.get("timestamp"), ev.get("timestampNanosecond", 0), ev.get("type"))
    return [norm(e) for e in got] == [norm(e) for e in expect.get("events", [])]


COUNTER_MEMBERS = {"mDiscardedEventsTotal": 0, "mOutFailedEventsTotal": 1, "mOutKeyNotFoundEventsTotal": 2, "mOutSuccessfulEventsTotal": 3,
                   "mInEventsTotal": 4, "mOutEventsTotal": 5}


def test_the_cases_of_the_reference_s_unit_test_through_the_product_s_host_code(golden_dir):
    doc = _unit(golden_dir)
    assert len({c["name"].split("/")[0] for c in doc["cases"]} | {c["name"] for c in doc["init_only"]}) == 14
    for case in doc["cases"]:
        assert case["reference_agrees"], case["name"]      # (the reference's own output equals its unit test's expectation)
        for first_trip in (0, 1):
            p = Product(case["config"], first_trip_columns=first_trip)
            got = p.process_group(case["in"])
            assert same_events(got, case["expect"]), (case["name"], got)
            c = p.counters()
            for member, value in case["asserted"].items():
                assert c[COUNTER_MEMBERS[member]] == value, (case["name"], member)
            assert c[:4] == case["reference_counters"], case["name"]
            assert [m for _, m in p.alarms] == case["reference_alarms"], case["name"]
    for case in doc["init_only"]:
        Product(case["config"])


def test_init_successes_failures_and_warnings_are_the_reference_s(golden_dir):
    """the fixture holds what the reference's own Init answered for each config: accepted or not, and the alarm texts it raised
    ("<message>: abort, module: ..." for a refusal, "<message>: use default value instead ..." / "<message>: ignore param ..." for
    a warning); the product refuses the same configs with the same message and raises the same warnings in the same order"""
    init = _unit(golden_dir)["init"]
    assert sum(i["ok"] for i in init) >= 8 and sum(not i["ok"] for i in init) >= 10
    for i in init:
        messages = [a.split(": ")[0] for a in i["alarms"]]
        if i["ok"]:
            assert Product(i["config"]).warnings() == messages, i["config"]
        else:
            with pytest.raises(ValueError) as e:
                Product(i["config"])
            assert [str(e.value)] == messages[-1:], i["config"]


def test_the_per_line_routine_against_the_model_on_random_lines_at_every_alignment():
    """delimSplitLine through HostLineSource (junk outside the line) at all 16 positions of a line inside its 16-byte unit"""
    L = _double()
    rng = random.Random(20261016)
    checked = 0
    for sep, quote, mode, nk in ((b",", b'"', "extend", 3), (b"|", b"'", "keep", 2), (b"\t", b"\t", "discard", 2), (b"||", b'"', "keep", 3),
                                 (b"@@@@", b'"', "extend", 2), (b",", b'"', "discard", 1)):
        h = ctypes.c_void_p()
        assert L.lc_delim_create(sep, len(sep), quote[0], {"extend": 0, "keep": 1, "discard": 2}[mode], nk, ctypes.byref(h)) == 0
        model = Engine(sep, quote, mode, nk)
        alphabet = [b"a", b"bc", b" ", sep, sep, quote, b"\r", sep[:1], quote + quote]
        W = 6
        for trial in range(1500):
            n = rng.choice([0, 1, 2, 5, 15, 16, 17, 40, 63, 64, 65, 130, 300])
            line = b"".join(rng.choice(alphabet) for _ in range(n))[: max(n, 0) * 2]
            if trial % 5 == 0:
                line = rng.choice([b"", b"  "]) + sep.join(quote + b"f" * rng.randint(0, 9) + quote if rng.random() < 0.3 else b"g" * rng.randint(0, 9)
                                                          for _ in range(rng.randint(1, 12))) + rng.choice([b"", b" \r", b"\r"])
            want = model.split_line(line)
            status = ctypes.c_uint8(9)
            ncols = ctypes.c_uint32(99)
            spans = (ctypes.c_int32 * (2 * W))(*([-7] * (2 * W)))
            L.dd_split_line(h, line, len(line), trial, W, ctypes.byref(status), ctypes.byref(ncols), spans)
            assert (status.value, ncols.value) == want[:2], (sep, quote, mode, line)
            for c, (b, e, doubled) in enumerate(want[2][:W]):
                assert (spans[2 * c] & 0x7FFFFFFF, spans[2 * c + 1], spans[2 * c] < 0) == (b, e, doubled), (sep, quote, mode, line, c)
            checked += 1
        L.lc_delim_destroy(h)
    assert checked == 9000
