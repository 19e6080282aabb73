"""processor_parse_json_gpu on a machine without a GPU: the product's PER-LINE ROUTINE (jsonWalkLine of csrc/json_vm.hpp, what
json_walk_kernel runs per lane, compiled for the host: tests/native/json_host_check.cpp) against tests/helpers/json_model.py record for
record, and the product's HOST code (csrc/processor_parse_json_gpu.cpp: Init, the gather, the mop-up rule, the stitch, the source-key
rules, counters, alarms) with tests/native/json_double.cpp standing in for the device trip."""
import ctypes
import itertools
import json

import numpy as np
import pytest

from helpers import json_cases as jc
from helpers import json_model as jm
from helpers import plugin_double
from helpers.native_build import load_double


def _double():
    vp, cp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    return load_double("json_double", ("json_double.cpp", "json_host_check.cpp", "processor_parse_json_gpu.cpp", "processor_parse_regex_gpu.cpp",
                                       "event_model.cpp"), {
        "jd_process_json": (vp, [vp, cp, ctypes.POINTER(i32), cp, sz]),
        "jd_free": (i32, [vp]),
        "jd_walk_stats": (i32, [ctypes.POINTER(ctypes.c_uint64)]),
        "jd_fail_next_trips": (i32, [i32]),
        "jd_fail_after": (i32, [i32]),
        "jh_walk_line": (None, [cp, u32, u32, u32, vp, vp, vp, vp, vp, ctypes.POINTER(i32)]),
        "jh_walk_line_first": (None, [cp, u32, u32, u32, vp, vp, vp, vp, vp]),
        "jh_walk_batch": (None, [vp, vp, u32, u32, vp, vp, vp, vp, vp]),
    })


def walk_line(line, head, W, first_only=False):
    """-> (status, nmembers, errpos, records MEMBER[W], shadow u8[len], went_deep)"""
    L = _double()
    status, nm, err = ctypes.c_uint8(9), ctypes.c_uint32(99), ctypes.c_uint32(99)
    rec = np.zeros(max(W, 1), jc.MEMBER)
    shadow = np.full(len(line) + 1, 0xEE, np.uint8)
    deep = ctypes.c_int(0)
    args = (bytes(line), len(line), head, W, ctypes.byref(status), ctypes.byref(nm), ctypes.byref(err), rec.ctypes.data, shadow.ctypes.data)
    if first_only:
        L.jh_walk_line_first(*args)
    else:
        L.jh_walk_line(*args, ctypes.byref(deep))
    return status.value, nm.value, err.value, rec, shadow, bool(deep.value)


def test_the_per_line_routine_on_the_contract_vectors_at_every_alignment():
    for case in jc.contract_cases():
        line = jc.expand(case["line"])
        for head in range(16):
            st, nm, err, rec, shadow, deep = walk_line(line, head, 8)
            assert st == jc.STATUS_NAMES[case["status"]], (case["name"], head, err)
            assert jc.same_as_model(line, st, nm, err, rec, shadow, 8) is None, (case["name"], head)
            if case["status"] == "fail":
                assert err == case["errpos"], (case["name"], head)
            assert deep == ("depth 65" in case["name"] or "depth 102" in case["name"]), case["name"]


def test_the_first_walk_leaves_a_line_deeper_than_64_levels_as_deep():
    for case in jc.contract_cases():
        line = jc.expand(case["line"])
        st, nm, err, _, _, _ = walk_line(line, 3, 4, first_only=True)
        if jm.max_depth_reached(line) > 64 and "left open" not in case["name"]:
            assert (st, nm) == (3, 0), case["name"]
        elif "depth" in case["name"]:
            assert st in (jm.OK, 3), case["name"]


def test_the_per_line_routine_against_the_model_on_the_generated_set():
    """the documents of tests/test_json_model.py (valid ones and one-byte mutations), line i at alignment 7 i"""
    L = _double()
    docs = jc.generated_set(20261017, 21000)
    data, off = jc.pack(docs)
    n, W = len(docs), 8
    status = np.zeros(n, np.uint8)
    nm = np.zeros(n, np.uint32)
    err = np.zeros(n, np.uint32)
    rec = np.zeros((n, W), jc.MEMBER)
    shadow = np.full(len(data), 0xEE, np.uint8)
    L.jh_walk_batch(data.ctypes.data, off.ctypes.data, n, W, status.ctypes.data, nm.ctypes.data, err.ctypes.data, rec.ctypes.data, shadow.ctypes.data)
    for i, doc in enumerate(docs):
        why = jc.same_as_model(doc, status[i], nm[i], err[i], rec[i], shadow[off[i]:off[i + 1]], W)
        assert why is None, (i, doc, why)
    assert int((status == 1).sum()) > 5000 and int((status == 0).sum()) > 5000


def test_only_the_bytes_of_escaped_texts_are_written_to_the_shadow():
    line = b'{"plain":"no escapes here","k\\u0041":"v\\n","nested":["\\t"],"z":"\\\\"}'
    st, nm, err, rec, shadow, _ = walk_line(line, 5, 8)
    assert (st, nm) == (jm.OK, 4)
    written = {i for i in range(len(line)) if shadow[i] != 0xEE}
    _, members, _ = jm.walk(line)
    allowed = set()
    for m in members:
        if m.key_text is not None:
            allowed |= set(range(m.kb, m.ke))
        if m.val_text is not None:
            allowed |= set(range(m.vb, m.ve))
    assert written and written <= allowed


class Product(plugin_double.Product):
    PREFIX, FREE, ALARM_TEXT = "lc_json_processor", "jd_free", None

    def __init__(self, config, first_trip_members=0):
        plugin_double.Product.__init__(self, config, _double())
        if first_trip_members:
            self.L.lc_json_processor_set_first_trip_members(self.h, first_trip_members)
        self.rc = 0

    def process_group(self, group):
        """fixture group (latin-1 text: one character per byte) -> the events that are left, contents as dicts of bytes"""
        err = ctypes.create_string_buffer(512)
        rc = ctypes.c_int(0)
        p = self.L.jd_process_json(self.h, json.dumps(group, ensure_ascii=False).encode("latin-1"), ctypes.byref(rc), err, 512)
        assert p, err.value
        self.rc = rc.value
        try:
            d = json.loads(ctypes.string_at(p).decode("latin-1"))
        finally:
            self.L.jd_free(p)
        return (d or {}).get("events", [])

    def process_contents(self, events):
        """events: dicts bytes -> bytes -> the same for the events that are left"""
        group = {"events": [{"contents": {k.decode("latin-1"): v.decode("latin-1") for k, v in ev.items()}, "timestamp": 1, "type": 1}
                            for ev in events]}
        return [{k.encode("latin-1"): v.encode("latin-1") for k, v in ev.get("contents", {}).items()} for ev in self.process_group(group)]

    def counters(self):
        return self.counter_values()


def _model_run(config, events):
    model = jm.Processor(config)
    out = [e for e in (model.process_event(ev) for ev in events) if e is not None]
    c = model.counters
    return out, [c["discarded"], c["out_failed"], c["out_key_not_found"], c["out_successful"]], model.alarms


def test_the_processor_on_the_contract_vectors_gives_the_literal_members():
    cases = jc.contract_cases()
    for first_trip in (0, 1):
        p = Product({"SourceKey": "content"}, first_trip_members=first_trip)
        events = [{b"content": jc.expand(c["line"]), b"other": b"o"} for c in cases]
        got = p.process_contents(events)
        assert len(got) == len(cases)
        n_fail = 0
        for case, ev in zip(cases, got):
            if case["status"] == "ok":
                want = {b"other": b"o"}
                for k, _, v in case["members"]:
                    want[jc.expand(k)] = jc.expand(v)
                assert ev == want, case["name"]
            else:
                assert ev == {b"other": b"o"}, case["name"]
                n_fail += case["status"] == "fail"
        c = p.counters()
        assert c[:6] == [0, n_fail, 0, len(cases), len(cases), len(cases)] and c[11] == 0
        assert [(k, m) for k, m in p.alarms] == [(0, b"parse json fail:" + jc.expand(c["line"])) for c in cases if c["status"] == "fail"]


POLICIES = [dict(KeepingSourceWhenParseFail=f, KeepingSourceWhenParseSucceed=s, CopingRawLog=r, **({"RenamedSourceKey": "raw"} if ren else {}))
            for f, s, r, ren in [(False, False, False, False), (True, False, True, False), (False, True, False, True), (True, True, True, True)]]


@pytest.mark.parametrize("policy", range(len(POLICIES)))
def test_the_policy_matrix_ok_fail_empty_and_key_missing(policy):
    config = dict(POLICIES[policy], SourceKey="content")
    events = [{b"content": b'{"a":"1","content":"inner"}', b"keep": b"k"},      # ok, and a member named like the source key
              {b"content": b'{"a":-0,"b":1.5,"c":null,"d":[1, 2],"a":"again"}'},   # ok, a repeated key
              {b"content": b'{"a":1'},                                           # fail, nothing else in the event
              {b"content": b'{"a":tru}', b"keep": b"k"},                         # fail
              {b"content": b""},                                                 # empty, nothing else
              {b"content": b"", b"keep": b"k"},                                  # empty
              {b"other": b"x"},                                                  # key missing
              {b"content": b'{"raw":"mine","__raw_log__":"mine too"}'}]           # members named like the keys the policy adds
    p = Product(config)
    got = p.process_contents(events)
    want, counters, alarms = _model_run(config, events)
    assert got == want
    assert p.counters()[:4] == counters and p.counters()[4] == len(events) and p.counters()[5] == len(want)
    assert [m for _, m in p.alarms] == alarms and all(k == 0 for k, _ in p.alarms)
    # literal spot checks, by hand from ProcessEvent :122-144
    if policy == 0:
        assert got[0] == {b"keep": b"k", b"a": b"1", b"content": b"inner"}
        assert got[1] == {b"a": b"again", b"b": b"1.500000", b"c": b"", b"d": b"[1, 2]"}
        assert len(got) == 6 and counters == [2, 2, 1, 5]          # the two events left without a content are erased; a missing key ends :117
        assert alarms == [b'parse json fail:{"a":1', b'parse json fail:{"a":tru}']
    if policy == 1:
        assert {b"content": b'{"a":1', b"__raw_log__": b'{"a":1'} in got and {b"content": b"", b"__raw_log__": b""} in got
        assert len(got) == 8 and counters == [0, 2, 1, 7]
    if policy == 3:
        assert got[0] == {b"keep": b"k", b"a": b"1", b"content": b"inner", b"raw": b'{"a":"1","content":"inner"}'}
        assert got[7] == {b"raw": b"mine", b"__raw_log__": b"mine too"}


def test_the_mop_up_rule_a_small_first_trip_gives_the_same_events_as_the_default():
    L = _double()
    stats = (ctypes.c_uint64 * 2)()
    docs = [d for d in jc.generated_set(7, 1500)]
    wide = b'{' + b",".join(b'"k%d":"\\u00e9%d"' % (i, i) for i in range(40)) + b'}'
    events = [{b"content": d} for d in docs] + [{b"content": wide}]
    config = {"SourceKey": "content", "KeepingSourceWhenParseFail": True}
    want, counters, alarms = _model_run(config, events)
    assert want[-1][b"k39"] == b"\xc3\xa939"
    for first in (1, 2, 5, 0, 64):
        p = Product(config, first_trip_members=first)
        L.jd_walk_stats(stats)
        calls0, lines0 = stats[0], stats[1]
        got = p.process_contents(events)
        L.jd_walk_stats(stats)
        assert stats[0] - calls0 == (1 if first == 64 else 2)          # one trip, and ONE mop-up
        if first == 0:
            assert stats[1] - lines0 == len(events) + sum(1 for d in docs + [wide] if jm.walk(d)[0] == jm.OK and len(jm.walk(d)[1]) > 32)
        assert got == want, first
        assert p.counters()[:4] == counters and [m for _, m in p.alarms] == alarms


def test_a_failed_device_trip_leaves_the_group_untouched_and_is_counted():
    L = _double()
    p = Product({"SourceKey": "content"})
    events = [{b"content": b'{"a":1}'}, {b"content": b"x"}, {b"other": b"y"}]
    L.jd_fail_next_trips(1)
    got = p.process_contents(events)
    assert p.rc != 0 and got == events
    c = p.counters()
    assert c[11] == 2 and c[2] == 1 and c[3] == 0 and c[0] == 0
    assert [k for k, _ in p.alarms] == [3]
    assert p.process_contents(events) == [{b"a": b"1"}, {b"other": b"y"}] and p.rc == 0


RAW = {"content": "no log event", "timestamp": 1, "type": 4}      # (the fixture's one event type besides the log event)


def _log(contents):
    return {"contents": contents, "timestamp": 1, "type": 1}


def test_a_failed_first_trip_is_reported_counted_and_a_healthy_call_behind_it_parses(capfd):
    """one parsable event, one without the key, one that is no log event; counters as [discarded, out_failed, out_key_not_found,
    out_successful, in_events, out_events]: the gather's out_failed (the raw event) and key_not_found are added behind a failed trip"""
    L = _double()
    events = [_log({"content": '{"a":1}'}), _log({"other": "y"}), RAW]
    text = "GPU JSON walk failed (rc=4: the JSON double has no device); 1 events left unparsed"
    p = Product({"SourceKey": "content"})
    L.jd_fail_next_trips(1)
    assert p.process_group({"events": events}) == events and p.rc == 4
    assert p.alarms == [(3, text.encode())]
    c = p.counters()
    assert c[:6] == [0, 1, 1, 0, 3, 3] and c[11] == 1
    # no sink: exactly one line on stderr
    L.lc_json_processor_set_alarm_sink(p.h, None, None)
    capfd.readouterr()
    L.jd_fail_next_trips(1)
    assert p.process_group({"events": events}) == events and p.rc == 4
    assert capfd.readouterr().err == "[processor_parse_json_gpu] " + text + "\n"
    assert len(p.alarms) == 1 and p.counters()[11] == 2
    assert p.process_group({"events": events}) == [_log({"a": "1"}), _log({"other": "y"}), RAW] and p.rc == 0
    c = p.counters()
    assert c[:6] == [0, 3, 3, 1, 9, 9] and c[11] == 2


def test_a_failed_second_trip_leaves_the_group_untouched_and_counts_the_first_trip_s_lines():
    L = _double()
    stats = (ctypes.c_uint64 * 2)()
    events = [_log({"content": '{"a":1,"b":"\\n"}'}), _log({"content": '{"a":1}'}), _log({"other": "y"})]
    p = Product({"SourceKey": "content"}, first_trip_members=1)
    L.jd_walk_stats(stats)
    calls0 = stats[0]
    L.jd_fail_after(1)
    assert p.process_group({"events": events}) == events and p.rc == 4
    L.jd_walk_stats(stats)
    assert stats[0] - calls0 == 1          # the first trip went through; the mop-up is the call that failed
    assert p.alarms == [(3, b"GPU JSON walk failed (rc=4: the JSON double has no device); 2 events left unparsed")]
    c = p.counters()
    assert c[:6] == [0, 0, 1, 0, 3, 3] and c[11] == 2
    assert p.process_group({"events": events}) == [_log({"a": "1", "b": "\n"}), _log({"a": "1"}), _log({"other": "y"})] and p.rc == 0
    assert p.counters()[:4] == [0, 0, 2, 2] and p.counters()[11] == 2


def test_init_answers_false_with_the_reference_s_messages():
    for config, message in (({}, "mandatory param SourceKey is missing"), ({"SourceKey": 1}, "param SourceKey is not of type string"),
                            ({"SourceKey": ""}, "mandatory string param SourceKey is empty")):
        with pytest.raises(ValueError) as e:
            Product(config)
        assert str(e.value) == message
    p = Product({"SourceKey": "content", "KeepingSourceWhenParseFail": "yes", "CopingRawLog": 1})
    assert p.warnings() == ["param KeepingSourceWhenParseFail is not of type bool", "param CopingRawLog is not of type bool"]


def test_the_cases_of_the_reference_s_unit_test_through_the_product_s_host_code():
    doc = jc.unittest_doc()
    assert len({c["name"].split("/")[0] for c in doc["cases"]} | {c["name"] for c in doc["init_only"]}) == 20
    names = {"discarded_events_total": 0, "out_failed_events_total": 1, "in_events_total": 4, "out_events_total": 5}
    for case in doc["cases"]:
        for first_trip in (0, 1):
            p = Product(case["config"], first_trip_members=first_trip)
            events = [{k.encode("latin-1"): v.encode("latin-1") for k, v in ev.items()} for ev in case["in"]]
            want = [{k.encode("latin-1"): v.encode("latin-1") for k, v in ev.items()} for ev in case["expect"]]
            got = p.process_contents(events)
            assert got == want, case["name"]
            for name, value in case["counters"].items():
                assert p.counters()[names[name]] == value, (case["name"], name)
            for probe in case.get("probe_substrings", []):
                assert any(probe.encode() in k or probe.encode() in v for ev in got for k, v in ev.items()), (case["name"], probe)
    for case in doc["init_only"]:
        Product(case["config"])
    p = Product({"SourceKey": "content"})
    assert p.process_contents([{b"content": s.encode("latin-1")} for s in doc["invalid_formats"]]) == []
    assert p.counters()[:4] == [7, 7, 0, 0] and len(p.alarms) == 7
