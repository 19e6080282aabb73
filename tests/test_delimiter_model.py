"""tests/helpers/delimiter_model.py against the reference's own output (tests/golden/delimiter_reference_outputs.json, written by
tests/golden/gen_delimiter_vectors.py from processor_parse_delimiter_native compiled from source): every case, nothing left out.
Only behind this test may the model stand in for the reference on a GPU box."""
import json
import os

from helpers.delimiter_model import BLANK, FAIL, OK, Engine, Processor


def _cases(golden_dir):
    with open(os.path.join(golden_dir, "delimiter_reference_outputs.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


def run_model(case):
    p = Processor(case["config"])
    events = [[[b"content", ln.encode("latin-1")]] for ln in case["lines"]] + [[[b"other", b"x"]]]
    out = p.process(events)
    return ([[[k.decode("latin-1"), v.decode("latin-1")] for k, v in ev] for ev in out], p.counters, [a.decode("latin-1") for a in p.alarms])


def test_the_model_equals_the_reference_s_output_on_every_case(golden_dir):
    cases = _cases(golden_dir)
    assert len(cases) >= 100
    seen = set()
    for k, case in enumerate(cases):
        out, counters, alarms = run_model(case)
        assert out == case["out"], (k, case["config"])
        assert counters == case["counters"], (k, case["config"])
        assert alarms == case["alarms"], (k, case["config"])
        seen.add((case["config"]["Separator"], case["config"].get("Quote"), case["config"]["OverflowedFieldsTreatment"]))
    # the fixture covers what it claims: five separators, quotes equal to the separator, the three modes
    assert {s for s, _, _ in seen} == {",", "|", "\t", "\\t", "||", "@@@@"}
    assert {m for _, _, m in seen} == {"extend", "keep", "discard"}
    assert any(s == q for s, q, _ in seen)


def test_the_model_equals_the_unit_test_s_expectations_on_every_case(golden_dir):
    with open(os.path.join(golden_dir, "delimiter_unittest_vectors.json"), encoding="utf-8") as f:
        doc = json.load(f)
    assert len(doc["cases"]) >= 30
    for case in doc["cases"]:
        p = Processor(case["config"])
        events = [[[k.encode("latin-1"), v.encode("latin-1")] for k, v in ev["contents"]] for ev in case["in"].get("events", [])]
        out = p.process(events)
        got = [{k.decode("latin-1"): v.decode("latin-1") for k, v in ev} for ev in out]
        assert got == [ev.get("contents", {}) for ev in case["expect"].get("events", [])], case["name"]
        assert p.counters == case["reference_counters"], case["name"]
        assert [a.decode("latin-1") for a in p.alarms] == case["reference_alarms"], case["name"]
        for member, index in (("mDiscardedEventsTotal", 0), ("mOutFailedEventsTotal", 1)):
            if member in case["asserted"]:
                assert p.counters[index] == case["asserted"][member], case["name"]


def test_the_engine_level_of_the_model_on_hand_made_lines():
    e = Engine(b",", b'"', "extend", 3)
    assert e.split_line(b"") == (BLANK, 0, [])
    assert e.split_line(b"  \r ") == (BLANK, 0, [])
    assert e.split_line(b' "a,b",c ') == (OK, 2, [(2, 5, False), (7, 8, False)])
    assert e.split_line(b'"a""b",') == (OK, 2, [(1, 5, True), (7, 7, False)])
    assert e.value(b'"a""b",', (1, 5, True)) == b'a"b'
    assert e.split_line(b'a"b')[0] == FAIL and e.split_line(b'"ab')[0] == FAIL and e.split_line(b'"a"b')[0] == FAIL
    k = Engine(b"||", b'"', "keep", 2)
    assert k.split_line(b"a||b||c||d") == (OK, 3, [(0, 1, False), (3, 4, False), (4, 10, False)])
    assert k.split_line(b"|") == (OK, 1, [(0, 1, False)])
    assert Engine(b"||", b'"', "extend", 2).split_line(b"a|||b||") == (OK, 3, [(0, 1, False), (3, 5, False), (7, 7, False)])
