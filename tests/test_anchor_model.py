"""tests/helpers/anchor_model.py (the reference's anchor.go restated on bytes) against the two fixture files: the reference's own unit
test read as data (anchor_unittest_vectors.json) and the model's recorded results (anchor_model_vectors.json).  Which tier pins what:
tests/golden/README_anchor.md."""
import pytest

from helpers import anchor_cases as ac
from helpers import anchor_model


def test_the_model_gives_the_unit_tests_stated_results():
    unit, _ = ac.load_fixtures()
    assert [e["case"] for e in unit["cases"]] == ["TestSourceKey", "TestNoKeyError", "TestNoAnchorErrorNoStart", "TestNoAnchorErrorNoStop"]
    first = unit["cases"][0]
    contents, alarms, pairs = anchor_model.process_log(first["run_config"], first["log"])
    assert [[k.decode(), v.decode()] for k, v in contents] == first["stated"] == [["time", "2017.09.12 20:55:36"], ["level", "info"]]
    assert alarms == [] and pairs == 2  # (KeepSource false: the source is gone, two fields came: 2 - 1 + 1)
    assert first["config"]["Anchors"][0]["Stop"] == "\\t" and len(first["config"]["Anchors"][0]["Stop"]) == 2  # backslash + t
    assert ac.rows_text(first["run_config"], first["value"]) == first["rows"] == "5 24 32 36"
    for e in unit["cases"][1:]:
        # as stated: the anchor is a json anchor (except TestNoKeyError's), which this project refuses ...
        if e["config"]["Anchors"][0].get("FieldType") == "json":
            with pytest.raises(anchor_model.Refused):
                anchor_model.init(e["config"])
        # ... as run: the same anchor as a string anchor; the outcome is decided at :175-189, before the type is looked at (:197)
        contents, alarms, _ = anchor_model.process_log(e["run_config"], e["log"])
        assert len(alarms) == 1 and alarms[0][0] == e["alarm_kind"], e["case"]
        assert e["stated_alarm"].encode() in alarms[0][1] and alarms[0][1].decode() == e["alarm"], e["case"]
        assert [[k.decode(), v.decode()] for k, v in contents] == e["contents"], e["case"]
    assert unit["cases"][1]["alarm"] == "anchor cannot find key:content\t" and unit["cases"][1]["contents"] == [["test_key", "test_value"]]
    assert unit["cases"][2]["contents"] == unit["cases"][3]["contents"] == []  # (the source removed, nothing appended)
    assert unit["cases"][2]["rows"] == "-1 -1" and unit["cases"][3]["rows"] == "-2 -1"


def test_the_model_gives_the_recorded_results():
    """the named cases entry by entry; a random set by its digests: the seeded values are the recorded ones, the model's answers are the
    recorded ones -- and where they are not, the two characters per value say which value it is"""
    _, model = ac.load_fixtures()
    assert len(model["named"]) >= 50
    for e in model["named"]:
        assert ac.rows_text(e["config"], e["value"].encode("utf-8")) == e["rows"], e["name"]
    for s in model["random"]:
        values = ac.set_values(s)
        got = ac.digest(values, [ac.rows_text(s["config"], v) for v in values])
        assert got["values_sha256"] == s["values_sha256"], s["name"]
        differing = [(i, values[i]) for i in range(s["n"]) if got["codes"][2 * i:2 * i + 2] != s["codes"][2 * i:2 * i + 2]]
        assert not differing and got["rows_sha256"] == s["rows_sha256"], (s["name"], differing[:5])
    assert len(ac.all_cases()) > 6000


def test_every_outcome_holds_three_percent_of_every_random_set():
    """field, no start and no stop of every anchor (but an outcome an empty needle rules out): the floor the generator asserted"""
    _, model = ac.load_fixtures()
    assert [s["name"] for s in model["random"]] == ["one_byte_needles", "overlapping_ab_needles", "three_and_four_byte_needles"]
    for s in model["random"]:
        values = ac.set_values(s)
        assert s["n"] == 2000 and len(values) == 2000 and max(len(v) for v in values) <= 24 and min(len(v) for v in values) == 0
        smallest = 1.0
        for anchor, shares in zip(s["config"]["Anchors"], ac.outcome_shares(s["config"], values)):
            assert anchor["Start"] and anchor["Stop"]  # (every outcome can be reached)
            for outcome, share in shares.items():
                assert share >= 0.03, (s["name"], anchor, outcome, share)
                smallest = min(smallest, share)
        assert round(smallest, 4) == s["smallest_share"]


def test_named_cases_say_what_their_names_say():
    _, model = ac.load_fixtures()
    rows = {e["name"]: e["rows"] for e in model["named"]}
    assert rows["start_empty"] == "0 2" and rows["stop_empty"] == "2 4" and rows["both_empty"] == "0 4" and rows["both_empty_empty_value"] == "0 0"
    assert rows["start_empty_empty_value"] == "-2 -1" and rows["stop_directly_behind_start"] == "2 2" and rows["stop_only_before_b"] == "-2 -1"
    assert rows["stop_overlaps_starts_tail"] == "-2 -1" and rows["stop_overlaps_starts_tail_then_real"] == "2 3"
    assert rows["aab_in_aaab"] == "4 4" and rows["aa_aa_on_aaa"] == "-2 -1" and rows["aa_aa_on_aaaa"] == "2 2"
    assert rows["needle_tail_in_the_next_value"] == "-1 -1" and rows["stop_tail_in_the_next_value"] == "-2 -1"
    assert rows["one_byte_stop_is_the_next_values_first_byte"] == "-2 -1" and rows["value_empty"] == "-1 -1"
    assert rows["value_is_start"] == "-2 -1" and rows["value_is_start_stop_empty"] == "3 3" and rows["value_is_start_plus_stop"] == "3 3"
    assert rows["two_anchors_same_start"] == "2 5 2 3" and rows["one_anchors_start_is_anothers_stop"] == "2 3 5 6"
    assert rows["three_outcomes_side_by_side"] == "2 3 -1 -1 -2 -1"
    for n in (1, 2, 3, 15, 16):
        assert len(rows["anchors_%d" % n].split()) == 2 * n
    assert {len(e["config"]["Anchors"][0]["Start"]) for e in model["named"] if e["name"].startswith("needle_len_")} == {1, 2, 4, 5, 31, 32}


def test_the_model_refuses_what_the_header_defines_as_refused():
    _, model = ac.load_fixtures()
    assert [e["name"] for e in model["refused"]] == ["seventeen_anchors", "start_of_33_bytes", "stop_of_33_bytes", "json_anchor"]
    for e in model["refused"]:
        with pytest.raises(anchor_model.Refused):
            anchor_model.init(e["config"])
    ok = anchor_model.init({"Anchors": [{"Start": "s" * 32, "Stop": "p" * 32, "FieldName": "f", "FieldType": "whatever"}] * 16})
    assert len(ok["Anchors"]) == 16 and not ok["KeepSource"] and not ok["NoKeyError"] and not ok["NoAnchorError"] and ok["SourceKey"] == b""
    assert anchor_model.cut_string(b"x" * 1023) == b"x" * 1023 and anchor_model.cut_string(b"x" * 1024 + b"y") == b"x" * 1024
