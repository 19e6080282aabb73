"""Writes tests/golden/anchor_unittest_vectors.json and tests/golden/anchor_model_vectors.json (run by hand:
python tests/golden/gen_anchor_vectors.py).

anchor_unittest_vectors.json: the cases of the reference's plugins/processor/anchor/anchor_test.go read as DATA -- TestSourceKey's value
with its two string anchors and the two results the test states for them, and the no-key / no-start / no-stop cases with the alarm
substrings they state.  Those three are recorded as stated (`config`, FieldType "json") AND as run (`run_config`, the same anchors as
string anchors): all three outcomes happen at anchor.go:175-189, before the type is looked at at :197.  The writer asserts that
tests/helpers/anchor_model.py gives exactly the stated results.

anchor_model_vectors.json: configurations, values and the model's recorded results (no program text): named cases aimed at every branch
of :172-199, configurations that are refused, and three seeded random sets of 2000 values over small alphabets that contain the
needles.  The writer asserts that in every set every outcome an anchor can reach (field, no start, no stop) holds at least 3 % of the
values.  Compact form (README_anchor.md): a result is b and e of every anchor joined by blanks; a random set is its seed and symbols
(helpers/anchor_cases.random_values makes the values) with digests of the values and of the recorded results."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from helpers import anchor_cases as ac  # noqa: E402
from helpers import anchor_model  # noqa: E402

RANDOM_PER_CONFIG, LONGEST = 2000, 24
SEED = 20261021
FLOOR = 0.03


# ---------------------------------------------------------------------------------------------- the reference's unit test, as data
def unittest_cases():
    source_value = ("time:2017.09.12 20:55:36" + "\\tlevel:info" +
                    "\\tjson:{\"key1\" :\"xx\", \"key2\": false, \"key3\":123.456, \"key4\" : { \"inner1\" : 1, \"inner2\" : false}}" +
                    "\\tjson2:{\"key\" : { \"inner1\" : 1, \"inner2\" : false}}")
    json_value = "json:{\"key\" : { \"inner1\" : 1, \"inner2\" : false}}"
    out = []
    # TestSourceKey: the two string anchors of newProcessor (the three json anchors behind them are out of this project's scope)
    config = {"Anchors": [{"Start": "time:", "Stop": "\\t", "FieldName": "time", "FieldType": "string", "ExpondJSON": False},
                          {"Start": "level:", "Stop": "\\t", "FieldName": "level", "ExpondJSON": False}],
              "SourceKey": "content", "NoKeyError": True}
    stated = [["time", "2017.09.12 20:55:36"], ["level", "info"]]
    contents, alarms, _ = anchor_model.process_log(config, [["content", source_value]])
    assert [[k.decode(), v.decode()] for k, v in contents] == stated and alarms == []
    out.append({"case": "TestSourceKey", "config": config, "run_config": config, "log": [["content", source_value]], "value": source_value,
                "stated": stated, "rows": ac.rows_text(config, source_value)})

    def alarm_case(name, anchor, log, substring, kind):
        as_stated = {"Anchors": [dict(anchor)], "SourceKey": "content", "NoKeyError": True, "NoAnchorError": True}
        as_run = {"Anchors": [{k: v for k, v in anchor.items() if k != "FieldType"}], "SourceKey": "content", "NoKeyError": True, "NoAnchorError": True}
        if name == "TestNoKeyError":
            del as_stated["NoAnchorError"], as_run["NoAnchorError"]
        contents, alarms, _ = anchor_model.process_log(as_run, log)
        assert len(alarms) == 1 and alarms[0][0] == kind and substring.encode() in alarms[0][1], (name, alarms)
        e = {"case": name, "config": as_stated, "run_config": as_run, "log": log, "stated_alarm": substring, "alarm_kind": kind,
             "alarm": alarms[0][1].decode(), "contents": [[k.decode(), v.decode()] for k, v in contents]}
        if log[0][0] == "content":
            e["value"] = log[0][1]
            e["rows"] = ac.rows_text(as_run, log[0][1])
        return e
    out.append(alarm_case("TestNoKeyError", {"Start": "NoKeyError:", "Stop": "", "FieldName": "NoKeyError"}, [["test_key", "test_value"]],
                          "anchor cannot find key:content", anchor_model.ALARM_NO_KEY))
    json_anchor = {"FieldName": "test", "FieldType": "json", "ExpondJSON": True, "IgnoreJSONError": False}
    out.append(alarm_case("TestNoAnchorErrorNoStart", dict(json_anchor, Start="666", Stop=""), [["content", json_value]], "anchor no start",
                          anchor_model.ALARM_NO_START))
    out.append(alarm_case("TestNoAnchorErrorNoStop", dict(json_anchor, Start="json:", Stop="888"), [["content", json_value]], "anchor no stop",
                          anchor_model.ALARM_NO_STOP))
    return out


# ---------------------------------------------------------------------------------------------- named model cases
A31 = "0123456789abcdefghijklmnopqrstu"
A32 = A31 + "v"
NAMED = [
    # empty needles
    ("start_empty", [("", ",")], "ab,cd", ""),
    ("start_empty_no_stop", [("", ",")], "abcd", ""),
    ("stop_empty", [("b", "")], "abcd", ""),
    ("stop_empty_start_at_the_end", [("cd", "")], "abcd", ""),
    ("both_empty", [("", "")], "abcd", ""),
    ("both_empty_empty_value", [("", "")], "", ""),
    ("start_empty_empty_value", [("", ",")], "", ""),
    ("stop_empty_no_start", [("x", "")], "abcd", ""),
    # the order of Start and Stop
    ("stop_directly_behind_start", [("k=", ";")], "k=;x", ""),
    ("stop_only_before_b", [("k=", ";")], ";;k=abc", ""),
    ("stop_before_and_behind", [("k=", ";")], ";k=ab;c;", ""),
    ("stop_overlaps_starts_tail", [("ab", "ba")], "aba", ""),
    ("stop_overlaps_starts_tail_then_real", [("ab", "ba")], "ababa", ""),
    ("start_in_one_quad_stop_in_the_same", [("<", ">")], "xx<yy>zz", ""),
    ("second_start_is_not_looked_at", [("k=", ";")], "k=a k=b;", ""),
    # self-overlapping needles
    ("aab_in_aaab", [("aab", "")], "aaab", ""),
    ("aab_stop_in_aaab", [("", "aab")], "aaab", ""),
    ("aa_aa_on_aaa", [("aa", "aa")], "aaa", ""),
    ("aa_aa_on_aaaa", [("aa", "aa")], "aaaa", ""),
    ("aa_aa_on_aaaaa", [("aa", "aa")], "aaaaa", ""),
    ("aba_ab_on_ababab", [("aba", "ab")], "ababab", ""),
    # near misses
    ("near_miss_start", [("time:", ";")], "time time:12;", ""),
    ("near_miss_stop", [("t:", "END")], "t:a EN ENDEND", ""),
    ("near_miss_both_many", [("abc:", "#?#")], "abcabc:x#?x#?#y", ""),
    # the value's end
    ("needle_tail_in_the_next_value", [("abc", "")], "xxab", "cdef"),
    ("stop_tail_in_the_next_value", [("x", "#?#")], "xab#?", "#rest"),
    ("one_byte_stop_is_the_next_values_first_byte", [("x", ";")], "xab", ";"),
    ("start_is_the_values_last_bytes", [("abc", ";")], "xxabc", ";"),
    ("value_empty", [("a", "b")], "", "ab"),
    ("value_is_start", [("abc", ";")], "abc", ""),
    ("value_is_start_stop_empty", [("abc", "")], "abc", ""),
    ("value_is_start_plus_stop", [("abc", ";;")], "abc;;", ""),
    ("stop_is_the_values_last_byte", [("k=", ";")], "k=" + "v" * 70 + ";", ""),
    ("start_across_the_first_stage_border", [("time:", "\t")], "x" * 61 + "time:12\tz", ""),
    ("stop_far_behind", [("a", "END")], "a" + "x" * 200 + "END", ""),
    # several anchors
    ("two_anchors_same_start", [("k=", ";"), ("k=", " ")], "k=a b;c", ""),
    ("one_anchors_start_is_anothers_stop", [("a:", "b:"), ("b:", "c:")], "a:1b:2c:3", ""),
    ("anchors_in_reverse_order_of_the_value", [("level:", "\t"), ("time:", "\t")], "time:12\tlevel:info\t", ""),
    ("a_missing_anchor_drops_only_its_field", [("a=", ";"), ("zz=", ";"), ("c=", ";")], "a=1;c=3;", ""),
    ("three_outcomes_side_by_side", [("a=", ";"), ("q=", ";"), ("c=", "!")], "a=1;c=3;", ""),
    # needle lengths 1, 2, 4, 5, 31, 32
    ("needle_len_1", [("<", ">")], "a<b>c", ""),
    ("needle_len_2", [("<<", ">>")], "a<<<b>>>c", ""),
    ("needle_len_4", [("BEG:", ":END")], "xBEGBEG:mid:EN:ENDx", ""),
    ("needle_len_5", [("time:", "level")], "time:12 leve level", ""),
    ("needle_len_31", [(A31, A31)], "x" + A31 + "mid" + A31[:30] + A31 + "y", ""),
    ("needle_len_32", [(A32, A32)], "xx" + A32[:31] + A32 + "mid" + A32 + "y", ""),
    ("needle_len_32_cut_by_the_end", [(A32, "")], "xx" + A32[:31], "v"),
    # anchor counts 1, 2, 3, 15, 16
    ("anchors_1", [("k0=", ";")], "k0=a;k1=b;", ""),
    ("anchors_2", [("k%d=" % i, ";") for i in range(2)], "k0=a;k1=b;", ""),
    ("anchors_3", [("k%d=" % i, ";") for i in range(3)], "k0=a;k1=b;k2=c", ""),
    ("anchors_15", [("k%d=" % i, ";") for i in range(15)], "".join("k%d=v%d;" % (i, i) for i in range(0, 15, 2)) + "k13=open", ""),
    ("anchors_16", [("k%d=" % i, ";") for i in range(16)], "".join("k%d=v%d;" % (i, i) for i in range(15, -1, -3)) + "k14=open", ""),
]

REFUSED = [
    ("seventeen_anchors", {"Anchors": [{"Start": "k%d=" % i, "Stop": ";", "FieldName": "f%d" % i} for i in range(17)]}, "17 anchors"),
    ("start_of_33_bytes", {"Anchors": [{"Start": "s" * 33, "Stop": ";", "FieldName": "f"}]}, "Start is 33 bytes long"),
    ("stop_of_33_bytes", {"Anchors": [{"Start": "s", "Stop": ";" * 33, "FieldName": "f"}]}, "Stop is 33 bytes long"),
    ("json_anchor", {"Anchors": [{"Start": "a", "Stop": "b", "FieldName": "ok"}, {"Start": "json:", "Stop": "", "FieldName": "val", "FieldType": "json"}]},
     "anchor 1 (FieldName \"val\") has FieldType \"json\""),
]

RANDOM_CONFIGS = [
    ("one_byte_needles", [(":", ","), (",", ":"), (" ", " ")], ["a", "b", ":", ",", " "]),
    ("overlapping_ab_needles", [("ab", "ba"), ("aab", "b"), ("aa", "aa"), ("aba", "ab")], ["a", "b", "c"]),
    ("three_and_four_byte_needles", [("abc:", "#?#"), ("#?#", "abc:"), ("c:#", "?#a")], ["a", "b", "c", ":", "#", "?", "abc:", "#?#"]),
]


def main():
    unit = {"source": "plugins/processor/anchor/anchor_test.go, read as data", "cases": unittest_cases()}
    with open(os.path.join(HERE, "anchor_unittest_vectors.json"), "w", encoding="utf-8") as f:
        json.dump(unit, f, ensure_ascii=False, separators=(",", ":"))
    named = []
    for name, pairs, value, tail in NAMED:
        config = ac.config_of(pairs)
        e = {"name": name, "config": config, "value": value, "rows": ac.rows_text(config, value)}
        if tail:
            e["tail"] = tail
        named.append(e)
    assert len({e["name"] for e in named}) == len(named)
    by_name = {e["name"]: e["rows"] for e in named}
    assert by_name["stop_overlaps_starts_tail"] == "-2 -1" and by_name["aa_aa_on_aaa"] == "-2 -1" and by_name["aa_aa_on_aaaa"] == "2 2"
    assert by_name["needle_tail_in_the_next_value"] == "-1 -1" and by_name["aab_in_aaab"] == "4 4"
    for name, config, _ in REFUSED:
        try:
            anchor_model.init(config)
        except anchor_model.Refused:
            continue
        raise AssertionError(name)
    sets, report = [], {}
    for k, (name, pairs, symbols) in enumerate(RANDOM_CONFIGS):
        config = ac.config_of(pairs)
        values = ac.random_values([s.encode() for s in symbols], SEED + k, RANDOM_PER_CONFIG, LONGEST)
        rows = [ac.rows_text(config, v) for v in values]
        shares = ac.outcome_shares(config, values)
        for a, (start, stop) in zip(shares, pairs):
            for outcome, share in a.items():
                if (outcome == "no_start" and start == "") or (outcome == "no_stop" and stop == ""):
                    continue  # (an outcome the anchor cannot reach)
                assert share >= FLOOR, (name, start, stop, outcome, share)
        report[name] = min(min(a.values()) for a in shares)
        sets.append(dict({"name": name, "config": config, "symbols": symbols, "seed": SEED + k, "n": RANDOM_PER_CONFIG, "longest": LONGEST,
                          "smallest_share": round(report[name], 4)}, **ac.digest(values, rows)))
    model = {"seed": SEED, "named": named, "refused": [{"name": n, "config": c, "message": m} for n, c, m in REFUSED], "random": sets}
    with open(os.path.join(HERE, "anchor_model_vectors.json"), "w", encoding="utf-8") as f:
        json.dump(model, f, ensure_ascii=False, separators=(",", ":"))
    print("unit cases %d, named %d, refused %d, smallest outcome shares %r" % (len(unit["cases"]), len(named), len(REFUSED), report))
    for fn in ("anchor_unittest_vectors.json", "anchor_model_vectors.json"):
        print(fn, os.path.getsize(os.path.join(HERE, fn)))


if __name__ == "__main__":
    main()
