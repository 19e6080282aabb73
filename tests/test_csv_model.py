"""tests/helpers/csv_model.py (the reader and writer rules of Go's encoding/csv as processor_csv uses them, line by line on bytes)
against the two fixture files -- the reference's own unit test read as data (csv_unittest_vectors.json) and the model's recorded results
(csv_model_vectors.json) -- and against two second opinions: CPython's csv module and the round trip through the model's own writer.
Which tier pins what: tests/golden/README_csv.md."""
import importlib.util
import os

import pytest

from helpers import csv_cases as cc
from helpers import csv_model


@pytest.fixture(scope="module")
def gen():
    """tests/golden/gen_csv_vectors.py as a module: the second opinions are the writer's own checks, run again on the recorded cases"""
    spec = importlib.util.spec_from_file_location("gen_csv_vectors", os.path.join(cc.GOLDEN, "gen_csv_vectors.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_model_gives_every_stated_value_of_the_unit_test():
    unit, _ = cc.load_fixtures()
    assert len(unit["cases"]) == 21 and sum(1 for e in unit["cases"] if not e["res"]) == 5
    for e in unit["cases"]:
        contents = [[b"content", e["value"].encode("utf-8")]]
        res, _ = csv_model.decode_csv(csv_model.init(e["config"]), contents, e["value"].encode("utf-8"))
        assert res == e["res"], e["case"]
        got = [[k.decode("utf-8"), v.decode("utf-8")] for k, v in contents]
        if e["contents"] is not None:  # (the test calls decodeCSV directly: the source content stays in the count)
            assert len(got) == e["contents"], e["case"]
        for i, v in e["values"].items():
            assert got[int(i)][1] == v, (e["case"], i)
        for i, k in e["keys"].items():
            assert got[int(i)][0] == k, (e["case"], i)
        assert got[1:] == e["appended"] and (res or got[1:] == []), e["case"]
        assert cc.result_text(e["config"], e["value"].encode("utf-8")) == e["result"], e["case"]


def test_the_model_gives_the_recorded_results():
    """the named cases one by one; a random set by its digests: the seeded values are the recorded ones, the model's answers are the
    recorded ones -- and where they are not, the two characters per value say which value it is"""
    _, model = cc.load_fixtures()
    assert len(model["named"]) > 150
    for e in model["named"]:
        assert cc.result_text(e["config"], e["value"].encode("latin-1")) == e["result"], e["name"]
    for s in model["random"]:
        values = cc.random_values(s["config"], s["seed"], s["n"], s["longest"])
        assert all(len(v) <= 24 for v in values)
        got = cc.digest(values, [cc.result_text(s["config"], v) for v in values])
        assert got["values_sha256"] == s["values_sha256"], s["name"]
        differing = [(i, values[i]) for i in range(s["n"]) if got["codes"][2 * i:2 * i + 2] != s["codes"][2 * i:2 * i + 2]]
        assert not differing and got["results_sha256"] == s["results_sha256"], (s["name"], differing[:5])
    assert len(cc.all_cases()) > 10000


def test_in_every_random_set_30_percent_decode_and_30_percent_fail():
    _, model = cc.load_fixtures()
    assert len(model["random"]) == 5
    assert sorted(len(cc.reader_config(s["config"])[0]) for s in model["random"]) == [1, 1, 1, 3, 3]
    assert sum(1 for s in model["random"] if cc.reader_config(s["config"])[1]) == 3
    for s in model["random"]:
        assert s["n"] == 2000 and len(s["codes"]) == 4000
        codes = [s["codes"][i:i + 2] for i in range(0, 4000, 2)]
        failed = sum(1 for c in codes if c in ("!B", "!Q"))
        assert 2000 - failed == s["decoded"] and s["decoded"] >= 600 and failed >= 600, (s["name"], s["decoded"], failed)
        assert codes.count("!B") > 100 and codes.count("!Q") > 100 and codes.count("!E") > 20, s["name"]


NAMED_RESULTS = {  # a few of the named cases stated here by hand, from the rules' text
    "empty_lines_mixed:1": "0:61,62", "only_empty_lines:1": "1", "cr_alone_is_eof:1": "1", "second_record_ignored:3": "0:61,62",
    "cr_at_value_end_unquoted:1": "0:61,62", "two_cr_at_value_end_unquoted:1": "0:61,620d", "cr_in_the_middle_of_a_field:1": "0:610d62,63",
    "crlf_inside_quotes:1": "0:610a62,63", "lone_cr_inside_quotes:3": "0:610d62,63", "cr_cr_lf_inside_quotes:1": "0:610d0a62,63",
    "quoted_field_over_three_lines:1": "0:78," + b"one\ntwo\nthree".hex() + ",79", "four_quotes:1": "0:22", "six_quotes:1": "0:2222",
    "doubled_quote_at_the_start:1": "0:2261,62", "doubled_quote_at_the_end:3": "0:6122,62", "closing_quote_then_crlf:1": "0:61",
    "closing_quote_then_cr_at_value_end:1": "0:61", "closing_quote_then_cr_then_other:1": "3", "closing_quote_then_other_byte:1": "3",
    "unterminated_at_value_end:1": "3", "unterminated_behind_lf:1": "3", "unterminated_behind_crlf:3": "3", "bare_quote_in_the_first_field:1": "2",
    "bare_quote_in_the_last_field:3": "2", "quote_behind_blank_without_trimming:1": "2", "empty_value:1": "1", "value_is_the_separator:3": "0:,",
    "trailing_separator:1": "0:61,62,", "trim_quote_behind_space:1": "0:61,62", "trim_blanks_only_line:1": "0:", "blanks_only_line_without_trimming:1": "0:2020",
    "trim_eats_the_lines_lf:1": "0:61,", "trim_empty_line_test_comes_first:1": "0:", "trim_c2_then_other_byte:1": "0:c2a161,62",
    "trim_truncated_e2_80_at_line_end:1": "0:61,e280", "trim_rune_e38080:3": "0:78,79,7a", "trim_rune_0a:1": "0:78,",
    "separator_first_byte_begins_another_character:3": "0:" + "a－b".encode().hex() + "," + "c｜d".encode().hex() + ",",
    "separator_first_two_bytes_then_the_value_ends:3": "0:61,62efbc", "separator_behind_closing_quote_near_miss:3": "3",
}


def test_named_cases_stated_by_hand():
    _, model = cc.load_fixtures()
    named = {e["name"]: e["result"] for e in model["named"]}
    for name, result in NAMED_RESULTS.items():
        assert named[name] == result, name
    for r in csv_model.SPACE_RUNES:  # trimming, for every white-space rune of the list
        assert "trim_rune_%s:1" % r.hex() in named and "trim_rune_%s:3" % r.hex() in named


def test_cpython_reads_the_same_first_record_and_the_round_trip_holds(gen):
    """every value the model decodes that holds no `\\r`, trimming off, a one-byte separator -- none left out -- through CPython's csv.reader
    (strict); and 1 to 6 random fields through the model's writer and back through its reader, for every random configuration"""
    cases = cc.all_cases()
    compared, trips = gen.check_second_opinions(cases)
    eligible = sum(1 for _, config, value, result in cases
                   if result[0] == "0" and b"\r" not in value and cc.reader_config(config) == (b",", False))
    assert compared == eligible > 300 and trips == 2000


def test_the_writer_quotes_as_csv_writer_does():
    w = csv_model.write
    assert w([b"78", b"90"]) == b"78,90\n" and w([b"normal", b'"quote"', b","]) == b'normal,"""quote""",","\n'
    assert w([b"  78", b"  ", b"  90"]) == b'"  78","  ","  90"\n' and w([b"78  ", b"  ", b"90  "]) == b'78  ,"  ",90  \n'
    assert w([b"", b"\\.", b"a\rb", b"a\nb"]) == b',"\\.","a\rb","a\nb"\n' and w([b"\xc2\xa0x", b"\xc2\xa1x"]) == b'"\xc2\xa0x",\xc2\xa1x\n'
    wide = cc.WIDE.encode()
    assert w([b"a,b", b"c" + wide + b"d"], wide) == b"a,b" + wide + b'"c' + wide + b'd"\n'


def test_init_takes_exactly_one_rune():
    for sep in ("", ",,", "ab", "，，"):
        with pytest.raises(csv_model.InvalidSeparator, match="invalid separator: " + sep):
            csv_model.init({"SplitSep": sep})
    for sep in ('"', "\r", "\n", "\0", "\ufffd"):
        assert csv_model.init({"SplitSep": sep})["valid"] is False
    assert csv_model.init({})["sep"] == b"," and csv_model.init({"SplitSep": "，"})["valid"] and csv_model.init({"SplitSep": "\U0001F600"})["valid"]
    assert csv_model.go_runes(b"\xffa") == [0xFFFD, ord("a")] and csv_model.go_runes("é，".encode()) == [0xE9, 0xFF0C]
