"""tests/helpers/kv_model.py (the reference's key_value_splitter.go restated with Go's bounds checks) against the two fixture files:
the reference's own unit test read as data (kv_unittest_vectors.json) and the model's recorded results (kv_model_vectors.json).  Which
tier pins what: tests/golden/README_kv.md."""
from helpers import kv_cases as kc
from helpers import kv_model


def test_the_model_gives_the_unit_tests_pairs():
    unit, _ = kc.load_fixtures()
    names = [e["case"] for e in unit["cases"]]
    assert names == ["TestSplit", "TestSplitWithEmptyKey", "TestSplitWithoutSeparator", "TestSplitWithMultiCharacterDelimiter",
                     "TestSplitWithChineseCharacter", "TestSplitWithQuote/1", "TestSplitWithQuote/2", "TestSplitWithQuote/3"]
    for e in unit["cases"]:
        source = e["config"]["SourceKey"]
        contents, alarms = kv_model.process_log(e["config"], [[source, e["value"]]])
        got = [[k.decode("utf-8"), v.decode("utf-8")] for k, v in contents]
        assert got[0] == [source, e["value"]] and len(got) == e["contents"], e["case"]  # KeepSource: the source stays in front
        assert got[1:] == e["pairs"], e["case"]                                        # in the order the Go appends them
        assert sorted(map(tuple, e["pairs"])) == sorted(map(tuple, e["stated"])), e["case"]  # exactly what the test states
        assert kc.rows_text(e["config"], e["value"].encode("utf-8")) == e["rows"] != kc.PANIC, e["case"]
    assert len(unit["cases"][-1]["pairs"]) == 18


def test_the_model_gives_the_recorded_results():
    """the named cases row by row; a random set by its digests: the seeded values are the recorded ones, the model's answers are the
    recorded ones -- and where they are not, the two characters per value say which value it is"""
    unit, model = kc.load_fixtures()
    for e in model["named"]:
        assert kc.rows_text(e["config"], e["value"].encode("utf-8")) == e["rows"], e["name"]
    for s in model["random"]:
        values = kc.random_values(s["config"], s["seed"], s["n"], s["longest"])
        got = kc.digest(values, [kc.rows_text(s["config"], v) for v in values])
        assert got["values_sha256"] == s["values_sha256"], s["name"]
        differing = [(i, values[i]) for i in range(s["n"]) if got["codes"][2 * i:2 * i + 2] != s["codes"][2 * i:2 * i + 2]]
        assert not differing and got["rows_sha256"] == s["rows_sha256"], (s["name"], differing[:5])
    assert len(kc.all_cases()) > 10000


def test_the_random_sets_keep_the_panic_caps():
    """no panic value with an empty or one-byte quote, at most 10 % with a longer one -- and some, so that the status is compared"""
    _, model = kc.load_fixtures()
    assert len(model["random"]) == 5
    for s in model["random"]:
        assert s["n"] == 2000 and len(s["codes"]) == 4000
        panics = s["codes"].count("!!")
        assert panics == s["panics"]
        if len(kv_model.init(s["config"])["Quote"]) <= 1:
            assert panics == 0, s["name"]
        else:
            assert 0 < panics <= 200, s["name"]
    named = {e["name"]: e["rows"] for e in model["named"]}
    assert named["long_quote_no_closing_panics"] == kc.PANIC and named["long_quote_wide_separator_closed_panics"] == kc.PANIC
    assert named["long_quote_no_closing_fits"] != kc.PANIC and named["long_quote_wide_separator_closed_fits"] != kc.PANIC


def test_the_models_slices_raise_where_go_panics():
    import pytest
    with pytest.raises(kv_model.GoPanic):
        kv_model._slice(b"abc", 0, 4)
    with pytest.raises(kv_model.GoPanic):
        kv_model._slice(b"abc", 3, 2)
    assert kv_model._slice(b"abc", 3, 3) == b"" and kv_model._from(b"abc", 3) == b""
    # Init's replacements of empty strings and newKeyValueSplitter's defaults
    c = kv_model.init({})
    assert (c["Delimiter"], c["Separator"], c["EmptyKeyPrefix"], c["NoSeparatorKeyPrefix"], c["Quote"]) == (b"\t", b":", b"empty_key_", b"no_separator_key_", b"")
    assert c["KeepSource"] and c["ErrIfSourceKeyNotFound"] and c["ErrIfSeparatorNotFound"] and c["ErrIfKeyIsEmpty"] and not c["DiscardWhenSeparatorNotFound"]
