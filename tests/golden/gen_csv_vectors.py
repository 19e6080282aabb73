"""Writes tests/golden/csv_unittest_vectors.json and tests/golden/csv_model_vectors.json (run by hand: python tests/golden/gen_csv_vectors.py).

csv_unittest_vectors.json: the cases of the reference's plugins/processor/csv/processor_csv_test.go read as DATA -- the configuration,
the source value, the stated result of decodeCSV, the stated number of contents and the stated values (the test calls decodeCSV
directly, so the source content stays in the count).  The writer asserts that tests/helpers/csv_model.py reproduces every stated value.

csv_model_vectors.json: configurations, values and the model's recorded results (no program text): named cases aimed at every branch
of the reader rules, each for a one-byte and a three-byte separator, and 2000 seeded random values per configuration over the alphabet
a, b, blank, tab, '"', the separator, \\r, \\n (and C2 A0 where TrimLeadingSpace is on).  The writer asserts that in every random set at
least 30 % of the values decode and at least 30 % fail, that CPython's csv module reads the same first record wherever the two readers'
rules coincide, and the round trip through the model's writer.  Compact form (README_csv.md): a named value and its fields are Latin-1
text (one character per byte), a result is the status code and, for a record, ":" and the fields in hex; a random set is its seed
(helpers/csv_cases.random_values makes the values) with digests of the values and of the recorded results (helpers/csv_cases.digest)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from helpers import csv_cases, csv_model  # noqa: E402

RANDOM_PER_CONFIG, LONGEST = 2000, 24
SEED = 20261020


# ---------------------------------------------------------------------------------------------- the reference's unit test, as data
def unittest_cases():
    base = {"SplitSep": ",", "SplitKeys": ["f1", "f2", "f3"]}
    preserve = dict(base, PreserveOthers=True)
    trimming = dict(preserve, TrimLeadingSpace=True)
    expand = dict(preserve, ExpandOthers=True, ExpandKeyPrefix="expand_")
    js = '  words{"a":123,"b":"string","c":[1,2,3],"d":{"e":"string"}}  '
    # (group, case, config, value, stated result, stated number of contents or None, {index: stated value}, {index: stated key})
    cases = [
        ("plain", "zero value", base, "", True, 2, {1: ""}, {}),
        ("plain", "purely blank chars", base, "  ", True, 2, {1: "  "}, {}),
        ("plain", "single field", base, "12", True, 2, {1: "12"}, {}),
        ("plain", "fits the schema", base, "12,34,56", True, 4, {1: "12", 2: "34", 3: "56"}, {1: "f1", 2: "f2", 3: "f3"}),
        ("plain", "fits the schema, all fields quoted", base, '"normal","""quote""",","', True, 4, {1: "normal", 2: '"quote"', 3: ","}, {}),
        ("plain", "fewer fields than keys", base, "12,34", True, 3, {1: "12", 2: "34"}, {}),
        ("plain", "more fields than keys", base, "12,34,56,78,90", True, 4, {1: "12", 2: "34", 3: "56"}, {}),
        ("plain", "includes json", base, '"' + js.replace('"', '""') + '"', True, 2, {1: js}, {}),
        ("plain", "upper quote has leading words", base, '12",34,56', False, None, {}, {}),
        ("plain", "upper quote has leading space", base, '  "12,34,56', False, None, {}, {}),
        ("plain", "bare quotes", base, '"12,34,56', False, None, {}, {}),
        ("plain", "lower quote has trailing words", base, '12","34,56', False, None, {}, {}),
        ("plain", "lower quote has trailing space", base, '"12"  ,34,56', False, None, {}, {}),
        ("preserve", "more fields than keys", preserve, "12,34,56,78,90", True, 5, {1: "12", 2: "34", 3: "56", 4: "78,90"}, {}),
        ("preserve", "more fields than keys, all quoted", preserve, '12,34,56,"normal","""quote""",","', True, 5,
         {1: "12", 2: "34", 3: "56", 4: 'normal,"""quote""",","'}, {}),
        ("preserve", "leading space", preserve, '  12,  ,"  34",  78,  ,"  90"', True, 5, {1: "  12", 2: "  ", 3: "  34", 4: '"  78","  ","  90"'}, {}),
        ("preserve", "trailing space", preserve, '12  ,  ,"34  ",78  ,  ,"90  "', True, 5, {1: "12  ", 2: "  ", 3: "34  ", 4: '78  ,"  ",90  '}, {}),
        ("trim", "purely blank chars", trimming, "  ", True, 2, {1: ""}, {}),
        ("trim", "leading space", trimming, '  12,  ,"  34",  78,  ,"  90"', True, 5, {1: "12", 2: "", 3: "  34", 4: '78,,"  90"'}, {}),
        ("trim", "upper quote has leading space", trimming, '  "12",34,56', True, 4, {1: "12", 2: "34", 3: "56"}, {}),
        ("expand", "more fields than keys", expand, '12,34,56,"normal","""quote""",","', True, 7,
         {1: "12", 2: "34", 3: "56", 4: "normal", 5: '"quote"', 6: ","}, {4: "expand_1", 5: "expand_2", 6: "expand_3"}),
    ]
    out = []
    for group, case, config, value, res, contents, values, keys in cases:
        c = csv_model.init(config)
        got = [[b"content", value.encode("utf-8")]]
        ok, _ = csv_model.decode_csv(c, got, value.encode("utf-8"))
        assert ok == res, (group, case, ok)
        if contents is not None:
            assert len(got) == contents, (group, case, len(got))
        for i, v in values.items():
            assert got[i][1].decode("utf-8") == v, (group, case, i, got[i][1])
        for i, k in keys.items():
            assert got[i][0].decode("utf-8") == k, (group, case, i, got[i][0])
        out.append({"case": group + "/" + case, "config": config, "value": value, "res": res, "contents": contents,
                    "values": {str(i): v for i, v in values.items()}, "keys": {str(i): k for i, k in keys.items()},
                    "appended": [[k.decode("utf-8"), v.decode("utf-8")] for k, v in got[1:]],
                    "result": csv_cases.result_text(config, value.encode("utf-8"))})
    return out


# ---------------------------------------------------------------------------------------------- named model cases
# values are written with `,` for the separator; each is recorded for `,` and for the three-byte separator
T = True
NAMED = [
    # leading empty lines
    ("empty_lines_lf", False, b"\n\na,b"),
    ("empty_lines_crlf", False, b"\r\n\r\na,b"),
    ("empty_lines_mixed", False, b"\n\r\n\n\r\na,b\n"),
    ("only_empty_lines", False, b"\n\r\n\n"),
    ("only_empty_lines_then_cr", False, b"\n\r\n\r"),
    ("empty_line_of_two_cr_is_a_record", False, b"\r\r\na"),
    ("second_record_ignored", False, b"a,b\nc,d,e\n"),
    ("second_record_with_a_bare_quote_ignored", False, b'a,b\nc"d'),
    # \r
    ("cr_at_value_end_unquoted", False, b"a,b\r"),
    ("two_cr_at_value_end_unquoted", False, b"a,b\r\r"),
    ("cr_alone_is_eof", False, b"\r"),
    ("cr_in_the_middle_of_a_field", False, b"a\rb,c"),
    ("crlf_ends_the_record", False, b"a,b\r\nc"),
    ("cr_cr_lf_keeps_one_cr", False, b"a,b\r\r\nc"),
    ("empty_last_field_before_crlf", False, b"a,\r\nc"),
    ("crlf_inside_quotes", False, b'"a\r\nb",c'),
    ("lone_cr_inside_quotes", False, b'"a\rb",c'),
    ("cr_cr_lf_inside_quotes", False, b'"a\r\r\nb",c'),
    ("cr_before_the_closing_quote", False, b'"a\r",c'),
    ("quoted_field_over_three_lines", False, b'x,"one\ntwo\r\nthree",y\nz'),
    ("quoted_field_with_an_empty_line_inside", False, b'"a\n\nb"'),
    # "" inside quotes
    ("doubled_quote_at_the_start", False, b'"""a",b'),
    ("doubled_quote_in_the_middle", False, b'"a""b",c'),
    ("doubled_quote_at_the_end", False, b'"a""",b'),
    ("four_quotes", False, b'""""'),
    ("four_quotes_then_a_field", False, b'"""",a'),
    ("two_quotes_are_an_empty_field", False, b'"",a'),
    ("six_quotes", False, b'""""""'),
    # behind a closing quote
    ("closing_quote_then_separator", False, b'"a",b'),
    ("closing_quote_then_lf", False, b'"a"\nb'),
    ("closing_quote_then_crlf", False, b'"a"\r\nb'),
    ("closing_quote_then_cr_at_value_end", False, b'"a"\r'),
    ("closing_quote_then_cr_then_other", False, b'"a"\rb'),
    ("closing_quote_then_cr_cr_lf", False, b'"a"\r\r\n'),
    ("closing_quote_then_other_byte", False, b'"a"b,c'),
    ("closing_quote_then_blank", False, b'"a" ,c'),
    ("closing_quote_at_value_end", False, b'a,"b"'),
    # unterminated
    ("unterminated_at_value_end", False, b'a,"bc'),
    ("unterminated_behind_lf", False, b'a,"bc\n'),
    ("unterminated_behind_crlf", False, b'a,"bc\r\n'),
    ("unterminated_behind_cr", False, b'a,"bc\r'),
    ("lone_quote", False, b'"'),
    # bare quotes
    ("bare_quote_in_the_first_field", False, b'a"b,c'),
    ("bare_quote_in_the_last_field", False, b'a,b,c"'),
    ("bare_quote_behind_the_line_is_ignored", False, b'a,b\n"'),
    ("quote_behind_blank_without_trimming", False, b' "a",b'),
    # ends
    ("empty_value", False, b""),
    ("value_is_the_separator", False, b","),
    ("trailing_separator", False, b"a,b,"),
    ("trailing_separator_then_lf", False, b"a,b,\nc"),
    ("separator_behind_a_closing_quote_at_value_end", False, b'"a",'),
    ("backslash_dot", False, b"\\.,a"),
    # trimming
    ("trim_quote_behind_space", T, b'  "a",\t"b"'),
    ("trim_blanks_only_line", T, b"  \nb"),
    ("blanks_only_line_without_trimming", False, b"  \nb"),
    ("trim_eats_the_lines_lf", T, b"a, \t\nb"),
    ("trim_eats_crlf", T, b"a, \r\nb"),
    ("trim_eats_cr_at_value_end", T, b"a, \r"),
    ("trim_empty_line_test_comes_first", T, b"\n \na"),
    ("trim_at_value_end", T, b"a,  "),
    ("trim_c2_then_other_byte", T, b" \xc2\xa1a,b"),
    ("trim_c2_then_ascii", T, b" \xc2a,b"),
    ("trim_c2_at_value_end", T, b"a, \xc2"),
    ("trim_truncated_e2_80_at_line_end", T, b"a, \xe2\x80\nb"),
    ("trim_truncated_e2_80_at_value_end", T, b"a, \xe2\x80"),
    ("trim_e2_80_8b_is_no_space", T, b"\xe2\x80\x8ba,b"),
    ("trim_e2_81_a0_is_no_space", T, b"\xe2\x81\xa0a,b"),
    ("trim_space_then_bare_quote_later", T, b' a"b'),
    ("trim_not_inside_quotes", T, b'"  a", "\n  b"'),
    ("trim_closing_quote_then_blank_is_an_error", T, b'"a" ,b'),
]
NAMED += [("trim_rune_%s" % r.hex(), T, b"x," + r + b"y," + r + r + b'"z"') for r in csv_model.SPACE_RUNES if r != b"\n"]
NAMED += [("trim_rune_0a", T, b"x,\ny")]
# a separator whose first byte also begins another character of the value (EF BC 8C beside EF BC 8D and EF BD 9C), three-byte only
WIDE_ONLY = [
    ("separator_first_byte_begins_another_character", False, "a－b，c｜d，".encode("utf-8")),
    ("separator_first_two_bytes_then_the_value_ends", False, "a，b".encode("utf-8") + b"\xef\xbc"),
    ("separator_behind_closing_quote_near_miss", False, '"a"'.encode("utf-8") + b"\xef\xbc\x8d"),
]

RANDOM_CONFIGS = [
    ("comma", {"SplitSep": ","}),
    ("comma_trim", {"SplitSep": ",", "TrimLeadingSpace": True}),
    ("wide", {"SplitSep": csv_cases.WIDE}),
    ("wide_trim", {"SplitSep": csv_cases.WIDE, "TrimLeadingSpace": True}),
    ("semicolon_trim", {"SplitSep": ";", "TrimLeadingSpace": True}),
]


def cpython_first_record(value, sep):
    """CPython's csv module on the same text: the first record that is not empty (CPython reports an empty line as the record []; the
    Go skips it).  The text goes in line by line, as a file would hand it over: csv.reader takes an iterable of LINES and refuses a
    line end that is followed by more text in one item."""
    import csv
    import io
    for row in csv.reader(io.StringIO(value.decode("latin-1"), newline=""), delimiter=sep.decode(), strict=True, skipinitialspace=False):
        if row:
            return [f.encode("latin-1") for f in row]
    return None


def check_second_opinions(cases):
    """-> (values compared with CPython, round trips made)"""
    import csv
    import random
    compared = 0
    for label, config, value, result in cases:
        sep, trim = csv_cases.reader_config(config)
        code, fields = csv_cases.fields_of(result)
        if code != 0 or b"\r" in value or trim or len(sep) != 1:
            continue
        try:
            got = cpython_first_record(value, sep)
        except csv.Error as e:
            raise AssertionError((label, value, "CPython: %s" % e))
        assert got == fields, (label, value, got, fields)
        compared += 1
    rng, trips = random.Random(SEED), 0
    for name, config in RANDOM_CONFIGS:
        sep, _ = csv_cases.reader_config(config)
        syms = [s for s in csv_cases.symbols(config) if s != b"\r"]
        for _ in range(400):
            fields = [b"".join(syms[rng.randrange(len(syms))] for _ in range(rng.randint(0, 6))) for _ in range(rng.randint(1, 6))]
            line = csv_model.write(fields, sep)
            status, back = csv_model.read(line, sep, False)
            if fields == [b""]:  # the writer's line for the record [""] is the empty line, which the reader skips
                assert (status, back) == (csv_model.EOF, []), (fields, line)
            else:
                assert (status, back) == (csv_model.OK, fields), (fields, line, status, back)
            trips += 1
    return compared, trips


def main():
    unit = {"source": "plugins/processor/csv/processor_csv_test.go, read as data", "cases": unittest_cases()}
    with open(os.path.join(HERE, "csv_unittest_vectors.json"), "w", encoding="utf-8") as f:
        json.dump(unit, f, ensure_ascii=True, separators=(",", ":"))
    named = []
    wide = csv_cases.WIDE.encode("utf-8")
    for name, trim, value in NAMED:
        for tag, sep in (("1", b","), ("3", wide)):
            config = {"SplitSep": sep.decode("utf-8"), "TrimLeadingSpace": bool(trim)}
            v = value.replace(b",", sep)
            named.append({"name": name + ":" + tag, "config": config, "value": v.decode("latin-1"), "result": csv_cases.result_text(config, v)})
    for name, trim, value in WIDE_ONLY:
        config = {"SplitSep": csv_cases.WIDE, "TrimLeadingSpace": bool(trim)}
        named.append({"name": name + ":3", "config": config, "value": value.decode("latin-1"), "result": csv_cases.result_text(config, value)})
    assert len({e["name"] for e in named}) == len(named)
    for code in "0123":
        assert sum(1 for e in named if e["result"][0] == code) >= 4, code
    sets, counts = [], {}
    for k, (name, config) in enumerate(RANDOM_CONFIGS):
        values = csv_cases.random_values(config, SEED + k, RANDOM_PER_CONFIG, LONGEST)
        results = [csv_cases.result_text(config, v) for v in values]
        decoded = sum(1 for r in results if r[0] in "01")
        failed = RANDOM_PER_CONFIG - decoded
        assert decoded * 10 >= RANDOM_PER_CONFIG * 3 and failed * 10 >= RANDOM_PER_CONFIG * 3, (name, decoded, failed)
        counts[name] = decoded
        sets.append(dict({"name": name, "config": config, "seed": SEED + k, "n": RANDOM_PER_CONFIG, "longest": LONGEST, "decoded": decoded},
                         **csv_cases.digest(values, results)))
    model = {"seed": SEED, "named": named, "random": sets}
    with open(os.path.join(HERE, "csv_model_vectors.json"), "w", encoding="utf-8") as f:
        json.dump(model, f, ensure_ascii=True, separators=(",", ":"))
    csv_cases.load_fixtures.cache_clear()
    csv_cases.all_cases.cache_clear()
    compared, trips = check_second_opinions(csv_cases.all_cases())
    print("unit cases %d, named %d, random decoded %r, compared with CPython %d, round trips %d" % (len(unit["cases"]), len(named), counts, compared, trips))
    for fn in ("csv_unittest_vectors.json", "csv_model_vectors.json"):
        print(fn, os.path.getsize(os.path.join(HERE, fn)))


if __name__ == "__main__":
    main()
