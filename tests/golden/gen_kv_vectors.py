"""Writes tests/golden/kv_unittest_vectors.json and tests/golden/kv_model_vectors.json (run by hand: python tests/golden/gen_kv_vectors.py).

kv_unittest_vectors.json: the six cases of the reference's plugins/processor/split/keyvalue/key_value_splitter_test.go read as DATA --
the configuration, the source value and the pairs the test states (the quote case for all three quote lengths) -- with the pairs in
the order the Go appends them.  The writer asserts that tests/helpers/kv_model.py gives exactly the stated pairs.

kv_model_vectors.json: configurations, values and the model's recorded results (no program text): named cases aimed at every branch
of concatQuotePair / getNearestQuote / getValue, and 2000 seeded random values per configuration over the nine-symbol alphabet
a, b, space, backslash, '"', "'", the delimiter, the separator, the quote.  The writer asserts the panic caps: none with an empty or
one-byte quote, at most 10 % with a longer one.  Compact form (README_kv.md): a named result is "P" (the reference panics) or the rows'
integers joined by blanks; a random set is its seed (helpers/kv_cases.random_values makes the values) with digests of the values and of
the recorded results (helpers/kv_cases.digest)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from helpers import kv_cases, kv_model  # noqa: E402

RANDOM_PER_CONFIG, LONGEST = 2000, 24
SEED = 20260714


def result_text(config, value):
    status, pairs = kv_model.split(config, value)
    if status == "panic":
        return "P"
    return " ".join(str(x) for _, _, _, spans in pairs for x in spans)


# ---------------------------------------------------------------------------------------------- the reference's unit test, as data
def quoted(value, quote):
    return quote + value + quote


def unittest_cases():
    base = {"KeepSource": True, "SourceKey": "content"}
    cases = [
        ("TestSplit", dict(base), "class:main\tuserid:123456\tmethod:get\tkey with empty:xxxxx\tmessage:\"wrong user\"", 6,
         [("class", "main"), ("userid", "123456"), ("method", "get"), ("key with empty", "xxxxx"), ("message", "\"wrong user\"")]),
        ("TestSplitWithEmptyKey", dict(base, EmptyKeyPrefix="MyEmptyPrefix_"),
         "class:main\tuserid:123456\tmethod:get\t:empty again\tmessage:\"wrong user\"\t:100 empty key\n\nhello", 7,
         [("class", "main"), ("userid", "123456"), ("method", "get"), ("message", "\"wrong user\""), ("MyEmptyPrefix_0", "empty again"),
          ("MyEmptyPrefix_1", "100 empty key\n\nhello")]),
        ("TestSplitWithoutSeparator", dict(base, NoSeparatorKeyPrefix="MySeparatorPrefix_"),
         "class:main\tuserid:123456\tmethod:get\tmessage:\"wrong user\"\t100 empty key\n\nhello\tno separator again", 7,
         [("class", "main"), ("userid", "123456"), ("method", "get"), ("message", "\"wrong user\""), ("MySeparatorPrefix_0", "100 empty key\n\nhello"),
          ("MySeparatorPrefix_1", "no separator again")]),
        ("TestSplitWithMultiCharacterDelimiter", dict(base, NoSeparatorKeyPrefix="MySeparatorPrefix_", Delimiter="#?#"),
         "class:main#?#userid:123456#?#method:get#?#message:\"wrong user\"#?#100 empty key\n\nhello#?#no separator again", 7,
         [("class", "main"), ("userid", "123456"), ("method", "get"), ("message", "\"wrong user\""), ("MySeparatorPrefix_0", "100 empty key\n\nhello"),
          ("MySeparatorPrefix_1", "no separator again")]),
        ("TestSplitWithChineseCharacter",
         dict(base, SourceKey="中文content", NoSeparatorKeyPrefix="MySeparatorPrefix_", Delimiter="#D中文分隔#", Separator="#S中文分隔#"),
         "class#S中文分隔#main#D中文分隔#userid#S中文分隔#123456#D中文分隔#method#S中文分隔#get#D中文分隔#message#S中文分隔#\"wrong user\"#D中文分隔#100 没有key\n\nhello#D中文分隔#没有分隔符again",
         7, [("class", "main"), ("userid", "123456"), ("method", "get"), ("message", "\"wrong user\""), ("MySeparatorPrefix_0", "100 没有key\n\nhello"),
             ("MySeparatorPrefix_1", "没有分隔符again")]),
    ]
    for quote in ("\"", "\"\"", "\"\"\""):
        value = ("a1:" + quoted("b \\\" c", quote) + " a2:" + quoted("b \\\" \\\" c \\\\", quote) + " class:main userid:123456" + " half_quote:\" " +
                 quoted("多  分  隔 ", quote) + " method:get " + quoted("中文", quote) + " chinesekey:" + quoted("中文", quote) + " " + quoted("", quote) +
                 " nullval:" + quoted("", quote) + " http_user_agent:" + quoted("User Agent", quote) + " message:" + quoted("wrong user", quote) +
                 " 100 empty key\n\nhello " + quoted("no separator again", quote) + " \"123")
        p = "MySeparatorPrefix_"
        cases.append(("TestSplitWithQuote/%d" % len(quote), dict(base, NoSeparatorKeyPrefix=p, Delimiter=" ", Quote=quote), value, 19,
                      [("a1", "b \\\" c"), ("a2", "b \\\" \\\" c \\\\"), ("class", "main"), ("userid", "123456"), ("method", "get"),
                       ("http_user_agent", "User Agent"), ("message", "wrong user"), ("nullval", ""), ("chinesekey", "中文"), ("half_quote", "\""),
                       (p + "0", "多  分  隔 "), (p + "1", "中文"), (p + "2", ""), (p + "3", "100"), (p + "4", "empty"), (p + "5", "key\n\nhello"),
                       (p + "6", "no separator again"), (p + "7", "\"123")]))
    out = []
    for name, config, value, contents, stated in cases:
        got, alarms = kv_model.process_log(config, [[config["SourceKey"], value]])
        appended = [[k.decode("utf-8"), v.decode("utf-8")] for k, v in got[1:]]
        assert len(got) == contents, (name, len(got))
        assert sorted(map(tuple, appended)) == sorted(stated), (name, appended)  # exactly the stated pairs
        out.append({"case": name, "config": config, "value": value, "contents": contents, "stated": [list(p) for p in stated], "pairs": appended,
                    "rows": result_text(config, value)})
    return out


# ---------------------------------------------------------------------------------------------- named model cases
LOGFMT = {"Delimiter": " ", "Separator": "=", "Quote": "\""}
WIDE = {"Delimiter": "#?#", "Separator": ": ", "Quote": "'"}
Q2 = {"Delimiter": " ", "Separator": "=", "Quote": "\"\""}
Q2S2 = {"Delimiter": ",", "Separator": "=>", "Quote": "''"}
NAMED = [
    # concatQuotePair's four conditions
    ("no_delimiter_no_extension", LOGFMT, 'a="x y'),
    ("pair_ends_with_quote", LOGFMT, 'a="x" b=2'),
    ("separator_quote_above_zero", LOGFMT, 'a="x y" b=2'),
    ("separator_quote_at_zero_is_not_above_zero", LOGFMT, '="x y" b=2'),
    ("separator_quote_at_zero_and_again_later", LOGFMT, '="x=" y" b=2'),
    ("prefix_quote_without_separator", LOGFMT, '"x y" b=2'),
    ("prefix_quote_separator_in_extension", LOGFMT, '"x y=z" b=2'),
    ("neither_condition", LOGFMT, 'a=x" y" b=2'),
    ("separator_quote_straddles_the_pair_end", {"Delimiter": "\"", "Separator": "=", "Quote": "\""}, 'a="x" b'),
    # getNearestQuote, one-byte quote
    ("escaped_once", LOGFMT, 'a="x \\" y" b=2'),
    ("escaped_twice_in_a_row", LOGFMT, 'a="x \\" \\" y" b=2'),
    ("escaped_back_to_back", LOGFMT, 'a="x \\"" y" b=2'),
    ("escaped_without_the_space", LOGFMT, 'a="x y\\" z" b=2'),
    ("escape_begins_before_the_search", LOGFMT, 'a="x \\" b=2'),
    ("escape_as_last_bytes", LOGFMT, 'a="x y \\"'),
    ("escape_then_one_byte", LOGFMT, 'a="x y \\"z'),
    ("escape_then_quote_as_last_byte", LOGFMT, 'a="x y \\""'),
    ("no_closing_quote", LOGFMT, 'a="x y z=1 c=2'),
    ("no_closing_quote_twice", LOGFMT, 'a="x y z=1 c=2 d=3'),
    ("no_closing_quote_delimiter_last", LOGFMT, 'a="x '),
    ("no_closing_quote_two_bytes_left", LOGFMT, 'a="x yz'),
    ("no_closing_quote_one_byte_left", LOGFMT, 'a="x y'),
    ("no_closing_quote_after_an_escape", LOGFMT, 'a="x \\" y z=1 w=2'),
    ("bytes_behind_closing_quote_are_no_delimiter", LOGFMT, 'a="x y"zb=2 c=3'),
    ("closing_quote_is_last_byte", LOGFMT, 'a="x y"'),
    ("closing_quote_then_one_byte", LOGFMT, 'a="x y"z'),
    ("closing_quote_then_delimiter_ends", LOGFMT, 'a="x y" '),
    ("wide_delimiter_skipped_whatever", WIDE, "a: 'x#?#y'zzzb: 2#?#c: 3"),
    ("wide_delimiter_not_whole_behind_quote", WIDE, "a: 'x#?#y'zz"),
    ("wide_escape", WIDE, "a: 'x#?#y \\' z'#?#b: 2"),
    ("wide_separator_first_byte_only", WIDE, "a:b: c#?#d:e"),
    ("wide_delimiter_first_bytes_only", WIDE, "a: b#?c#?#d: e##?#"),
    # ends
    ("value_ends_with_delimiter", LOGFMT, "a=1 "),
    ("value_is_the_delimiter", LOGFMT, " "),
    ("value_is_two_delimiters", LOGFMT, "  "),
    ("empty_value", LOGFMT, ""),
    ("empty_value_no_quote", {}, ""),
    ("default_config", {}, "class:main\tuserid:123456\t:x\tnosep\t"),
    ("delimiter_equals_separator", {"Delimiter": ":", "Separator": ":", "Quote": "\""}, 'a:b:"c:d":e'),
    ("separator_in_quoted_value", LOGFMT, 'a="x=y z=w" b=2'),
    ("separator_equals_quote", {"Delimiter": " ", "Separator": "\"", "Quote": "\""}, 'a"b" c "d e" f'),
    ("quote_is_a_space", {"Delimiter": ",", "Separator": "=", "Quote": " "}, "a= x,y \\ z ,b=2"),
    ("quote_is_a_backslash", {"Delimiter": " ", "Separator": "=", "Quote": "\\"}, "a=\\x \\\\ y\\ b=2"),
    # getValue
    ("value_len_is_twice_the_quote", LOGFMT, 'a="" b=""x c="'),
    ("value_len_one_below", LOGFMT, 'a=" b=2'),
    ("no_separator_value_stripped", LOGFMT, '"x" "" " y'),
    ("long_quote_len_twice", Q2, 'a="""" b=2'),
    ("long_quote_len_one_below", Q2, 'a=""" b=2'),
    ("long_quote_overlapping_ends", {"Delimiter": " ", "Separator": "=", "Quote": "\"\"\""}, 'a=""""" b=2'),
    # quotes of two or more bytes
    ("long_quote_closed", Q2, 'a=""x y"" b=2'),
    ("long_quote_prefix", Q2, '""x y"" b=2'),
    ("long_quote_no_closing_panics", Q2, 'a=""x '),
    ("long_quote_no_closing_fits", Q2, 'a=""x yz'),
    ("long_quote_no_closing_goes_on", Q2, 'a=""x yz c=1 d=2'),
    ("long_quote_half_quote_behind", Q2, 'a=""x y" b=2'),
    ("long_quote_wide_separator_closed_fits", Q2S2, "a=>''x,y'',b=>2"),
    ("long_quote_wide_separator_closed_panics", Q2S2, "a=>''x,y''"),
    ("long_quote_wide_separator_separator_behind_quote", Q2S2, "''x,y''=>,b=>2"),
    ("long_quote_wide_separator_none_fits", Q2S2, "a=>''x,yzw"),
    ("long_quote_wide_separator_none_panics", Q2S2, "a=>''x,y"),
]

RANDOM_CONFIGS = [
    ("default", {}),
    ("logfmt", LOGFMT),
    ("wide_needles_one_byte_quote", WIDE),
    ("two_byte_quote", Q2),
    ("two_byte_quote_two_byte_separator", Q2S2),
]


def main():
    unit = {"source": "plugins/processor/split/keyvalue/key_value_splitter_test.go, read as data", "cases": unittest_cases()}
    with open(os.path.join(HERE, "kv_unittest_vectors.json"), "w", encoding="utf-8") as f:
        json.dump(unit, f, ensure_ascii=False, separators=(",", ":"))
    named = []
    for name, config, value in NAMED:
        named.append({"name": name, "config": config, "value": value, "rows": result_text(config, value.encode("utf-8"))})
    assert len({e["name"] for e in named}) == len(named)
    assert sum(1 for e in named if e["rows"] == "P") >= 3
    sets, counts = [], {}
    for k, (name, config) in enumerate(RANDOM_CONFIGS):
        values = kv_cases.random_values(config, SEED + k, RANDOM_PER_CONFIG, LONGEST)
        rows = [result_text(config, v) for v in values]
        panics = rows.count("P")
        if len(kv_model.init(config)["Quote"]) <= 1:
            assert panics == 0, (name, panics)
        else:
            assert 0 < panics <= RANDOM_PER_CONFIG // 10, (name, panics)
        counts[name] = panics
        sets.append(dict({"name": name, "config": config, "seed": SEED + k, "n": RANDOM_PER_CONFIG, "longest": LONGEST, "panics": panics},
                         **kv_cases.digest(values, rows)))
    model = {"seed": SEED, "named": named, "random": sets}
    with open(os.path.join(HERE, "kv_model_vectors.json"), "w", encoding="utf-8") as f:
        json.dump(model, f, ensure_ascii=False, separators=(",", ":"))
    print("unit cases %d, named %d (panic %d), random panics %r" % (len(unit["cases"]), len(named), sum(1 for e in named if e["rows"] == "P"), counts))
    for fn in ("kv_unittest_vectors.json", "kv_model_vectors.json"):
        print(fn, os.path.getsize(os.path.join(HERE, fn)))


if __name__ == "__main__":
    main()
