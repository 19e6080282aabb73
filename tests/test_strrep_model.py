"""tests/helpers/strrep_model.py, the reference of every strrep test, held to what it models: the reference's own unit-test cases read as
data (tests/golden/strrep_unittest_vectors.json), the rules of include/strrep/lc_strrep.h one by one, and an independent witness for the
unquote: on the subset of escapes where Python's own literal rules coincide with Go's, ast.literal_eval of the wrapped value.  A model
of Go's code, not Go: tests/golden/README_strrep.md."""
import ast
import random

from helpers import strrep_cases as sc
from helpers import strrep_model as model

UNQ = sc.UNQUOTE


def test_the_references_unit_test_cases():
    doc = sc.load_vectors()
    assert [e["case"].split("/")[-1] for e in doc["cases"]] == ["TestProcessorConstReplaceWork", "unquote1", "unquote2", "unquote3", "const"]
    for e in doc["cases"]:
        assert model.init_error(e["config"]) is None
        got, alarms, counters = model.process_logs(e["config"], [e["log"]])
        assert [list(kv) for kv in got[0]] == e["contents"] and alarms == [], e["case"]
        assert counters["values"] == counters["changed"] == counters["replace_count"] == 1
    dest = doc["dest_key"]
    assert "stays with the Go plugin" in model.init_error(dest["config"])
    as_const = dict(dest["config"], Method="const", Match="16", ReplaceString="*/24")  # the same shape through a method served here
    assert [list(kv) for kv in model.process_logs(as_const, [dest["log"]])[0][0]] == dest["stated"]
    messages = [model.init_error(e["config"]) for e in doc["init_errors"]]
    assert messages == ["stays with the Go plugin", "no source key error", "no source key error", "no source key error"]
    assert model.init_error({"SourceKey": "k"}) == "no method error" and model.init_error({"SourceKey": "k", "Method": "const"}) == "no match error"
    assert len(doc["refused_at_create"]) == 8
    assert all("stays with the Go plugin" in model.init_error(e["config"]) for e in doc["refused_at_create"])


def test_const_rules():
    assert model.apply(sc.const("aa", "b"), b"aaaaa") == (model.CHANGED, b"bba")
    assert model.apply(sc.const("aa", "b"), b"abab") == (0, None)
    assert model.apply(sc.const("ab", ""), b"abab") == (model.CHANGED, b"")
    assert model.apply(sc.const("ab", "ab"), b"xab") == (model.CHANGED, b"xab")
    assert model.apply(sc.const("aba", "-"), b"ababababa") == (model.CHANGED, b"-b-ba")
    assert model.init_error(sc.const("m" * 33)) and model.init_error(sc.const("m", "r" * 257)) and not model.init_error(sc.const("m" * 32, "r" * 256))


def test_unquote_rules():
    def u(v):
        return model.apply(UNQ, v)
    ok, err = model.CHANGED, (model.ERROR, None)
    assert u(b'"') == err and u(b'""') == (ok, b"") and u(b"") == (0, None) and u(b"plain") == (0, None)
    assert u(b'say "hi"') == (0, None)  # form B: every quote goes to \x22 and back
    assert u(b'"a"b"') == err and u(b"a\\") == err and u(b'"a\\"') == err and u(b"a\\\\\\") == err and u(b"a\\\\") == (ok, b"a\\")
    assert u(b"a\nb") == err and u(b'"a\nb"') == err and u(b"a\\nb") == (ok, b"a\nb")
    assert u("啊é\U0001F600".encode()) == (0, None) and u(b'"\xe5\x95\x8a"') == (ok, "啊".encode())
    assert u(b"\xe4\xb8") == (ok, b"\xef\xbf\xbd" * 2)  # six bytes: the output can be three times the input
    assert u(b"\xc0\x80") == (ok, b"\xef\xbf\xbd" * 2) and u(b"\xe0\x80\x80") == (ok, b"\xef\xbf\xbd" * 3) and u(b"\xed\xa0\x80") == (ok, b"\xef\xbf\xbd" * 3)
    assert u(b"\xf4\x90\x80\x80") == (ok, b"\xef\xbf\xbd" * 4) and u(b"\xf4\x8f\xbf\xbf") == (0, None)
    assert u(b'"\\a\\b\\f\\n\\r\\t\\v\\\\\\""') == (ok, b'\a\b\f\n\r\t\v\\"') and u(b"\\'") == err
    assert u(b"\\xff") == (ok, b"\xff") and u(b"\\xFf\\x4a") == (ok, b"\xffJ") and u(b"\\x4") == err and u(b"\\x4g") == err
    assert u(b"\\101\\377") == (ok, b"A\xff") and u(b"\\400") == err and u(b"\\12") == err and u(b"\\128") == err
    assert u(b"\\u554a") == (ok, "啊".encode()) and u(b"\\U0001f600") == (ok, "\U0001F600".encode()) and u(b"\\u0041") == (ok, b"A")
    assert u(b"\\ud800") == err and u(b"\\udfff") == err and u(b"\\U00110000") == err and u(b"\\U0010FFFF") == (ok, "\U0010FFFF".encode())
    assert u(b"\\u55") == err and u(b"\\q") == err and u(b"\\") == err
    assert u(b'a\\"b') == (ok, b"a\\x22b")  # the replacement happens BEFORE the decode: a literal backslash
    assert u(b'\\\\"') == (ok, b'\\"') and u(b'"a\\"b"') == (ok, b'a"b')
    assert model.alarm_text(UNQ, b"a\\") == b"error:invalid syntax\tmethod:unquote\tsource_key:content\tcontent:a\\\t"


# ---------------------------------------------------------------------------------------------- the witness
def _witness_values(seed, n):
    """values built ONLY from the subset on which Python's bytes-literal and str-literal rules coincide with Go's"""
    rnd = random.Random(seed)
    plain = [bytes([b]) for b in range(0x20, 0x7F) if b not in (0x22, 0x5C, 0x27)] + [b"'", b"\t"]

    def rune():
        while True:
            r = rnd.choice((rnd.randrange(0x80), rnd.randrange(0x800), rnd.randrange(0x10000), rnd.randrange(0x110000)))
            if not 0xD800 <= r <= 0xDFFF:
                return r

    def piece():
        k = rnd.randrange(9)
        if k < 3:
            return rnd.choice(plain)
        if k == 3:
            return b"\\" + rnd.choice(b"abfnrtv\\").to_bytes(1, "little")
        if k == 4:
            return b"\\x%02x" % rnd.randrange(0x80) if rnd.random() < .5 else b"\\x%02X" % rnd.randrange(0x80)
        if k == 5:
            return b"\\%03o" % rnd.randrange(0o200)
        if k == 6:
            r = rune()
            return b"\\u%04x" % r if r < 0x10000 else b"\\U%08x" % r
        if k == 7:
            return b"\\U%08X" % rune()
        while True:  # well-formed UTF-8, raw
            r = rune()
            if r >= 0x80:
                return chr(r).encode("utf-8")

    return [b"".join(piece() for _ in range(rnd.randrange(0, 40))) for _ in range(n)]


def test_pythons_own_literals_agree_on_the_common_subset():
    values = _witness_values(20260, 4000)
    checked = 0
    for k, body in enumerate(values):
        value = b'"' + body + b'"' if k % 2 else body  # form A and form B (no raw quote in the subset)
        want = ast.literal_eval('"' + body.decode("utf-8") + '"').encode("utf-8")
        flags, out = model.apply(UNQ, value)
        assert not flags & model.ERROR, value
        assert (out if flags & model.CHANGED else value) == want, value
        checked += 1
    assert checked == len(values) == 4000
    assert sum(1 for v in values if b"\\U" in v) > 500 and sum(1 for v in values if b"\\x" in v) > 500
