"""tests/helpers/codec_model.py, the Python model of the field codecs (include/codec/lc_codec.h), against its independent witnesses:
CPython's base64, binascii and hashlib -- over the whole deterministic corpus of tests/helpers/codec_cases.py, which the host program
and the GPU tests run against the model.  The decode's error OFFSETS have no second witness: they rest on the rules the header restates
(tests/golden/README_codec.md)."""
import base64
import binascii
import hashlib
import re

from helpers import codec_cases as cc
from helpers import codec_model as model


def strip(value):
    return value.replace(b"\r", b"").replace(b"\n", b"")


def test_encode_equals_base64_b64encode_on_the_corpus():
    values = [v for _, v in cc.md5_cases()]
    assert {len(v) for v in values} >= set(range(41)) | {46, 47, 48, 49, 50, 510, 511, 512, 513, 514}
    for v in values:
        assert model.encode(v) == base64.b64encode(v)
        assert len(model.encode(v)) == 4 * ((len(v) + 2) // 3)
    assert model.encode(b"") == b"" and model.encode(b"123") == b"MTIz"


def test_md5_equals_hashlib_on_the_corpus():
    values = [v for _, v in cc.md5_cases()]
    assert {len(v) for v in values} >= {0, 55, 56, 57, 63, 64, 65, 119, 120, 121}
    for v in values:
        assert model.md5_hex(v) == hashlib.md5(v).hexdigest().encode()
    assert model.md5_hex(b"") == b"d41d8cd98f00b204e9800998ecf8427e" and model.md5_hex(b"123") == b"202cb962ac59075b964b07152d234b70"


def test_decode_inverts_encode():
    for _, v in cc.md5_cases():
        assert model.decode(model.encode(v)) == (v, None)
        assert model.decode(cc.mime(v)) == (v, None)
    assert model.decode(b"") == (b"", None) and model.decode(b"\r\n") == (b"", None)


def test_every_accepted_value_decodes_to_what_cpython_gives():
    accepted = [(v, model.decode(v)[0]) for _, v in cc.decode_cases() if model.decode(v)[1] is None]
    assert len(accepted) > 3000
    for v, out in accepted:
        assert base64.b64decode(strip(v), validate=True) == out, v
    assert model.decode(b"QR==") == model.decode(b"QQ==") == (b"A", None)  # non-strict: the unused bits are not checked


def in_a_listed_class(value):
    """tests/golden/README_codec.md: the classes of values the rules REJECT and CPython (after CR/LF removal, validate=True) accepts"""
    s = strip(value)
    m = re.fullmatch(rb"([A-Za-z0-9+/]*)(={1,2})", s)
    if not m:
        return False
    j, pads = len(m.group(1)) % 4, len(m.group(2))
    return j == 0 or (j == 3 and pads == 2)  # padding no quantum asked for / one `=` too many


def test_every_disagreement_on_rejected_values_falls_into_a_listed_class():
    rejected = [v for _, v in cc.decode_cases() if model.decode(v)[1] is not None]
    assert len(rejected) > 3000
    disagreements = 0
    for v in rejected:
        try:
            base64.b64decode(strip(v), validate=True)
        except (binascii.Error, ValueError):
            continue
        disagreements += 1
        assert in_a_listed_class(v), v
    assert model.decode(b"=") == (None, 0) and in_a_listed_class(b"=")  # a leading `=`: CPython 3.10 decodes it to b""
    assert disagreements < len(rejected) // 4


def test_the_error_rules_one_by_one():
    """the offsets, rule by rule, as include/codec/lc_codec.h states them"""
    d = model.decode
    assert d(b"QUJDR") == (None, 4)            # a lone trailing character: len - 1
    assert d(b"QUJDRE") == (None, 4)           # two and three without padding: len - (k % 4)
    assert d(b"QUJDREV") == (None, 4)
    assert d(b"QUJD\r\nRE\r\n") == (None, 8)   # ... counted in alphabet bytes only: len - 2, not the position of `R`
    assert d(b"QUJD=") == (None, 4)            # `=` at j = 0
    assert d(b"QUJDR=") == (None, 5)           # `=` at j = 1
    assert d(b"QUJDRE=") == (None, 7)          # a single `=` at j = 2 at the end: len
    assert d(b"QUJDRE=\r\n") == (None, 9)
    assert d(b"QUJDRE=x") == (None, 6)         # `=x` at j = 2: q - 1 (Go's quirk)
    assert d(b"QUJDRE=\r\nx") == (None, 8)     # ... q - 1 is the LF
    assert d(b"QUJDRE==x") == (None, 8)        # trailing garbage behind `==`
    assert d(b"QUJDREV=x") == (None, 8)        # ... and behind `=`
    assert d(b"QUJDREV==") == (None, 8)
    assert d(b"QUJD-REVG") == (None, 4)        # a non-alphabet byte
    assert d(b"QUJD_REVG-") == (None, 4)       # two errors: the first wins
    assert d(b"QUJDRE=\r\n=\r\n") == (b"ABCD", None) and d(b"QUJDREU=\n") == (b"ABCDE", None)
    assert model.error_text(4) == "illegal base64 data at input byte 4"
    assert d(b"test_value") == (None, 4)       # the reference's TestDecodeError value
