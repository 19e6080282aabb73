"""What the JSON parser's test files share: the two fixture files read into byte strings, the seeded generator of documents and
one-byte mutations, and the comparison of what a walk reported (the host routine's or the kernel's) with tests/helpers/json_model.py."""
import json
import os
import random

import numpy as np

from helpers import json_model as jm

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
MEMBER = np.dtype([("kb", "<u4"), ("ke", "<u4"), ("vb", "<u4"), ("ve", "<u4"), ("type", "u1"), ("reserved", "u1", (3,))])
assert MEMBER.itemsize == 20
ESCAPED = 0x80000000
TYPE_NAMES = ["STRING", "INT", "DOUBLE", "TRUE", "FALSE", "NULL", "OBJECT", "ARRAY"]
STATUS_NAMES = {"fail": jm.FAIL, "ok": jm.OK, "empty": jm.EMPTY}


def expand(text):
    """a fixture text -> bytes: each character one byte; a list of [text, count] parts is repeated and joined"""
    if isinstance(text, list):
        return b"".join(expand(t) * k for t, k in text)
    return text.encode("latin-1")


def contract_cases():
    with open(os.path.join(GOLDEN, "json_contract_vectors.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


def unittest_doc():
    with open(os.path.join(GOLDEN, "json_unittest_vectors.json"), encoding="utf-8") as f:
        return json.load(f)


def rendered(line, members):
    return [[k, TYPE_NAMES[m.type], v] for m in members for k, v in [jm.render(line, m)]]


# ------------------------------------------------------------------------------------------------ generated documents
_WORDS = ["a", "b", "msg", "level", "time", "content", "k0", "user_id", "ts", "é", "键", "😀", "", "x y", "long_key_" * 5]
_BLANKS = ["", "", "", " ", "  ", "\t", "\n", "\r\n"]


def _gen_string(rng):
    parts = []
    for _ in range(rng.choice([0, 1, 1, 2, 3, 6, 12])):
        r = rng.random()
        if r < 0.55:
            parts.append("".join(rng.choice("abcdefghij XYZ0123456789-_./:") for _ in range(rng.randrange(1, 9))))
        elif r < 0.65:
            parts.append(rng.choice(['\\"', "\\\\", "\\/", "\\b", "\\f", "\\n", "\\r", "\\t"]))
        elif r < 0.75:
            parts.append("\\u%04x" % rng.choice([0, 0x41, 0xE9, 0x7FF, 0x800, 0x20AC, 0xD7FF, 0xE000, 0xFFFF, rng.randrange(0xD800)]))
        elif r < 0.8:
            c = rng.randrange(0x10000, 0x110000) - 0x10000
            parts.append(("\\u%04X\\u%04X" if rng.random() < 0.5 else "\\u%04x\\u%04x") % (0xD800 + (c >> 10), 0xDC00 + (c & 0x3FF)))
        else:
            parts.append(rng.choice(["é", "ß", "€", "键", "😀", "߿", "ࠀ", "￿", "\U00010000", "\U0010ffff", "\x7f"]))
    return '"' + "".join(parts) + '"'


def _gen_number(rng):
    r = rng.random()
    if r < 0.4:
        return str(rng.choice([0, 1, -1, 7, 42, -300, 10 ** rng.randrange(1, 19), -10 ** rng.randrange(1, 19), rng.randrange(-10 ** 6, 10 ** 6)]))
    if r < 0.5:
        return rng.choice(["18446744073709551615", "18446744073709551616", "-9223372036854775808", "-9223372036854775809", "-0", "0",
                           "9223372036854775807", "9223372036854775808", "99999999999999999999", "123456789012345678901234567890"])
    s = ("-" if rng.random() < 0.3 else "") + str(rng.randrange(0, 10 ** rng.randrange(1, 8)))
    if rng.random() < 0.7:
        s += "." + "".join(rng.choice("0123456789") for _ in range(rng.randrange(1, 9)))
    if rng.random() < 0.4:
        s += rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randrange(0, 30))
    return s


def _gen_value(rng, depth):
    r = rng.random()
    if r < 0.35:
        return _gen_string(rng)
    if r < 0.6:
        return _gen_number(rng)
    if r < 0.75:
        return rng.choice(["true", "false", "null"])
    if depth >= 5 or r < 0.8:
        return rng.choice(["{}", "[]", "[ ]", "{ }"])
    b = lambda: rng.choice(_BLANKS)       # noqa: E731
    if r < 0.9:
        return "[" + ",".join(b() + _gen_value(rng, depth + 1) + b() for _ in range(rng.randrange(1, 5))) + "]"
    return _gen_object(rng, depth + 1)


def _gen_object(rng, depth, members=None):
    b = lambda: rng.choice(_BLANKS)       # noqa: E731
    n = rng.randrange(0, 7) if members is None else members
    out = []
    for _ in range(n):
        key = _gen_string(rng) if rng.random() < 0.25 else json.dumps(rng.choice(_WORDS), ensure_ascii=rng.random() < 0.5)
        out.append(b() + key + b() + ":" + b() + _gen_value(rng, depth) + b())
    return "{" + (",".join(out) if out else b()) + "}"


def gen_document(rng):
    r = rng.random()
    if r < 0.03:      # what CPython takes and the contract does not
        return rng.choice(['{"a":NaN}', '{"a":[Infinity]}', '{"a":-Infinity}', '{"a":"\\ud800"}', '{"\\udc00":1}', '{"a":["\\ud83dx"]}', "[1,2]", '"s"',
                           "12", "true", "null", ' {"a":1} ', "[]"]).encode("utf-8")
    members = rng.choice([None, None, None, 31, 32, 33, 40]) if r < 0.1 else None
    return (rng.choice(_BLANKS) + _gen_object(rng, 1, members) + rng.choice(_BLANKS)).encode("utf-8")


_MUTANT_BYTES = b'"\\{}[]:,0123456789-+.eEtfnu \t\n\x00\x1f\x7f\x80\xbf\xc0\xc2\xe0\xed\xf0\xf4\xf5\xffaxDdCc'


def mutate(rng, doc):
    """one byte replaced, inserted or deleted"""
    if not doc:
        return bytes([rng.choice(_MUTANT_BYTES)])
    at = rng.randrange(len(doc))
    r = rng.random()
    if r < 0.5:
        return doc[:at] + bytes([rng.choice(_MUTANT_BYTES)]) + doc[at + 1:]
    if r < 0.75:
        return doc[:at] + bytes([rng.choice(_MUTANT_BYTES)]) + doc[at:]
    return doc[:at] + doc[at + 1:]


def generated_set(seed, count):
    """count documents: a valid one, then two one-byte mutations of it, and so on"""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        doc = gen_document(rng)
        out.append(doc)
        out.append(mutate(rng, doc))
        out.append(mutate(rng, doc))
    return out[:count]


def pack(lines):
    off = np.zeros(len(lines) + 1, np.int64)
    if lines:
        off[1:] = np.cumsum([len(ln) for ln in lines])
    data = np.frombuffer(b"".join(lines) + b"\0", np.uint8).copy()
    return data, off


# ------------------------------------------------------------------------------------------------ a walk's report against the model
def same_as_model(line, status, nmembers, errpos, records, shadow, W, want=None):
    """records: MEMBER[W] of the line; shadow: the line's own shadow bytes (len(line)).  Returns None, or what differs."""
    st, members, err = want if want is not None else jm.walk(line)
    if int(status) != st:
        return "status %d, the model says %d (error offset %d / %d)" % (status, st, errpos, err)
    if st == jm.FAIL and int(errpos) != err:
        return "error offset %d, the model says %d" % (errpos, err)
    if st != jm.OK:
        return None if int(nmembers) == 0 else "members on a line that is not OK"
    if int(nmembers) != len(members):
        return "%d members, the model says %d" % (nmembers, len(members))
    for k, m in enumerate(members[:W]):
        r = records[k]
        got = (int(r["kb"]) & ~ESCAPED, int(r["ke"]), bool(int(r["kb"]) & ESCAPED), int(r["vb"]) & ~ESCAPED, int(r["ve"]),
               bool(int(r["vb"]) & ESCAPED), int(r["type"]))
        if got != m.record():
            return "member %d: %r, the model says %r" % (k, got, m.record())
        if m.key_text is not None and bytes(shadow[m.kb:m.kb + len(m.key_text)]) != m.key_text:
            return "member %d: unescaped key %r, the model says %r" % (k, bytes(shadow[m.kb:m.kb + len(m.key_text)]), m.key_text)
        if m.val_text is not None and bytes(shadow[m.vb:m.vb + len(m.val_text)]) != m.val_text:
            return "member %d: unescaped value %r, the model says %r" % (k, bytes(shadow[m.vb:m.vb + len(m.val_text)]), m.val_text)
    return None
