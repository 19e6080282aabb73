"""tests/helpers/jsonl_model.py, the Python model of the JSON-lines serializer that the host and GPU tests compare with.  rapidjson is
not available to the tests, so the reference's serializer is not compiled: the model is PINNED on the rules of the issue
(JsonSerializer.cpp:30-84, Writer::WriteString), and held here to one independent witness that shares no code with it -- CPython's
json.dumps on the latin-1 decoding, hex digits of \\u00xx upper-cased -- and to json.loads of every record.  The cut at the first NUL and
the order of the tags rest on reading the reference's source alone.  tests/golden/jsonl_vectors.json is the model's output
(README_jsonl.md).  CPU only."""
import json
import os
import random
import re

from helpers import jsonl_cases as jc
from helpers import jsonl_model as jm

REACTIVE = [0x22, 0x5C, 0x01, 0x08, 0x09, 0x0A, 0x0C, 0x0D, 0x1F, 0x2F, 0x7F, 0x80, 0xFF]


def witness(s):
    """CPython's escape of a string without a NUL, bytewise"""
    text = json.dumps(s.decode("latin-1"), ensure_ascii=False)
    text = re.sub(r"\\u00([0-9a-f]{2})", lambda m: "\\u00" + m.group(1).upper(), text)
    return text.encode("latin-1")


def test_the_escape_equals_cpython_s_on_every_byte_and_on_random_strings():
    for c in range(1, 256):
        assert jm.string(bytes([c])) == witness(bytes([c])), c
    assert jm.string(b"\x1f") == b'"\\u001F"' and jm.string(b"\x0b") == b'"\\u000B"' and jm.string(b"/\x7f\x80\xff") == b'"/\x7f\x80\xff"'
    rng = random.Random(41)
    for _ in range(20000):
        n = rng.choice([0, 1, 2, 5, 16, 17, 40, 100])
        s = bytes(rng.choice(REACTIVE) if rng.random() < 0.4 else rng.randrange(1, 256) for _ in range(n))
        assert jm.string(s) == witness(s), s


def test_the_nul_cut():
    assert jm.string(b"\0") == b'""' and jm.string(b'ab\0"\\\x01') == b'"ab"' and jm.string(b"ab\0cd\0") == b'"ab"'
    assert jm.record(5, [(b"k\0ey", b"v\0al")], [(b"t\0a", b"x\0y")]) == b'{"t":"x","__time__":5,"k":"v"}\n'


def test_the_reference_s_unit_test_expectation():
    """JsonSerializerUnittest's log case: the four tags, time 1234567890, key -> value; an empty event beside it writes nothing; only
    empty events give no bytes"""
    tags = [(b"__topic__", b"topic"), (b"__source__", b"source"), (b"__machine_uuid__", b"machine_uuid"), (b"__pack_id__", b"pack_id")]
    want = (b'{"__machine_uuid__":"machine_uuid","__pack_id__":"pack_id","__source__":"source","__topic__":"topic",'
            b'"__time__":1234567890,"key":"value"}\n')
    assert jm.records([(1234567890, [(b"key", b"value")])], tags) == want
    assert jm.records([(1234567890, [(b"key", b"value")]), (1234567890, [])], tags) == want
    assert jm.records([(1234567890, []), (1, [])], tags) == b""
    assert jm.head() == b'{"__time__":' and len(jm.head()) == 12


def test_the_order_of_the_tags():
    tags = [(b"ab", b"2"), (b"\x80", b"5"), (b"a", b"1"), (b"b", b"4"), (b"a\xc3\xa9", b"3"), (b"Z", b"0")]
    assert jm.head(tags) == b'{"Z":"0","a":"1","ab":"2","a\xc3\xa9":"3","b":"4","\x80":"5","__time__":'


def _parsed(data):
    return [json.loads(line.decode("latin-1"), object_pairs_hook=lambda pairs: [list(p) for p in pairs]) for line in data.split(b"\n")[:-1]]


def _check_records(data, tags, rows, spec):
    """json.loads of every record: the tags in the map's order, the time, the item keys and values cut at NUL"""
    keys, matched, unmatched = spec
    want = []
    for line, status, caps, t in rows:
        items = matched if status == 1 else unmatched
        if not items:
            continue
        pairs = [[jm.cut(k).decode("latin-1"), jm.cut(v).decode("latin-1")] for k, v in sorted(tags)] + [["__time__", t]]
        for k, s in items:
            value = line if s == 0 else (line[caps[2 * s - 2]:caps[2 * s - 1]] if caps[2 * s - 2] >= 0 else b"")
            pairs.append([jm.cut(keys[k]).decode("latin-1"), jm.cut(value).decode("latin-1")])
        want.append(pairs)
    assert _parsed(data) == want


def build_vectors():
    vectors = []
    for config, group in jc.vector_inputs():
        keys, matched, unmatched, rows, tags = jc.engine_batch(config, group)
        data = jc.model_batch(keys, matched, unmatched, rows, tags)[1]
        _check_records(data, tags, rows, (keys, matched, unmatched))
        vectors.append({"kind": "group", "config": config, "group": group, "bytes": data.hex()})
    for keys, matched, unmatched, rows, tags in jc.engine_vectors():
        data = jc.model_batch(keys, matched, unmatched, rows, tags)[1]
        _check_records(data, tags, rows, (keys, matched, unmatched))
        vectors.append({"kind": "engine", "keys": [k.hex() for k in keys], "matched": [list(x) for x in matched], "unmatched": [list(x) for x in unmatched],
                        "rows": [[line.hex(), st, list(caps), t] for line, st, caps, t in rows], "tags": [[k.hex(), v.hex()] for k, v in tags],
                        "bytes": data.hex()})
    return vectors


def test_the_golden_file_is_the_model_s_output_and_every_record_parses_back():
    vectors = build_vectors()
    assert len(vectors) == 26 + 2 and os.path.getsize(jc.GOLDEN) < 400 << 10
    assert jc.load_golden() == json.loads(json.dumps(vectors))
    lines = [e["contents"]["content"] for v in vectors if v["kind"] == "group" for e in v["group"]["events"]]
    for needle in ('"', "\\", "\x00", "\x7f", "\t", "\x01", "\x1f"):
        assert any(needle in line for line in lines), repr(needle)
    assert {len(v["group"].get("tags", {})) for v in vectors if v["kind"] == "group"} == {0, 1, 5}
    times = {e["timestamp"] for v in vectors if v["kind"] == "group" for e in v["group"]["events"]}
    assert {0, 9, 10, (1 << 32) - 1, 10 ** 9} <= times


if __name__ == "__main__":   # writes the golden file: python tests/test_jsonl_model.py (from the repository's root, tests/ on the path)
    with open(jc.GOLDEN, "w", encoding="utf-8") as f:
        f.write(json.dumps(build_vectors(), ensure_ascii=True, separators=(",", ":")) + "\n")
