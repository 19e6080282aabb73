"""The MODEL of the JSON-lines encoder (include/jsonl/lc_jsonl.h), pure Python over bytes, written from the rules of the reference's
JsonEventGroupSerializer (JsonSerializer.cpp:30-84) and rapidjson's Writer::WriteString with default flags -- not from csrc/jsonl_vm.hpp.
tests/test_jsonl_model.py holds it to CPython's json.dumps (the escape) and json.loads (every record).  The cut at the first NUL and the
order of the tags rest on reading the reference's source alone."""

import re

_REACTIVE = re.compile(rb'[\x00-\x1f"\\]')
_SHORT = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x09: b"\\t", 0x0A: b"\\n", 0x0C: b"\\f", 0x0D: b"\\r"}


def cut(s):
    """a string as the const Ch* overloads see it: up to its first NUL"""
    at = s.find(b"\0")
    return s if at < 0 else s[:at]


def escape(s):
    """Writer::WriteString's bytes between the quotes, for a string without a NUL (callers cut first)"""
    def one(m):
        c = m.group()[0]
        return _SHORT[c] if c in _SHORT else b"\\u00%02X" % c
    return _REACTIVE.sub(one, s)


def string(s):
    return b'"' + escape(cut(s)) + b'"'


def head(tags=()):
    """tags: [(key, value)] with distinct keys, any order -> {"k":"v",...,"__time__":   (std::map's order: bytewise, unsigned, shorter first)"""
    tags = sorted(tags, key=lambda kv: kv[0])
    assert len({k for k, _ in tags}) == len(tags)
    return b"{" + b"".join(string(k) + b":" + string(v) + b"," for k, v in tags) + b'"__time__":'


def record(time, contents, tags=()):
    """one log event: time (seconds, written in decimal), contents [(key, value)] in the event's order; no content: no record"""
    if not contents:
        return b""
    return head(tags) + b"%d" % time + b"".join(b"," + string(k) + b":" + string(v) for k, v in contents) + b"}\n"


def records(events, tags=()):
    """events: [(time, [(key, value)])] -> the bytes of the group"""
    return b"".join(record(t, contents, tags) for t, contents in events)
