"""A Python model of the JSON parser: walk() is the per-line walk (csrc/json_vm.hpp jsonWalkLine) written the other way round -- an
index-driven descent over the bytes instead of one state per byte -- and process_event() is ProcessorParseJsonNative::ProcessEvent
(core/plugin/processor/ProcessorParseJsonNative.cpp:107-145) with the simdjson branch's rendering (:150-238).

The contract it implements is the one of tests/golden/README_json.md.  Expectations that come from here are THE MODEL'S, not the
reference's: tests/test_json_model.py holds the model to the hand-written vectors and to CPython's json module."""

FAIL, OK, EMPTY = 0, 1, 2
STRING, INT, DOUBLE, TRUE, FALSE, NULL, OBJECT, ARRAY = range(8)
MAX_DEPTH = 1024
RAW_LOG_KEY = "__raw_log__"

_BLANK = b" \t\n\r"
_SIMPLE = {0x22: 0x22, 0x5C: 0x5C, 0x2F: 0x2F, 0x62: 8, 0x66: 12, 0x6E: 10, 0x72: 13, 0x74: 9}
_HEX = b"0123456789abcdefABCDEF"
_DIGITS = b"0123456789"


class _Fail(Exception):
    def __init__(self, pos):
        self.pos = pos


class Member:
    """key / value spans relative to the line; *_text: the unescaped bytes where the source has escapes, else None"""
    __slots__ = ("kb", "ke", "key_text", "vb", "ve", "val_text", "type")

    def __init__(self, kb, ke, key_text, vb, ve, val_text, type_):
        self.kb, self.ke, self.key_text, self.vb, self.ve, self.val_text, self.type = kb, ke, key_text, vb, ve, val_text, type_

    def record(self):
        """what the routine reports: (key_begin, key_end, key_escaped, val_begin, val_end, val_escaped, type) with the ends of escaped
        texts at begin + the unescaped length"""
        ke = self.kb + len(self.key_text) if self.key_text is not None else self.ke
        ve = self.vb + len(self.val_text) if self.val_text is not None else self.ve
        return (self.kb, ke, self.key_text is not None, self.vb, ve, self.val_text is not None, self.type)


def _ws(b, i):
    n = len(b)
    while i < n and b[i] in _BLANK:
        i += 1
    return i


def _need(b, i):
    if i >= len(b):
        raise _Fail(len(b))
    return b[i]


def _hex4(b, j):
    v = 0
    for k in range(4):
        c = _need(b, j + k)
        if c not in _HEX:
            raise _Fail(j + k)
        v = v * 16 + int(chr(c), 16)
    return v, j + 4


def _utf8(b, j):
    """b[j] >= 0x80: one well-formed sequence (Unicode table 3-7) -> the index behind it"""
    c = b[j]
    if c < 0xC2 or c > 0xF4:
        raise _Fail(j)
    need = 1 if c < 0xE0 else 2 if c < 0xF0 else 3
    lo, hi = 0x80, 0xBF
    if c == 0xE0:
        lo = 0xA0
    elif c == 0xED:
        hi = 0x9F
    elif c == 0xF0:
        lo = 0x90
    elif c == 0xF4:
        hi = 0x8F
    for k in range(1, need + 1):
        x = _need(b, j + k)
        if x < lo or x > hi:
            raise _Fail(j + k)
        lo, hi = 0x80, 0xBF
    return j + need + 1


def _string(b, i):
    """b[i] is the opening quote -> (index of the closing quote, unescaped bytes or None)"""
    j = i + 1
    out = None
    while True:
        c = _need(b, j)
        if c == 0x22:
            return j, (bytes(out) if out is not None else None)
        if c == 0x5C:
            if out is None:
                out = bytearray(b[i + 1:j])
            e = _need(b, j + 1)
            if e in _SIMPLE:
                out.append(_SIMPLE[e])
                j += 2
            elif e == 0x75:
                cu, j = _hex4(b, j + 2)
                if 0xD800 <= cu <= 0xDBFF:
                    if _need(b, j) != 0x5C:
                        raise _Fail(j)
                    if _need(b, j + 1) != 0x75:
                        raise _Fail(j + 1)
                    low, j = _hex4(b, j + 2)
                    if not 0xDC00 <= low <= 0xDFFF:
                        raise _Fail(j - 1)
                    cu = 0x10000 + ((cu - 0xD800) << 10) + (low - 0xDC00)
                elif 0xDC00 <= cu <= 0xDFFF:
                    raise _Fail(j - 1)
                out += chr(cu).encode("utf-8")
            else:
                raise _Fail(j + 1)
        elif c < 0x20:
            raise _Fail(j)
        elif c < 0x80:
            if out is not None:
                out.append(c)
            j += 1
        else:
            k = _utf8(b, j)
            if out is not None:
                out += b[j:k]
            j = k


def _number(b, i):
    """-> (index behind the literal, is an integer literal)"""
    j = i
    if b[j] == 0x2D:
        j += 1
    c = _need(b, j)
    if c == 0x30:
        j += 1
    elif c in _DIGITS:
        while j < len(b) and b[j] in _DIGITS:
            j += 1
    else:
        raise _Fail(j)
    integer = True
    if j < len(b) and b[j] == 0x2E:
        integer = False
        j += 1
        if _need(b, j) not in _DIGITS:
            raise _Fail(j)
        while j < len(b) and b[j] in _DIGITS:
            j += 1
    if j < len(b) and b[j] in b"eE":
        integer = False
        j += 1
        if _need(b, j) in b"+-":
            j += 1
        if _need(b, j) not in _DIGITS:
            raise _Fail(j)
        while j < len(b) and b[j] in _DIGITS:
            j += 1
    return j, integer


def _members(b):
    n = len(b)
    i = _ws(b, 0)
    if _need(b, i) != 0x7B:
        raise _Fail(i)
    stack = [True]          # True: an object.  The root is level 1
    i += 1
    members = []
    state = "first"         # first: behind an opening bracket; next: behind a comma; after: behind a value
    key = (0, 0, None)
    vb = 0
    while stack:
        i = _ws(b, i)
        c = _need(b, i)
        closing = 0x7D if stack[-1] else 0x5D
        if state == "after":
            if c == 0x2C:
                i += 1
                state = "next"
                continue
            if c != closing:
                raise _Fail(i)
        if c == closing and state != "next":
            stack.pop()
            if len(stack) == 1:
                members.append(Member(key[0], key[1], key[2], vb, i + 1, None, OBJECT if c == 0x7D else ARRAY))
            i += 1
            state = "after"
            continue
        if stack[-1]:
            if c != 0x22:
                raise _Fail(i)
            e, text = _string(b, i)
            if len(stack) == 1:
                key = (i + 1, e, text)
            i = _ws(b, e + 1)
            if _need(b, i) != 0x3A:
                raise _Fail(i)
            i = _ws(b, i + 1)
            c = _need(b, i)
        top = len(stack) == 1
        if top:
            vb = i
        if c == 0x22:
            e, text = _string(b, i)
            if top:
                members.append(Member(key[0], key[1], key[2], i + 1, e, text, STRING))
            i = e + 1
        elif c in b"{[":
            if len(stack) == MAX_DEPTH:
                raise _Fail(i)
            stack.append(c == 0x7B)
            i += 1
            state = "first"
            continue
        elif c == 0x2D or c in _DIGITS:
            e, integer = _number(b, i)
            if top:
                kind, begin = DOUBLE, i
                if integer:
                    v = int(b[i:e])
                    if (-(1 << 63) <= v) if b[i] == 0x2D else (v < (1 << 64)):
                        kind = INT
                        if b[i] == 0x2D and v == 0:
                            begin = i + 1        # "-0" is 0
                members.append(Member(key[0], key[1], key[2], begin, e, None, kind))
            i = e
        elif c in b"tfn":
            word, kind = {0x74: (b"true", TRUE), 0x66: (b"false", FALSE), 0x6E: (b"null", NULL)}[c]
            for k, ch in enumerate(word):
                if _need(b, i + k) != ch:
                    raise _Fail(i + k)
            if top:
                members.append(Member(key[0], key[1], key[2], i, i + len(word), None, kind))
            i += len(word)
        else:
            raise _Fail(i)
        state = "after"
    i = _ws(b, i)
    if i < n:
        raise _Fail(i)
    return members


def walk(line):
    """-> (status, members, error offset)"""
    line = bytes(line)
    if not line:
        return EMPTY, [], 0
    try:
        return OK, _members(line), 0
    except _Fail as f:
        return FAIL, [], f.pos


def max_depth_reached(line):
    """the deepest level the walk opens before it ends (for the tests that ask which lines need the second launch)"""
    depth = most = 0
    in_string = escaped = False
    for c in bytes(line):
        if in_string:
            if escaped:
                escaped = False
            elif c == 0x5C:
                escaped = True
            elif c == 0x22:
                in_string = False
        elif c == 0x22:
            in_string = True
        elif c in b"{[":
            depth += 1
            most = max(most, depth)
        elif c in b"}]":
            depth -= 1
    return most


def render(line, m):
    """(key bytes, value bytes) of a member as the simdjson branch renders them (:190-238)"""
    key = m.key_text if m.key_text is not None else line[m.kb:m.ke]
    if m.type == STRING:
        value = m.val_text if m.val_text is not None else line[m.vb:m.ve]
    elif m.type == NULL:
        value = b""
    elif m.type == DOUBLE:
        value = b"%f" % float(line[m.vb:m.ve])      # std::to_string(double): snprintf("%f") of the correctly rounded double
    else:
        value = line[m.vb:m.ve]
    return bytes(key), bytes(value)


class Processor:
    """ProcessEvent :107-145 over events given as ordered (key, value) byte pairs"""

    def __init__(self, config):
        self.source_key = config["SourceKey"].encode()
        self.keep_fail = bool(config.get("KeepingSourceWhenParseFail", False))
        self.keep_succeed = bool(config.get("KeepingSourceWhenParseSucceed", False))
        self.renamed = (config.get("RenamedSourceKey") or config["SourceKey"]).encode()
        self.coping_raw_log = bool(config.get("CopingRawLog", False))
        self.counters = {"discarded": 0, "out_failed": 0, "out_key_not_found": 0, "out_successful": 0}
        self.alarms = []

    def process_event(self, contents):
        """contents: dict bytes -> bytes (insertion-ordered) -> the event's new contents, or None when the event is erased"""
        ev = dict(contents)
        if self.source_key not in ev:
            self.counters["out_key_not_found"] += 1
            return ev
        raw = ev[self.source_key]
        status, members, _ = walk(raw)
        ok = status == OK
        overwritten = False
        if ok:
            for m in members:
                k, v = render(raw, m)
                if k == self.source_key:
                    overwritten = True
                ev[k] = v
        elif status == FAIL:
            self.alarms.append(b"parse json fail:" + raw)
            self.counters["out_failed"] += 1
        if not ok or not overwritten:
            ev.pop(self.source_key, None)
        if (ok and self.keep_succeed) or (not ok and self.keep_fail):
            ev.setdefault(self.renamed, raw)
        if not ok and self.keep_fail and self.coping_raw_log:
            ev.setdefault(RAW_LOG_KEY.encode(), raw)
        if not ok and not self.keep_fail and not ev:
            self.counters["discarded"] += 1
            return None
        self.counters["out_successful"] += 1
        return ev
