"""processor_string_replace (plugins/processor/stringreplace/processor_string_replace.go), methods const and unquote, restated on bytes:
the one reference of every strrep test.  const is bytes.replace.  unquote restates strconv.Unquote of Go 1.23 as include/strrep/lc_strrep.h
words it; whether bytes are well-formed UTF-8 is asked of CPython's strict bytes.decode("utf-8") on the candidate sequence, so the model
shares no arithmetic with the kernels.  A model of Go's code, not Go: tests/golden/README_strrep.md."""

CHANGED, ERROR = 1, 2
ALARM_UNQUOTE, ALARM_TRIP_FAILED = 1, 2
MAX_MATCH, MAX_REPLACE = 32, 256
SIMPLE = {ord("a"): 7, ord("b"): 8, ord("f"): 12, ord("n"): 10, ord("r"): 13, ord("t"): 9, ord("v"): 11, ord("\\"): 0x5C, ord('"'): 0x22}


class UnquoteError(ValueError):
    pass


def init_error(config):
    """the message of the create call's refusal, or None (Init :61-95, and what lc_strrep.h defines)"""
    if not config.get("SourceKey"):
        return "no source key error"
    method = config.get("Method", "")
    if method == "const":
        if not config.get("Match"):
            return "no match error"
        if len(config["Match"].encode("utf-8")) > MAX_MATCH:
            return "Match is %d bytes long" % len(config["Match"].encode("utf-8"))
        if len(config.get("ReplaceString", "").encode("utf-8")) > MAX_REPLACE:
            return "ReplaceString is %d bytes long" % len(config["ReplaceString"].encode("utf-8"))
        return None
    if method == "regex":
        return "stays with the Go plugin"
    if method == "unquote":
        return None
    return "no method error"


def _well_formed(seq):
    try:
        seq.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def go_unquote(s):
    """strconv.Unquote(s) for an input that begins with `"` -> (bytes, a backslash escape or a replaced byte was met)"""
    if len(s) < 2 or s[:1] != b'"':
        raise UnquoteError("invalid syntax")
    out, i, escaped = bytearray(), 1, False
    while True:
        if i >= len(s):
            raise UnquoteError("no closing quote")
        c = s[i]
        if c == 0x22:
            if i != len(s) - 1:
                raise UnquoteError("a quote in front of the last byte")
            return bytes(out), escaped
        if c == 0x0A:
            raise UnquoteError("a raw newline")
        if c >= 0x80:
            for n in (2, 3, 4):
                if i + n <= len(s) and _well_formed(s[i:i + n]):
                    out += s[i:i + n]
                    i += n
                    break
            else:
                out += b"\xef\xbf\xbd"
                escaped = True
                i += 1
            continue
        if c != 0x5C:
            out.append(c)
            i += 1
            continue
        escaped = True
        if i + 1 >= len(s):
            raise UnquoteError("a backslash at the end")
        e = s[i + 1]
        i += 2
        if e in SIMPLE:
            out.append(SIMPLE[e])
        elif e in b"xuU":
            n = {ord("x"): 2, ord("u"): 4, ord("U"): 8}[e]
            digits = s[i:i + n]
            if len(digits) < n or any(d not in b"0123456789abcdefABCDEF" for d in digits):
                raise UnquoteError("hex digits")
            v = int(digits, 16)
            i += n
            if e == ord("x"):
                out.append(v)
            elif v > 0x10FFFF or 0xD800 <= v <= 0xDFFF:
                raise UnquoteError("no code point")
            else:
                out += chr(v).encode("utf-8")
        elif e in b"01234567":
            digits = s[i - 1:i + 2]
            if len(digits) < 3 or any(d not in b"01234567" for d in digits):
                raise UnquoteError("octal digits")
            v = int(digits, 8)
            if v > 255:
                raise UnquoteError("octal above 255")
            out.append(v)
            i += 2
        else:
            raise UnquoteError("escape %r" % bytes([e]))


def unquote_input(value):
    """:117-121 -> (the input of strconv.Unquote, form A?)"""
    if value.startswith(b'"') and value.endswith(b'"'):
        return value, True
    return b'"' + value.replace(b'"', b"\\x22") + b'"', False


def apply(config, value):
    """one value -> (flags, new bytes or None); config: the Go struct's fields as a dict, value: bytes"""
    if config["Method"] == "const":
        match, repl = config["Match"].encode("utf-8"), config.get("ReplaceString", "").encode("utf-8")
        if match not in value:
            return 0, None
        return CHANGED, value.replace(match, repl)
    text, form_a = unquote_input(value)
    try:
        out, escaped = go_unquote(text)
    except UnquoteError:
        return ERROR, None
    if not form_a and out == value:  # (form B, nothing to decode: a `"` went to \x22 and back)
        assert not escaped or b'"' in value
        return 0, None
    return CHANGED, out


def result(config, value):
    """what the Go assigns: the new value, or the value itself"""
    flags, out = apply(config, value)
    return out if flags & CHANGED else value


def alarm_text(config, value):
    return b"error:invalid syntax\tmethod:unquote\tsource_key:" + config["SourceKey"].encode("utf-8") + b"\tcontent:" + value + b"\t"


def process_logs(config, logs):
    """ProcessLogs :101-140 over logs of [key, value] str pairs -> (logs, [(kind, bytes)] alarms in order, counters as a dict)"""
    out, alarms = [], []
    c = {"values": 0, "changed": 0, "unquote_errors": 0, "failed_trips": 0, "replace_count": 0}
    dest = config.get("DestKey", "")
    for log in logs:
        contents = [list(kv) for kv in log]
        for cont in contents[:len(contents)]:  # (range evaluates the slice once: appended contents are not visited)
            if cont[0] != config["SourceKey"]:
                continue
            value = cont[1].encode("utf-8")
            flags, new = apply(config, value)
            c["values"] += 1
            c["replace_count"] += 1
            if flags & ERROR:
                c["unquote_errors"] += 1
                alarms.append((ALARM_UNQUOTE, alarm_text(config, value)))
            if flags & CHANGED:
                c["changed"] += 1
            text = (new if flags & CHANGED else value).decode("utf-8", "surrogateescape")
            if dest:
                contents.append([dest, text])
            else:
                cont[1] = text
        out.append([tuple(kv) for kv in contents])
    return out, alarms, c
