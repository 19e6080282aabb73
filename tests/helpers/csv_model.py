"""processor_csv as a model on bytes: the reader rules of Go 1.23's encoding/csv as plugins/processor/csv/processor_csv.go uses them
(Comma = SplitSep, TrimLeadingSpace as configured, LazyQuotes = false, Comment = 0, FieldsPerRecord = 0; the FIRST record only), the
csv.Writer rules of its remainder, and decodeCSV / ProcessLogs around them.  Written LINE BY LINE, the way the Go reads: read_line()
hands out one line with its end rewritten, read() works on that line alone.  csrc/csv_vm.hpp is one pass over the raw bytes; the two
share no structure, so that either can show the other wrong.  tests/golden/README_csv.md says what pins the model itself."""

OK, EOF, BARE_QUOTE, QUOTE = "ok", "eof", "bare_quote", "quote"
STATUS_CODE = {OK: 0, EOF: 1, BARE_QUOTE: 2, QUOTE: 3}
SENTENCE = {BARE_QUOTE: b'bare " in non-quoted-field', QUOTE: b'extraneous or missing " in quoted-field'}
INVALID_DELIM = b"csv: invalid field or comment delimiter"
ALARM_NO_SOURCE_KEY, ALARM_DECODE, ALARM_KEY_COUNT, ALARM_TRIP_FAILED = 1, 2, 3, 4

# unicode.IsSpace, as UTF-8
SPACE_RUNES = [b"\t", b"\n", b"\v", b"\f", b"\r", b" ", b"\xc2\x85", b"\xc2\xa0", b"\xe1\x9a\x80"] + \
              [b"\xe2\x80" + bytes([c]) for c in range(0x80, 0x8B)] + [b"\xe2\x80\xa8", b"\xe2\x80\xa9", b"\xe2\x80\xaf", b"\xe2\x81\x9f", b"\xe3\x80\x80"]

DEFAULTS = {"SourceKey": "", "NoKeyError": False, "SplitKeys": [], "SplitSep": ",", "TrimLeadingSpace": False, "PreserveOthers": False,
            "ExpandOthers": False, "ExpandKeyPrefix": "", "KeepSource": False}


class InvalidSeparator(ValueError):
    pass


def go_runes(text):
    """[]rune(string) of Go for UTF-8 bytes: malformed input gives U+FFFD per byte"""
    out, i = [], 0
    while i < len(text):
        for width in (1, 2, 3, 4):
            try:
                ch = text[i:i + width].decode("utf-8")
            except UnicodeDecodeError:
                continue
            if len(ch) == 1:
                out.append(ord(ch))
                i += width
                break
        else:
            out.append(0xFFFD)
            i += 1
    return out


def init(config):
    """Init :46-54 over the defaults -> the configuration with bytes where the Go has strings; "valid": validDelim(Comma)"""
    c = dict(DEFAULTS)
    c.update(config)
    sep = c["SplitSep"].encode("utf-8") if isinstance(c["SplitSep"], str) else c["SplitSep"]
    runes = go_runes(sep)
    if len(runes) != 1:
        raise InvalidSeparator("invalid separator: " + sep.decode("utf-8", "replace"))
    c["sep"] = sep
    c["valid"] = runes[0] not in (0, ord('"'), 13, 10, 0xFFFD)
    return c


def length_nl(line):
    return 1 if line.endswith(b"\n") else 0


def trim_left_space(line):
    """bytes.IndexFunc(line, !unicode.IsSpace): the line without its leading white-space runes"""
    while True:
        for r in SPACE_RUNES:
            if line.startswith(r):
                line = line[len(r):]
                break
        else:
            return line


class _Lines:
    def __init__(self, value):
        self.rest = value

    def read_line(self):
        """-> the next line with its end rewritten, or None at the end of the input (readLine)"""
        if not self.rest:
            return None
        cut = self.rest.find(b"\n")
        if cut < 0:
            line, self.rest = self.rest, b""
            if line.endswith(b"\r"):  # the last line without `\n` loses one trailing `\r`
                line = line[:-1]
            return line
        line, self.rest = self.rest[:cut + 1], self.rest[cut + 1:]
        if line.endswith(b"\r\n"):
            line = line[:-2] + b"\n"
        return line


def read(value, sep=b",", trim=False):
    """r.Read() -> (status, fields): (OK, [bytes, ...]), (EOF, []), or an error status with []"""
    lines = _Lines(value)
    while True:  # empty lines, before any trimming
        line = lines.read_line()
        if line is None:
            return EOF, []
        if len(line) != length_nl(line):
            break
    fields = []
    while True:
        if trim:
            line = trim_left_space(line)
        if not line.startswith(b'"'):  # an unquoted field
            i = line.find(sep)
            field = line[:i] if i >= 0 else line[:len(line) - length_nl(line)]
            if b'"' in field:
                return BARE_QUOTE, []
            fields.append(field)
            if i < 0:
                return OK, fields
            line = line[i + len(sep):]
            continue
        line = line[1:]  # a quoted field
        text = b""
        while True:
            i = line.find(b'"')
            if i >= 0:
                text += line[:i]
                line = line[i + 1:]
                if line.startswith(b'"'):
                    text += b'"'
                    line = line[1:]
                elif line.startswith(sep):
                    line = line[len(sep):]
                    fields.append(text)
                    break  # the next field
                elif length_nl(line) == len(line):
                    fields.append(text)
                    return OK, fields
                else:
                    return QUOTE, []
            elif line:
                text += line
                line = lines.read_line()
                if line is None:
                    line = b""
            else:
                return QUOTE, []  # the input ends inside the quotes


def field_needs_quotes(field, sep):
    if not field:
        return False
    if field == b"\\." or sep in field or any(c in field for c in (b'"', b"\r", b"\n")):
        return True
    return any(field.startswith(r) for r in SPACE_RUNES)


def write(fields, sep=b","):
    """csv.Writer.Write + Flush -> the line with its final `\\n`"""
    out = []
    for f in fields:
        out.append(b'"' + f.replace(b'"', b'""') + b'"' if field_needs_quotes(f, sep) else f)
    return sep.join(out) + b"\n"


def cut_string(value):
    return value if len(value) < 1024 else value[:1024]


def decode_csv(c, contents, value):
    """decodeCSV :60-110 on an initialised config: appends to contents -> (res, [(kind, text)] alarms)"""
    keys = [k.encode("utf-8") if isinstance(k, str) else k for k in c["SplitKeys"]]
    if not keys:
        if c["PreserveOthers"]:
            contents.append([b"_decode_preserve_", value])
        return True, []
    if not c["valid"]:
        return False, [(ALARM_DECODE, b"cannot decode log:" + INVALID_DELIM + b"\tlog:" + cut_string(value) + b"\t")]
    status, record = read(value, c["sep"], c["TrimLeadingSpace"])
    if status in (BARE_QUOTE, QUOTE):
        return False, [(ALARM_DECODE, b"cannot decode log:" + SENTENCE[status] + b"\tlog:" + cut_string(value) + b"\t")]
    if status == EOF:
        record = [b""]
    k = 0
    while k < len(keys) and k < len(record):
        contents.append([keys[k], record[k]])
        k += 1
    if k < len(record) and c["PreserveOthers"]:
        if c["ExpandOthers"]:
            prefix = c["ExpandKeyPrefix"].encode("utf-8")
            while k < len(record):
                contents.append([prefix + b"%d" % (k + 1 - len(keys)), record[k]])
                k += 1
        else:
            contents.append([b"_decode_preserve_", write(record[k:], c["sep"])[:-1]])
    alarms = []
    if len(keys) != len(record):
        alarms.append((ALARM_KEY_COUNT, b"decode keys not match, split len:%d" % len(record) + b"\tlog:" + cut_string(value) + b"\t"))
    return True, alarms


def process_log(config, contents):
    """ProcessLogs :112-130 for one log: contents [[key bytes, value bytes], ...] -> (contents, alarms)"""
    c = init(config)
    contents = [list(kv) for kv in contents]
    source = c["SourceKey"].encode("utf-8")
    for i, (key, value) in enumerate(contents):
        if not source or source == key:
            res, alarms = decode_csv(c, contents, value)
            if not (c["KeepSource"] or not res):
                del contents[i]
            return contents, alarms
    return contents, ([(ALARM_NO_SOURCE_KEY, b"cannot find key:" + source + b"\t")] if c["NoKeyError"] else [])
