"""The reference's processor_split_key_value restated line by line (plugins/processor/split/keyvalue/key_value_splitter.go:53-192), on
bytes as Go indexes strings, every slice through a helper that raises GoPanic where Go's bounds check panics.  It is the reference of
every key-value test: the per-value routine of csrc/kv_vm.hpp is never its own reference.

split(cfg, value) -> the engine's view: ("ok", [(kind, key, value, spans)]) or ("panic", None), where kind is "pair", "nosep" (the
reference's noSeparatorKeyIndex pairs, before DiscardWhenSeparatorNotFound) or "empty" (emptyKeyIndex), and spans = (key begin, key end,
value begin, value end) relative to the value's first byte as include/kvsplit/lc_kvsplit.h reports them.
process_log(cfg, contents) -> (contents, alarms): the Go processLog on a list of [key, value]."""

DEFAULTS = {"SourceKey": "", "Delimiter": "", "Separator": "", "KeepSource": True, "EmptyKeyPrefix": "", "NoSeparatorKeyPrefix": "", "Quote": "",
            "DiscardWhenSeparatorNotFound": False, "ErrIfSourceKeyNotFound": True, "ErrIfSeparatorNotFound": True, "ErrIfKeyIsEmpty": True}
LC_KV_OK, LC_KV_REF_PANIC = 0, 1
# alarm kinds of lc_kvsplit_set_alarm_sink
ALARM_NO_SOURCE_KEY, ALARM_NO_SEPARATOR, ALARM_EMPTY_KEY, ALARM_REF_PANIC, ALARM_TRIP_FAILED = 1, 2, 3, 4, 5


class GoPanic(Exception):
    pass


def _b(x):
    return x if isinstance(x, bytes) else x.encode("utf-8")


def init(config):
    """Init :53-69 over newKeyValueSplitter's defaults :194-206 -> a dict with bytes needles"""
    c = dict(DEFAULTS)
    c.update(config)
    for k in ("SourceKey", "Delimiter", "Separator", "EmptyKeyPrefix", "NoSeparatorKeyPrefix", "Quote"):
        c[k] = _b(c[k])
    if len(c["Delimiter"]) == 0:
        c["Delimiter"] = b"\t"
    if len(c["Separator"]) == 0:
        c["Separator"] = b":"
    if len(c["EmptyKeyPrefix"]) == 0:
        c["EmptyKeyPrefix"] = b"empty_key_"
    if len(c["NoSeparatorKeyPrefix"]) == 0:
        c["NoSeparatorKeyPrefix"] = b"no_separator_key_"
    return c


def _slice(s, lo, hi):
    """s[lo:hi] with Go's check: 0 <= lo <= hi <= len(s)"""
    if not 0 <= lo <= hi <= len(s):
        raise GoPanic("slice bounds out of range [%d:%d] with length %d" % (lo, hi, len(s)))
    return s[lo:hi]


def _from(s, lo):
    return _slice(s, lo, len(s))


def _to(s, hi):
    return _slice(s, 0, hi)


def _index(s, sub):
    return s.find(sub)  # strings.Index: the first occurrence, -1 without one, 0 for an empty needle


def get_nearest_quote(c, content, start_pos):  # :160-182
    quote, separator = c["Quote"], c["Separator"]
    while start_pos < len(content):
        if len(quote) == 1:
            last_quote_content = _index(_from(content, start_pos), b" \\" + quote)
            last_quote = _index(_from(content, start_pos + 1), quote)
            start_pos = last_quote + start_pos + 1 + len(quote)
            if last_quote_content >= 0:
                if last_quote_content + 1 == last_quote:
                    continue
                elif last_quote >= 0:
                    return start_pos
            else:
                return start_pos
        else:
            start_pos += _index(_from(content, start_pos + 1), quote) + len(separator + quote)
            return start_pos
    return start_pos


def concat_quote_pair(c, pair, content, d_idx):  # :145-158
    quote, separator = c["Quote"], c["Separator"]
    if d_idx >= 0 and len(quote) > 0 and not pair.endswith(quote) and (_index(pair, separator + quote) > 0 or pair.startswith(quote)):
        last_quote = get_nearest_quote(c, content, d_idx)
        if last_quote >= 0:
            d_idx = last_quote
            pair = _to(content, d_idx)
    return pair, d_idx


def get_value(c, value):  # :184-192 -> (value, how many bytes were taken from its front)
    len_q = len(c["Quote"])
    if len_q > 0:
        if len(value) >= 2 * len_q and value.startswith(c["Quote"]) and value.endswith(c["Quote"]):
            return _slice(value, len_q, len(value) - len_q), len_q
    return value, 0


def split_key_value(c, content, on_pair, on_alarm=None):  # :99-143; on_pair(kind, key, value, spans) -> appended?
    empty_key_index = 0
    no_separator_key_index = 0
    delimiter, separator = c["Delimiter"], c["Separator"]
    base = 0  # where `content` begins in the value
    while True:
        d_idx = _index(content, delimiter)
        pair = content if d_idx == -1 else _to(content, d_idx)
        pair, d_idx = concat_quote_pair(c, pair, content, d_idx)
        pos = _index(pair, separator)
        if pos == -1:
            if c["ErrIfSeparatorNotFound"] and on_alarm:
                on_alarm(ALARM_NO_SEPARATOR, b"can not find separator in " + pair)
            if not c["DiscardWhenSeparatorNotFound"]:
                value, cut = get_value(c, pair)
                on_pair("nosep", c["NoSeparatorKeyPrefix"] + str(no_separator_key_index).encode(), value,
                        (-1, no_separator_key_index, base + cut, base + cut + len(value)))
                no_separator_key_index += 1
        else:
            key = _to(pair, pos)
            value, cut = get_value(c, _from(pair, pos + len(separator)))
            vb = base + pos + len(separator) + cut
            kind, spans = "pair", (base, base + pos, vb, vb + len(value))
            if len(key) == 0:
                key = c["EmptyKeyPrefix"] + str(empty_key_index).encode()
                kind, spans = "empty", (-2, empty_key_index, vb, vb + len(value))
                empty_key_index += 1
                if c["ErrIfKeyIsEmpty"] and on_alarm:
                    on_alarm(ALARM_EMPTY_KEY, b"the key of pair with value (" + value + b") is empty")
            on_pair(kind, key, value, spans)
        if d_idx == -1 or d_idx + len(delimiter) > len(content):
            break
        content = _from(content, d_idx + len(delimiter))
        base += d_idx + len(delimiter)


def split(config, value):
    """the engine's view of one value: nothing discarded, no alarms"""
    c = init(config)
    c["DiscardWhenSeparatorNotFound"] = False
    pairs = []
    try:
        split_key_value(c, _b(value), lambda kind, k, v, spans: pairs.append((kind, k, v, spans)))
    except GoPanic:
        return "panic", None
    return "ok", pairs


def process_log(config, contents):
    """processLog :82-97 as this project DEFINES it: a value on which the reference panics leaves the log unchanged and raises
    ALARM_REF_PANIC.  contents: [[key, value], ...] (bytes) -> (new contents, [(kind, text)])"""
    c = init(config)
    contents = [[_b(k), _b(v)] for k, v in contents]
    alarms = []
    for idx, (key, value) in enumerate(contents):
        if len(c["SourceKey"]) == 0 or c["SourceKey"] == key:
            out = [list(p) for p in contents]
            if not c["KeepSource"]:
                del out[idx]
            pending = []
            try:
                split_key_value(c, value, lambda kind, k, v, spans: out.append([k, v]), lambda kind, text: pending.append((kind, text)))
            except GoPanic:
                return contents, [(ALARM_REF_PANIC, b"the reference indexes out of range on this value: log left unchanged")]
            return out, pending
    if c["ErrIfSourceKeyNotFound"]:
        alarms.append((ALARM_NO_SOURCE_KEY, b"can not find key: " + c["SourceKey"]))
    return contents, alarms
