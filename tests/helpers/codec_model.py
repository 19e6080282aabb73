"""A Python model of the field codecs (include/codec/lc_codec.h: base64 encode, base64 decode, MD5), written from the rules the issue
and the header state -- not from csrc/codec_vm.hpp -- and without base64 / binascii / hashlib, which are the WITNESSES it is held against
in tests/test_codec_model.py.  Everything works on bytes."""
import functools
import math

OUT, ERROR = 1, 2
ALARM_DECODE, ALARM_NO_KEY, ALARM_TRIP_FAILED = 1, 2, 3
COUNTERS = ("values", "out", "decode_errors", "no_key", "failed_trips")
OPS = ("base64_encode", "base64_decode", "md5")
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
SEXTET = {c: i for i, c in enumerate(ALPHABET)}
SKIP = b"\r\n"
PAD = ord("=")


def encode(value):
    out = bytearray()
    for i in range(0, len(value), 3):
        chunk = value[i:i + 3]
        bits = int.from_bytes(chunk + b"\0" * (3 - len(chunk)), "big")
        chars = [ALPHABET[(bits >> s) & 63] for s in (18, 12, 6, 0)]
        out += bytes(chars[:len(chunk) + 1]) + b"=" * (3 - len(chunk))
    return bytes(out)


def _bytes_of(sextets, count):
    bits = 0
    for s in sextets:
        bits = (bits << 6) | s
    total = 6 * len(sextets)
    whole = total // 8
    return (bits >> (total - 8 * whole)).to_bytes(whole, "big")[:count] if whole else b""


def decode(value):
    """-> (decoded bytes, None) or (None, error offset)"""
    n = len(value)
    p = next((i for i, c in enumerate(value) if c not in SEXTET and c not in SKIP), None)
    sextets = [SEXTET[c] for c in (value if p is None else value[:p]) if c in SEXTET]
    k = len(sextets)
    if p is None:
        if k % 4 == 0:
            return _bytes_of(sextets, 3 * k // 4), None
        return None, n - k % 4
    if value[p] != PAD:
        return None, p
    j = k % 4
    if j < 2:
        return None, p
    i = p + 1
    if j == 2:
        while i < n and value[i] in SKIP:
            i += 1
        if i == n:
            return None, n
        if value[i] != PAD:
            return None, i - 1
        i += 1
    while i < n and value[i] in SKIP:
        i += 1
    if i < n:
        return None, i
    return _bytes_of(sextets, 3 * (k // 4) + j - 1), None


_S = [7, 12, 17, 22] * 4 + [5, 9, 14, 20] * 4 + [4, 11, 16, 23] * 4 + [6, 10, 15, 21] * 4
_K = [int(abs(math.sin(i + 1)) * 2 ** 32) & 0xFFFFFFFF for i in range(64)]


def md5_hex(value):
    """RFC 1321, as 32 lower-case hex digits"""
    msg = value + b"\x80" + b"\0" * ((55 - len(value)) % 64) + (8 * len(value)).to_bytes(8, "little")
    h = [0x67452301, 0xefcdab89, 0x98badcfe, 0x10325476]
    for at in range(0, len(msg), 64):
        x = [int.from_bytes(msg[at + 4 * i:at + 4 * i + 4], "little") for i in range(16)]
        a, b, c, d = h
        for i in range(64):
            if i < 16:
                f, g = (b & c) | (~b & d), i
            elif i < 32:
                f, g = (d & b) | (~d & c), (5 * i + 1) % 16
            elif i < 48:
                f, g = b ^ c ^ d, (3 * i + 5) % 16
            else:
                f, g = c ^ (b | ~d), (7 * i) % 16
            f = (f + a + _K[i] + x[g]) & 0xFFFFFFFF
            a, d, c = d, c, b
            b = (b + ((f << _S[i]) | (f >> (32 - _S[i])))) & 0xFFFFFFFF
        h = [(v + w) & 0xFFFFFFFF for v, w in zip(h, (a, b, c, d))]
    return b"".join(v.to_bytes(4, "little") for v in h).hex().encode()


@functools.lru_cache(maxsize=None)
def apply(op, value):
    """-> (flags, output bytes or None, error offset or None)"""
    if op == "base64_encode":
        return OUT, encode(value), None
    if op == "md5":
        return OUT, md5_hex(value), None
    assert op == "base64_decode"
    out, err = decode(value)
    return (OUT, out, None) if err is None else (ERROR, None, err)


def error_text(offset):
    return "illegal base64 data at input byte %d" % offset


def init_error(config):
    return None if config.get("Op") in OPS else "Op"


def process_logs(config, logs):
    """logs: [[(key, value), ...], ...] (str) -> (logs, alarms as (kind, bytes), counters).  Values are UTF-8 text on both sides."""
    op, source = config["Op"], config.get("SourceKey", "")
    new_key = config.get("MD5Key", "") if op == "md5" else config.get("NewKey", "")
    counters = dict.fromkeys(COUNTERS, 0)
    alarms, out = [], []
    for log in logs:
        log = [tuple(kv) for kv in log]
        at = next((i for i, (k, _) in enumerate(log) if k == source), None)
        if at is None:
            counters["no_key"] += 1
            if config.get("NoKeyError"):
                alarms.append((ALARM_NO_KEY, ("cannot find key:%s\t" % source).encode("utf-8")))
        else:
            counters["values"] += 1
            flags, new, err = apply(op, log[at][1].encode("utf-8"))
            if flags & OUT:
                counters["out"] += 1
                if op == "base64_encode" and not new_key:
                    log[at] = (log[at][0], new.decode("utf-8"))
                else:
                    log.append((new_key, new.decode("utf-8")))
            else:
                counters["decode_errors"] += 1
                if config.get("DecodeError"):
                    alarms.append((ALARM_DECODE, ("decode base64 error:%s\t" % error_text(err)).encode("utf-8")))
        out.append(log)
    return out, alarms, counters
