"""Test-only: the deterministic edge tables of the timestamp parser (strptimeRun of csrc/strptime_vm.hpp, strptime_kernel of
csrc/strptime_kernel.hpp).  One author for tests/test_timestamp_edges.py (the per-value routine on the host) and
tests/test_gpu_timestamp_edges.py (the kernel: its dword source and its workgroup of 255 new values).

What a value must give comes from helpers/timestamp_model.strptime_ns (tests/test_timestamp_model.py holds it to the reference's
recorded vectors); the civil seconds of the broken-down fields come from Python's own calendar (datetime.date.toordinal), which shares
no arithmetic with the kernel or the model.  same_as_prev follows the rule of include/lc_timestamp.h: both values parsed, equal
matched - frac_len, equal bytes over that prefix; index 0 and a value behind an absent or failed one read 0.  Not part of the product."""
import datetime

import numpy as np

from helpers import timestamp_model as model

INT_MIN = -2 ** 31
LC_TS_OK, LC_TS_HAS_YEAR, LC_TS_DST, LC_TS_EPOCH, LC_TS_ABSENT = 1, 2, 4, 8, 0x80
KEYS = ("status", "secs", "nanos", "matched", "frac_len", "same_as_prev")
_EPOCH_DAY = datetime.date(1970, 1, 1).toordinal()
CALENDAR_FORMAT = "%Y-%m-%d %H:%M:%S"
YEARS = [1, 4, 100, 400, 1582, 1600, 1700, 1899, 1900, 1901, 1968, 1969, 1970, 1971, 1972, 1999, 2000, 2001, 2037, 2038, 2039, 2100, 2106,
         2400, 9999]
DAYS = (1, 28, 29, 30, 31)
TIMES = ((0, 0, 0), (23, 59, 59), (23, 59, 60), (12, 0, 61))
BORDERS = (1, 254, 255, 256, 509, 510, 511)      # value i and the one before it; 255 and 510 open workgroups 1 and 2
BORDER_SETS = ((1, 254, 509), (255, 510), (256, 511))      # one launch each: a pair's two values belong to no other pair
N_BORDER = 600


def civil_seconds(year, mon0, mday, tod):
    """Python's calendar: days from 1970-01-01 to the first of the month, any mday (days beyond the month run on into the next), and
    the second of the day (60 and 61 run on into the next minute).  Years outside datetime's move by whole 400-year cycles."""
    cycles = 0
    while year < 1:
        year, cycles = year + 400, cycles - 1
    while year > 9999:
        year, cycles = year - 400, cycles + 1
    return (datetime.date(year, mon0 + 1, 1).toordinal() - _EPOCH_DAY + cycles * 146097 + mday - 1) * 86400 + tod


_rows = {}


def model_row(fmt, value):
    """what the routine must report for one value -> (status, secs, nanos or None where a failed "%s" leaves it open, matched, frac_len)"""
    key = (fmt, value)
    if key not in _rows:
        matched, tm, ns, ns_len, epoch = model.strptime_ns(value, fmt)
        ok = matched >= 0
        tod = tm["hour"] * 3600 + tm["min"] * 60 + tm["sec"]
        status = (LC_TS_OK if ok else 0) | (LC_TS_DST if tm["isdst"] else 0)
        if epoch is not None:
            status, secs = status | LC_TS_EPOCH | LC_TS_HAS_YEAR, epoch
        elif tm["year"] != INT_MIN:
            status, secs = status | LC_TS_HAS_YEAR, civil_seconds(tm["year"] + 1900, tm["mon"], tm["mday"], tod)
        else:
            secs = tm["mon"] << 40 | tm["mday"] << 32 | tod
        _rows[key] = (status, secs, ns if ok or fmt != "%s" else None, matched if ok else 0, max(ns_len, 0) if ok else 0)
    return _rows[key]


def expected(fmt, values):
    """values: bytes, or None for an absent one -> the six arrays, and the mask of the nanos that are held"""
    n = len(values)
    out = {"status": np.zeros(n, np.uint8), "secs": np.zeros(n, np.int64), "nanos": np.zeros(n, np.uint32), "matched": np.zeros(n, np.int32),
           "frac_len": np.zeros(n, np.int32), "same_as_prev": np.zeros(n, np.uint8)}
    held = np.ones(n, bool)
    prefix = [None] * n       # the matched prefix of a value that parsed
    for i, v in enumerate(values):
        if v is None:
            out["status"][i] = LC_TS_ABSENT
            continue
        status, secs, ns, matched, flen = model_row(fmt, v)
        out["status"][i], out["secs"][i], out["matched"][i], out["frac_len"][i] = status, secs, matched, flen
        if ns is None:
            held[i] = False
        else:
            out["nanos"][i] = ns
        if status & LC_TS_OK:
            prefix[i] = v[:matched - flen]
            out["same_as_prev"][i] = 1 if i and prefix[i - 1] is not None and prefix[i - 1] == prefix[i] else 0
    return out, held


def compare(got, fmt, values, what):
    """all six arrays of a launch against the model and the rule, bit for bit"""
    want, held = expected(fmt, values)
    for k in KEYS:
        g = np.asarray(got[k]).view(want[k].dtype)[:len(values)]
        differ = g != want[k]
        if k == "nanos":
            differ &= held
        if differ.any():
            i = int(np.nonzero(differ)[0][0])
            raise AssertionError("%s: %s of value %d %r (behind %r): %r, the model %r" % (what, k, i, values[i], values[i - 1] if i else None, int(g[i]), int(want[k][i])))


# ---------------------------------------------------------------------------------------------- the calendar table
def calendar_table():
    """-> [(format, value, civil seconds by datetime or None: the model alone holds it)]"""
    table = []
    for y in YEARS:
        for m in range(1, 13):
            first = datetime.date(y, m, 1).toordinal() - _EPOCH_DAY
            for d in DAYS:
                for hh, mm, ss in TIMES:
                    table.append((CALENDAR_FORMAT, b"%04d-%02d-%02d %02d:%02d:%02d" % (y, m, d, hh, mm, ss), (first + d - 1) * 86400 + hh * 3600 + mm * 60 + ss))
    for m in range(1, 13):      # year 0000 lies outside datetime
        for d in DAYS:
            table.append((CALENDAR_FORMAT, b"0000-%02d-%02d 23:59:60" % (m, d), None))
    for yy in (0, 68, 69, 99):  # the pivot of %y: 69..99 are 19xx, 00..68 are 20xx
        for m in range(1, 13):
            for d in DAYS:
                table.append(("%y%m%d", b"%02d%02d%02d" % (yy, m, d), (datetime.date((2000 if yy <= 68 else 1900) + yy, m, 1).toordinal() - _EPOCH_DAY + d - 1) * 86400))
    epoch = [b"7", b"170000000", b"1700000000", b"17000000001", b"1700000000123456789", b"17000000001234567891", b"99999999999999999999",
             b"+1700000000", b"-1700000000", b"-17000000001", b"+17000000001", b" 1700000000", b"0", b"-0", b"0000000000", b"00000000001", b"",
             b"1700000000.5", b"1234567890987654321", b"12345678901", b"1234567890000000001", b"1234567890x", b"12345678909x", b"x"]
    for v in epoch:
        digits = v.lstrip(b"+").isdigit() and len(v.lstrip(b"+")) <= 10 and int(v) != 0
        table.append(("%s", v, int(v) if digits else None))
    return table


def by_format(table):
    groups = {}
    for fmt, value, secs in table:
        groups.setdefault(fmt, []).append((value, secs))
    return groups


# ---------------------------------------------------------------------------------------------- packed values
class Batch:
    """values in one data buffer: value i = data[off[i] + begin[i] .. off[i] + end[i]); values[i] is what the model reads (None: absent)"""

    def __init__(self, pad_front=0):
        self.blob = bytearray((b"7:1 " * 2)[:pad_front])
        self.off, self.spans, self.values = [], [], []

    def add(self, text, absent=None, before=b"", after=b""):
        """text (with `before` and `after` around it, outside the span) behind what is there; absent: "negative" = span (-1, -1),
        "reversed" = end < begin, "line" = a good span the caller's line status takes away -- the bytes are there all the same"""
        self.off.append(len(self.blob))
        self.blob += before + text + after
        b, e = len(before), len(before) + len(text)
        self.spans.append({None: (b, e), "line": (b, e), "negative": (-1, -1), "reversed": (b + 3, b + 1)}[absent])
        self.values.append(None if absent else bytes(text))

    def view(self, off, begin, end):
        """a value that lies in bytes already placed"""
        self.off.append(off)
        self.spans.append((begin, end))
        self.values.append(bytes(self.blob[off + begin:off + end]))

    def arrays(self, ngroups=1, group=0):
        """-> (data u8 padded to a whole 16-byte unit plus one more with digits, never zeros; off i32[n]; spans i32[n, 2 * ngroups] with
        the other groups' entries junk, large and negative)"""
        n = len(self.off)
        size = (len(self.blob) + 15) // 16 * 16 + 16
        data = np.frombuffer(bytes(self.blob) + b"0123456789" * ((size - len(self.blob)) // 10 + 1), np.uint8)[:size].copy()
        spans = np.empty((n, 2 * ngroups), np.int32)
        spans[:, 0::2], spans[:, 1::2] = 0x7FFFFF00, -0x7FFFFF00
        spans[1::2, 0::2], spans[1::2, 1::2] = -5, 0x7FFFFFF0
        spans[:, 2 * group:2 * group + 2] = np.array(self.spans, np.int32).reshape(n, 2)
        return data, np.array(self.off, np.int32), spans


# ---------------------------------------------------------------------------------------------- the 255-value border
FRACTION_FORMAT, YEARLESS_FORMAT = "%Y-%m-%d %H:%M:%S.%f", "%b %d %H:%M:%S"
VARIANTS = ("equal", "fraction_digits", "fraction_length", "last_byte", "first_byte", "predecessor_fails", "predecessor_shorter",
            "predecessor_absent_negative", "predecessor_absent_reversed", "value_absent")


def _text(fmt, i, day=b"05", first=None, frac=b"123", bump=0):
    hh, mm, ss = i // 3600, i // 60 % 60, (i % 60) ^ bump      # neighbours differ in their seconds; bump: in the last digit only
    if fmt == FRACTION_FORMAT:
        return (first or b"2") + b"024-03-%s %02d:%02d:%02d.%s" % (day, hh, mm, ss, frac)
    return (first or b"M") + b"ar %s %02d:%02d:%02d" % (day, hh, mm, ss)


def border_batch(fmt, variant, pad_front, borders, n=N_BORDER, absent_kind=None, sprinkle=False, before=b"", after=b""):
    """n values, each distinct from its neighbours, but for the pairs (i - 1, i) of `borders`, which are `variant`; the predecessors carry
    0..3 bytes of junk behind what the format consumes (inside their span), so the dword residues of both values vary.  absent_kind:
    how the absent value of the three absent variants is absent (default: by its span); sprinkle: every ninth value away from the
    borders is absent by its line as well; before / after: bytes around every value, outside its span"""
    has_frac = fmt == FRACTION_FORMAT
    junk = b"zy x"
    texts = [_text(fmt, i) for i in range(n)]
    absent = [None] * n
    if sprinkle:
        for i in range(4, n, 9):
            if all(abs(i - b) > 2 for b in borders):
                absent[i] = "line"
    for i in borders:
        cur = prev = texts[i]
        if variant == "fraction_digits" and has_frac:
            prev = _text(fmt, i, frac=b"456")
        elif variant == "fraction_length" and has_frac:
            prev, cur = _text(fmt, i, frac=b"12"), _text(fmt, i, frac=b"123456")
        elif variant == "last_byte":
            prev = _text(fmt, i, bump=1)
        elif variant == "first_byte":
            prev = _text(fmt, i, first=b"3" if has_frac else b"m")
        elif variant == "predecessor_fails":
            k = cur.rindex(b":") - 2
            prev = cur[:k] + b"7" + cur[k + 1:]      # minutes of 70 and more: %M stops behind the 7 and no colon follows
        elif variant == "predecessor_shorter":
            prev = _text(fmt, i, day=b"5")
        elif variant in ("predecessor_absent_negative", "predecessor_absent_reversed"):
            absent[i - 1] = absent_kind or variant.rsplit("_", 1)[1]
        elif variant == "value_absent":
            absent[i] = absent_kind or "negative"
            texts[i + 1] = cur      # its successor equals the value before the absent one, and reads 0 all the same
        else:
            assert variant in ("equal", "fraction_digits", "fraction_length"), variant
        texts[i - 1], texts[i] = prev, cur
    batch = Batch(pad_front)
    for i in range(n):
        tail = junk[:(BORDERS.index(i + 1) + pad_front) % 4] if i + 1 in borders else b""
        batch.add(texts[i] + tail, absent=absent[i], before=before, after=after)
    return batch


# ---------------------------------------------------------------------------------------------- the span end
SPAN_END_VALUES = [
    ("%Y-%m-%d %H:%M:%S.%f", b"2024-03-05 12:34:56.123456789"),
    ("%d/%b/%Y:%H:%M:%S %z", b"05/Mar/2024:12:34:56 +0830"),
    ("%b %d %H:%M:%S", b"Mar 15 12:34:56"),
    ("%s", b"17000000001234"),
    ("%y%m%d %I:%M:%S %p", b"240305 11:34:56 PM"),
    ("%A %B %d %Y", b"Wednesday September 14 2024"),
]


def span_end_batch(value, pad_front):
    """`value` truncated to every length 0 .. len, twice: as views of ONE copy (the byte behind a truncation is the very byte the match
    would go on with: a digit, the next letter of a name) and as copies packed back to back (the byte behind is the next copy's first)"""
    batch = Batch(pad_front)
    batch.add(value)
    at = batch.off[0]
    for k in range(len(value) + 1):
        batch.view(at, 0, k)
    for k in range(len(value) + 1):
        batch.add(value[:k])
    return batch
