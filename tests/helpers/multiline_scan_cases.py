"""The case table of the record scan (ml_flags_kernel, ml_bounds_kernel; csrc/multiline_scan.hpp): flag bytes chosen from the scan's own
geometry, not from a workload.  Deterministic: every array comes from a generator seeded by the family's name and the item count.

A case is Case(name, mode, flags, n_dyn): `flags` holds one byte per item -- bit 0 / 1 / 2: the item matches the start / continue / end
pattern, bit 3 (the "empty bit"): as a line of a read buffer the item is empty; n_dyn is the device-side item count the launch is given
(None: no count, the launch works on max_items = len(flags)).  forms(case) gives the three shapes every case runs in: item records
(off=None, empty bits cleared) and byte records over a terminated and an unterminated value.

The geometry restated here (multiline_scan.hpp): one workgroup of 512 threads, one slice of items per thread, a slice holds
max(16, ceil(n / 512)) items; ml_flags_kernel works in blocks of 256 items.  The expected records always come from
helpers/multiline_walk.walk, which knows nothing of slices."""
import zlib
from collections import namedtuple

import numpy as np

from helpers.multiline_walk import F_CONT, F_EMPTY, F_END, F_START, REC_LAST, REC_MATCHED, REC_RUN
from loongcollector_amd import multiline as ML

Case = namedtuple("Case", "name mode flags n_dyn")

THREADS, MIN_SLICE, FLAG_BLOCK = 512, 16, 256


def slice_items(n):
    return max(MIN_SLICE, (n + THREADS - 1) // THREADS)


def slice_count(n):
    return (n + slice_items(n) - 1) // slice_items(n)


BASE_MODES = (1, 3, 4, 5, 6, 7)                     # every mode with a start or an end pattern
MODES = tuple(b | d | f for b in BASE_MODES for d in (0, ML.ML_DISCARD) for f in (0, ML.ML_FLUSH))
# the sizes the full cross of MODES runs on, and why
SIZES = (0, 1,                                      # smallest inputs
         15, 16, 17,                                # one slice / two slices
         255, 256, 257,                             # ml_flags_kernel block border
         8191, 8192, 8193,                          # slices of 16 become slices of 17; 512 of them become 482
         8208,                                      # 16 * 513
         8703, 8704, 8705)                          # 512 full slices of 17, then slices of 18
LARGE_SIZES = (16384, 16385, 100003)                # slices of 32, 33 and 196 items
# the larger sizes run on every base mode once, with the flush and the discard bit spread over them
LARGE_MODES = (1 | ML.ML_FLUSH, 3 | ML.ML_FLUSH, 4, 5 | ML.ML_FLUSH | ML.ML_DISCARD, 6 | ML.ML_FLUSH, 7)


def mode_name(mode):
    return "".join(c for c, b in (("S", 1), ("C", 2), ("E", 4)) if mode & b) + ("-discard" if mode & ML.ML_DISCARD else "") + \
        ("-flush" if mode & ML.ML_FLUSH else "")


def _rng(family, n):
    return np.random.default_rng(zlib.crc32(("%s/%d" % (family, n)).encode()))


def _biased(family, n, value, share):
    rng = _rng(family, n)
    fl = rng.integers(0, 16, size=n, dtype=np.uint8)
    fl[rng.random(n) < share] = value
    return fl


def _queue(n):
    """item i has the continue bit except where i % per == 7: in the continue + end modes every slice but the first ends, unmatched, a
    run that began in the slice before, and hands it to phase D; with the flush the tail queues one more"""
    fl = np.full(n, F_CONT, dtype=np.uint8)
    fl[np.arange(n) % slice_items(n) == 7] = 0
    return fl


def _span(n, last):
    """one run from item 3 to item n - 2 (all continue), and what the last item does to it"""
    fl = np.full(n, F_CONT, dtype=np.uint8)
    fl[:3] = 0
    fl[3] = F_START | F_CONT
    fl[n - 1] = last
    return fl


def _slice_edges(n, first, last, rest):
    per = slice_items(n)
    fl = np.full(n, rest, dtype=np.uint8)
    at = np.arange(n) % per
    if last is not None:
        fl[at == per - 1] = last
        if n:
            fl[n - 1] = last
    fl[at == 0] = first
    return fl


def _empty_at(n, pos):
    """a run from item 0 (start + continue), continued by every item but `pos`, which is an empty line that matches nothing; the item
    behind it starts the next run"""
    fl = np.full(n, F_CONT, dtype=np.uint8)
    fl[0] |= F_START
    fl[pos] = F_EMPTY
    if pos + 1 < n:
        fl[pos + 1] |= F_START
    return fl


def families(n, large=False):
    """-> [(family name, flags)] for n items"""
    if large:
        out = [("rand98C", _biased("rand98C", n, F_CONT, 0.98)), ("queue", _queue(n)), ("span-flush", _span(n, F_CONT))]
        if n < 50000:
            out += [("rand", _biased("rand", n, 0, 0.0)), ("span-unmatched", _span(n, 0))]
        return out
    out = [("rand", _biased("rand", n, 0, 0.0)), ("rand90C", _biased("rand90C", n, F_CONT, 0.90)),
           ("rand98C", _biased("rand98C", n, F_CONT, 0.98)), ("rand90none", _biased("rand90none", n, 0, 0.90)),
           ("queue", _queue(n)),
           ("allS", np.full(n, F_START, np.uint8)), ("allC", np.full(n, F_CONT, np.uint8)), ("allE", np.full(n, F_END, np.uint8)),
           ("none", np.zeros(n, np.uint8)),
           ("sliceE", _slice_edges(n, F_END, F_END, F_CONT)),        # an E on the first and the last item of every slice
           ("sliceS", _slice_edges(n, F_START, None, F_CONT))]       # an S on the first item of every slice only
    if n >= 6:
        out += [("span-unmatched", _span(n, 0)), ("span-matched", _span(n, F_END)), ("span-flush", _span(n, F_CONT))]
    # the empty bit where the rule can go wrong (byte records; the item form of these cases runs with the bit cleared)
    per = slice_items(n)
    t = 2 if n > 2 * per else 1
    spots = []
    if t * per - 1 < n and n > 1:
        spots.append(("empty-slice-last", t * per - 1))              # the unmatched range ends on a slice's last item
    if t * per < n:
        spots.append(("empty-slice-first", t * per))                 # ... on the next slice's first item
    if n > 1:
        spots.append(("empty-value-last", n - 1))                    # ... on the last item of the value
    for name, pos in spots:
        out.append((name, _empty_at(n, pos)))
    # single unmatched empty lines at a block border of ml_flags_kernel (where n does not reach it: at the end of the value)
    fl = np.zeros(n, np.uint8)
    for pos in (FLAG_BLOCK - 1, FLAG_BLOCK, n - 1):
        if 0 <= pos < n:
            fl[pos] = F_EMPTY
    if n:
        out.append(("empty-single", fl))
    return out


def cases(mode, large=False):
    """every case of the table for one mode; n_dyn alternates between "no device-side count" and "a count equal to max_items\""""
    k = 0
    for n in (LARGE_SIZES if large else SIZES):
        for name, fl in families(n, large):
            yield Case("%s/%d/%s" % (name, n, mode_name(mode)), mode, fl, None if k % 2 == 0 else n)
            k += 1


def find(family, n, mode, large=False):
    for c in cases(mode, large):
        if c.name == "%s/%d/%s" % (family, n, mode_name(mode)):
            return c
    raise KeyError((family, n, mode))


def line_table(flags, seed=0):
    """the offsets[n+1] + one separator byte table of a value whose line i is empty exactly where the empty bit is set, and 1..5 bytes
    long otherwise -> off (uint32[n + 1]); the value has off[n] bytes when it ends with a separator, off[n] - 1 when it does not"""
    n = len(flags)
    length = np.random.default_rng(1000 + seed + n).integers(1, 6, size=n, dtype=np.int64)
    length[(np.asarray(flags) & F_EMPTY) != 0] = 0
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(length + 1)
    return off.astype(np.uint32)


def forms(case, n=None):
    """-> [(form name, flags as the scan sees them, off or None, nbytes)] for the first n items of the case (default: all)"""
    fl = case.flags if n is None else case.flags[:n]
    n = len(fl)
    out = [("items", fl & 7, None, 0)]
    off = line_table(fl)
    out.append(("bytes-terminated", fl, off, int(off[n])))
    if n and not fl[n - 1] & F_EMPTY:       # (an unterminated empty last line does not exist: a trailing separator opens no line)
        out.append(("bytes-unterminated", fl, off, int(off[n]) - 1))
    return out


def walk_arrays(mode, flags, off=None, nbytes=0):
    """helpers/multiline_walk.walk with the records as a (records, 3) uint32 array, as the library lays them out -> (records, counts)"""
    from helpers import multiline_walk
    recs, counts = multiline_walk.walk(mode, flags, off, nbytes)
    return np.array(recs, dtype=np.uint32).reshape(-1, 3), counts


# ---------------------------------------------------------------------------------------------- reading the walk's item records
def groups(item_records):
    """the emissions behind item-form records: [(first item, last item, kind)], kind "matched" or "unmatched"; one HandleUnmatchLogs
    call is a record without LC_ML_RUN followed by its LC_ML_RUN records"""
    out = []
    for b, length, fl in item_records:
        if fl & REC_MATCHED:
            out.append([b, b + length - 1, "matched", fl])
        elif fl & REC_RUN:
            out[-1][1] = b
        else:
            out.append([b, b, "unmatched", fl])
    return [tuple(g) for g in out]


def queued_runs(item_records, n):
    """-> (runs that phase C must queue for phase D, 1 if the flush queues one more): an unmatched run is queued by the slice that ends it
    when its first item lies in an earlier slice; the flush's unmatched run is always queued (its records carry LC_ML_LAST in item form)"""
    per = slice_items(n)
    queued = flush = 0
    for first, last, kind, fl in groups(item_records):
        if kind != "unmatched":
            continue
        if fl & REC_LAST:
            flush = 1
        elif first // per < last // per:
            queued += 1
    return queued, flush


def slices_that_queue(item_records, n):
    """the slices whose phase C queues a run"""
    per = slice_items(n)
    return {last // per for first, last, kind, fl in groups(item_records)
            if kind == "unmatched" and not fl & REC_LAST and first // per < last // per}


def writer_of(item_records, k, n):
    """who writes record k of an item-form result: "C" (a slice's own pass), "D" (a queued run), "flush-matched" (thread 0 behind phase
    C) or "flush-run" (the flush's queued run)"""
    per = slice_items(n)
    at = 0
    for first, last, kind, fl in groups(item_records):
        size = 1 if kind == "matched" else last - first + 1
        if k < at + size:
            if fl & REC_LAST:
                return "flush-matched" if kind == "matched" else "flush-run"
            return "D" if kind == "unmatched" and first // per < last // per else "C"
        at += size
    raise IndexError(k)
