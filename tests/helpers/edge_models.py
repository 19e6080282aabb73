"""Plain restatements of the small kernels around the match kernels (split, length scheduler, span filter), fast enough for the
buffer sizes where those kernels' geometry edges lie.  tests/test_edge_models.py holds each of them to the existing per-byte
oracles; tests/test_gpu_edge_kernels.py holds the kernels to them."""
import numpy as np

from loongcollector_amd.binding import LC_GAVE_UP, LC_MATCH, LC_NOMATCH, LC_OVERFLOW
from oracle.oracle import OracleRegex


def split_table_from_hits(hits, nbytes, terminated):
    """The offsets[n+1] table of a buffer whose separators sit at the sorted positions `hits`: every separator closes a line, an
    unterminated tail is one more line whose closing entry is nbytes + 1 (len[i] = off[i+1] - off[i] - 1).  uint32, as on the device"""
    hits = np.asarray(hits, dtype=np.uint64)
    if nbytes == 0:
        return np.zeros(1, dtype=np.uint32)
    parts = [np.zeros(1, dtype=np.uint64), hits + np.uint64(1)]
    if not terminated:
        parts.append(np.array([nbytes + 1], dtype=np.uint64))
    return np.concatenate(parts).astype(np.uint32)


def split_table_np(buf, split_char=10):
    """oracle.split_oracle.split_table without the per-byte loop"""
    arr = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf, dtype=np.uint8)
    n = int(arr.shape[0])
    hits = np.flatnonzero(arr == split_char)
    return split_table_from_hits(hits, n, n > 0 and int(arr[n - 1]) == split_char)


def sched_bucket(length):
    """sched_kernel.hpp schedBucket: 32-byte length classes, longest first, everything from 8160 bytes up in bucket 0"""
    return 255 - np.minimum(np.asarray(length, dtype=np.int64) >> 5, 255)


def span_filter_model(lines, status, caps, rules):
    """lc_span_filter_device restated.  lines: [(offset, line bytes)], status: uint8[n], caps: int32[n, 2G] (offsets inside the line,
    -1 for a group that did not take part), rules: [(pattern, 1-based group)].
    -> (counts [lines, survivors, parser did not match, undecided], {line: row [line, offset, length, 2G capture offsets]})"""
    compiled = [(OracleRegex(p), g) for p, g in rules]
    counts = [len(lines), 0, 0, 0]
    rows = {}
    for i, (o, line) in enumerate(lines):
        st = int(status[i])
        if st == LC_NOMATCH:
            counts[2] += 1
        elif st in (LC_OVERFLOW, LC_GAVE_UP):
            counts[3] += 1
        if st != LC_MATCH:
            continue
        keep = True
        for rx, g in compiled:
            b, e = int(caps[i, 2 * (g - 1)]), int(caps[i, 2 * (g - 1) + 1])
            value = line[b:e] if b >= 0 else b""    # boost's {last, last}: a group that did not take part has the empty value
            if rx.fullmatch(value) is None:
                keep = False
                break
        if keep:
            counts[1] += 1
            rows[i] = [i, o, len(line)] + [int(x) for x in caps[i]]
    return counts, rows
