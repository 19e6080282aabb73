"""Deferred capture stamps of the one-stamp pair kernel (csrc/tdfa_stream_kernel.hpp kLabDeferStamps: what the compact 512-lane
kernel runs with LC_TDFA_DEFER_STAMPS=1).  The walk -- a queue of two events per lane, the wave's flush as soon as some lane holds
two, the flush in front of a chunk's settled DOUBLEs, the flush at the end of the line -- is restated store for store in
tests/helpers/deferred_stamps.py DeferredPair1Wave and pinned here against the stamp-per-pair walk (TdfaPair1Interp) and the oracle:
the same captures whatever the other lanes of the wave make the queue do.  The kernel itself meets the oracle in
tests/test_gpu_deferred_stamps.py."""
import json
import os

import numpy as np
import pytest

from loongcollector_amd import binding as B, corpus
from oracle.oracle import OracleRegex
from tests.helpers.deferred_stamps import DeferredPair1Wave

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 130]
# adjacent one-byte fields (a stamp on every byte: three and four real stamps of one lane in an 8-byte chunk, DOUBLE entries) ...
ONE_BYTE_FIELDS = rb"(\w)(\w)(\w)(\w)(\w)(\w)(\w)(\w)(\w) (\d*)(.*)"
# ... and a repeated group of them: the SAME registers are stamped again two bytes on, so a DOUBLE's second register has a plain
# stamp of an earlier iteration waiting in the queue when its chunk is settled
REPEATED_FIELDS = rb"(?:(\w)(\d?))*"


def _force_pair1(monkeypatch):
    monkeypatch.setenv("LC_TDFA_PAIR", "2")
    monkeypatch.setenv("LC_TDFA_COMPACT", "512")


def _wave(rx):
    blob = rx.table(B.LC_TABLE_TDFA_WIDE_BLOB, np.uint32)
    assert blob is not None and int(blob[7]) and int(blob[int(blob[7]) // 4 + 4]) == 1, "no one-stamp pair table"
    return DeferredPair1Wave(rx)


def _oracle(pattern, lines):
    data = np.frombuffer(b"".join(lines), np.uint8)
    length = np.array([len(s) for s in lines], np.int64)
    off = np.zeros(len(lines), np.int64)
    off[1:] = np.cumsum(length)[:-1]
    caps, status = OracleRegex(pattern).fullmatch_batch(data, off, length)
    return [[int(v) for v in caps[i]] if status[i] else None for i in range(len(lines))]


def _check(w, lines, want, heads, tag):
    """the wave walk, in waves of up to 64 lines, against `want` and against the stamp-per-pair walk of every line alone"""
    stats = {"flushes": 0, "max_real": 0, "double_flushes": 0, "doubles": 0}
    for head in heads:
        for at in range(0, len(lines), 64):
            part = lines[at:at + 64]
            w.doubles = 0
            got = w.walk_wave(part, head=head)
            for k, s in enumerate(part):
                assert got[k] == want[at + k], (tag, head, at + k, s[:60])
                assert got[k] == w.fullmatch_pair1(s, head=head), (tag, head, at + k, s[:60])
            stats["flushes"] += w.flushes
            stats["max_real"] = max(stats["max_real"], w.max_real_in_chunk)
            stats["double_flushes"] += w.double_flushes
    return stats


@pytest.mark.parametrize("kind", ["A", "B"])
def test_deferred_walk_on_the_bench_corpus_every_alignment(kind, monkeypatch):
    _force_pair1(monkeypatch)
    pattern = corpus.REGEX_A if kind == "A" else corpus.REGEX_B
    w = _wave(B.GpuRegex(pattern))
    data, off, length = corpus.apache_batch(96, kind, poison_every=7, empty_every=3)
    lines = [bytes(data[off[i]:off[i] + length[i]]) for i in range(96)]
    # every length at which a chunk, a stage or the line ends: prefixes of a corpus line (they do not match: the walk and the
    # status still have to agree) and lines of the format cut to size in their last, free field
    lines += [lines[0][:n] for n in LENGTHS]
    stem = b'1.2.3.4 - u [10/Oct/2026:13:55:36 +0000] "GET /a HTTP/1.1" 200 5 "-" "'
    lines += [stem + b"x" * (n - len(stem) - 1) + b'"' for n in LENGTHS if n > len(stem)]
    want = _oracle(pattern, lines)
    assert sum(x is not None for x in want) > 64
    stats = _check(w, lines, want, range(16), kind)
    assert stats["flushes"] > 0


def test_three_and_four_real_stamps_of_one_lane_in_one_chunk(monkeypatch):
    _force_pair1(monkeypatch)
    w = _wave(B.GpuRegex(ONE_BYTE_FIELDS))
    # (the fixture's start registers are derived from one another: a chain of derive words, applied behind the walk)
    assert len(w.derive) > 0 and {a for _, a, _ in w.derive} & {b for b, _, _ in w.derive}, w.derive
    lines = [b"abcdefghi 123 rest", b"abcdefghi ", b"abcdefghi 1", b"abcdefgh", b"abcdefghij 1", b"", b"a", b"abcdefghi 12345678901234567890 x"]
    lines += [b"abcdefghi " + b"7" * (n - 10) for n in LENGTHS if n >= 10] + [b"abcdefghi 1"[:n] for n in (0, 1, 7, 8, 9)]
    want = _oracle(ONE_BYTE_FIELDS, lines)
    assert want[0] is not None and want[3] is None
    seen = set()
    for head in range(16):
        # (alone in its wave, and with the others: the queue of a lane is flushed by what the other lanes hold)
        for part in ([lines[0]], [lines[1]], lines):
            st = _check(w, part, [want[lines.index(s)] for s in part], [head], "fields")
            seen.add(st["max_real"])
    assert 3 in seen and 4 in seen, seen


def test_a_double_meets_a_pending_stamp_of_its_register(monkeypatch):
    _force_pair1(monkeypatch)
    w = _wave(B.GpuRegex(REPEATED_FIELDS))
    lines = [b"a1b2c3d4e5", b"111a1a1", b"b1xxaa", b"111b1xa11", b"abababab", b"11ccxb1b1xc", b"b1xx,aa", b"111a;a1", b"", b"a", b"a1",
             b"1a2b3c4d5e6f7g8h9i0j1k2l3m4n5o6p7q8r9s0t"]
    lines += [(b"a1bc2" * 30)[:n] for n in LENGTHS]
    want = _oracle(REPEATED_FIELDS, lines)
    stats = _check(w, lines, want, range(16), "repeated")
    assert stats["double_flushes"] > 0, stats


def test_deferred_walk_on_the_golden_patterns_that_take_a_pair_table(monkeypatch):
    _force_pair1(monkeypatch)
    with open(os.path.join(GOLDEN, "regex_golden.json"), encoding="utf-8") as f:
        golden = json.load(f)
    took = checked = 0
    for c in golden["cases"]:
        try:
            rx = B.GpuRegex(c["p"].encode("latin-1"))
        except B.RegexUnsupportedError:
            continue
        if rx.info()["engine"] != B.LC_ENGINE_TDFA:
            continue
        blob = rx.table(B.LC_TABLE_TDFA_WIDE_BLOB, np.uint32)
        if blob is None or not int(blob[7]) or int(blob[int(blob[7]) // 4 + 4]) != 1:
            continue
        w = DeferredPair1Wave(rx)
        took += 1
        subs = [s.encode("latin-1") for s, _ in c["subs"]]
        want = [None if x is None else [int(v) for v in x[2:]] for _, x in c["subs"]]   # (the vectors carry group 0 first)
        _check(w, subs, want, range(16), c["p"])                # (against the vectors AND the stamp-per-pair walk, every alignment)
        checked += 16 * len(subs)
    assert took >= 20 and checked >= 16 * 500, (took, checked)
