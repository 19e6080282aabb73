"""The record scan of the multiline processors (csrc/multiline_scan.hpp) past 8 192 items, on the CPU.

Two comparisons, in this order:
  1. tests/helpers/multiline_walk.walk -- one sequential pass over flag bytes -- against MultilineOracle.split on real lines and real
     regexes: the reference's own unit-test cases and buffers on either side of every slice-size switch.  This is what makes the walk a
     reference; lc_multiline_bounds_model cannot be one, it is the kernel's own code compiled for the host.
  2. lc_multiline_bounds_model against the walk on the case table of tests/helpers/multiline_scan_cases.py, whose flag bytes are chosen
     from the scan's geometry (tests/test_gpu_multiline_scan.py runs the same table through the kernels).
Two mutation checks show that the table can fail.  Everything is exact; there is no tolerance anywhere."""
import json
import os
import random

import numpy as np
import pytest

from helpers import multiline_scan_cases as T
from helpers import multiline_walk as W
from loongcollector_amd import multiline as ML
from oracle.multiline_oracle import MultilineOracle


@pytest.fixture(scope="module")
def vectors(golden_dir):
    with open(os.path.join(golden_dir, "multiline_vectors.json"), encoding="utf-8") as f:
        return json.load(f)


def _walk_equals_the_oracle(o, val, what):
    mode, flags, off = W.flags_and_table(o, val)
    recs, counts = W.walk(mode, flags, off, len(val))
    exp_recs, exp_counters = o.split(val)
    assert [(b, l, f & 1) for b, l, f in recs] == exp_recs, what
    assert counts[:3] == exp_counters and counts[3] == len(exp_recs), what
    # the flush's records, and those emitted while an unterminated last line is looked at, carry isLastLog; no other record does
    n = len(flags)
    if recs and not (mode & ML.ML_DISCARD):
        tail = off[n] == len(val) + 1
        for b, l, f in recs:
            if f & W.REC_LAST:
                assert tail or counts[4], what                      # (only the flush sets it on a terminated value)
    # the same walk with item records names the same ranges by item (an empty line at the end of an unmatched range is a rule of the
    # line splitter alone)
    if b"\n\n" in b"\n" + val + b"\n":
        return
    items, icounts = W.walk(mode, flags)
    assert icounts == counts, what
    assert [(off[b], exp_recs[k][1] if (f & W.REC_LAST and f & 1 and k == len(items) - 1) else off[b + c] - 1 - off[b], f & 1)
            for k, (b, c, f) in enumerate(items)] == exp_recs, what


def test_walk_reproduces_the_reference_unit_test_cases(vectors):
    values = ["\n".join(vectors["lines"][t] for t in c["in"]).encode("utf-8") for c in vectors["cases"]]
    for c, val in zip(vectors["cases"], values):
        _walk_equals_the_oracle(MultilineOracle(**c["config"]), val, c["cite"])
    # ... and every scan config on every one of those values, with and without a line feed at the end
    for config in W.SCAN_CONFIGS:
        o = MultilineOracle(**config)
        for val in values:
            _walk_equals_the_oracle(o, val, (config, val))
            _walk_equals_the_oracle(o, val + b"\n", (config, val))


def test_walk_empty_lines_last_and_runs():
    """the hand-made values of tests/test_multiline.py (empty lines at the end of unmatched ranges; LAST and RUN bits), on the walk"""
    for val in (b"BEGIN\n\n", b"BEGIN\nx\n\n", b"BEGIN\n", b"a\n\n", b"\n", b"\n\n", b"a\n\nb", b" a\n\nEND\n\n\n"):
        for cfg in ({"StartPattern": "BEGIN", "EndPattern": "END"}, {"EndPattern": "END"}, {"StartPattern": "BEGIN"},
                    {"ContinuePattern": r"\s+.*", "EndPattern": "END"}, {"StartPattern": "BEGIN", "ContinuePattern": r"\s+.*"}):
            _walk_equals_the_oracle(MultilineOracle(**cfg), val, (cfg, val))

    def bits(cfg, val):
        o = MultilineOracle(**cfg)
        mode, flags, off = W.flags_and_table(o, val)
        recs, _ = W.walk(mode, flags, off, len(val))
        return [(f >> 1) & 1 for _, _, f in recs], [bool(f & W.REC_LAST) for _, _, f in recs]
    # continue + end: a log that fails its end pattern goes to HandleUnmatchLogs as ONE run; the flush marks LAST (:288-298)
    assert bits({"ContinuePattern": r"\s+.*", "EndPattern": r"\}"}, b" a\n b\nnoise\n c\n d") == \
        ([0, 1, 1, 0, 1], [False, False, False, True, True])
    # start only: the record emitted while the LAST line is processed carries isLastLog (:174, :327-329), and so does the flush
    assert bits({"StartPattern": "S"}, b"S1\nx\nS2")[1] == [True, True]
    assert bits({"StartPattern": "S"}, b"S1\nx\nS2\n")[1] == [False, True]


@pytest.mark.parametrize("config", W.SCAN_CONFIGS)
def test_walk_against_the_oracle_on_either_side_of_the_slice_switches(config):
    """8 191 / 8 192 / 8 193 lines (slices of 16 become slices of 17), 8 704 / 8 705 (17 become 18), 20 000 (slices of 40): each buffer
    with one of the five biases of tests/test_multiline.py.  The scan's host model runs on the same buffers, so model, walk and oracle
    agree where the slice size changes."""
    rng = random.Random(5)
    o = MultilineOracle(**config)
    for k, n in enumerate((8191, 8192, 8193, 8704, 8705, 20000)):
        bias = W.BIASES[(k + W.SCAN_CONFIGS.index(config)) % len(W.BIASES)]
        val = W.biased_buffer(rng, n, bias)
        _walk_equals_the_oracle(o, val, (config, n, bias))
        mode, flags, off = W.flags_and_table(o, val)
        recs, counts = T.walk_arrays(mode, flags, off, len(val))
        got, got_counts = ML.bounds_model(mode, flags, off, len(val), raw=True)
        assert np.array_equal(got, recs) and W.counts_of_library(got_counts) == counts, (config, n, bias)


def _model_equals_the_walk(case):
    n = len(case.flags) if case.n_dyn is None else min(case.n_dyn, len(case.flags))
    for form, flags, off, nbytes in T.forms(case, n):
        recs, counts = T.walk_arrays(case.mode, flags, off, nbytes)
        got, got_counts = ML.bounds_model(case.mode, flags, off, nbytes, raw=True)
        assert W.counts_of_library(got_counts) == counts, (case.name, form)
        assert got.shape == recs.shape, (case.name, form)
        bad = np.flatnonzero((got != recs).any(axis=1))
        assert bad.size == 0, (case.name, form, "first wrong record", int(bad[0]), got[bad[0]].tolist(), recs[bad[0]].tolist())
        assert int(got_counts[4]) == 0 and int(got_counts[5]) == 0


@pytest.mark.parametrize("mode", T.MODES, ids=T.mode_name)
def test_scan_model_equals_the_walk_on_the_case_table(mode):
    ran = 0
    for case in T.cases(mode):
        _model_equals_the_walk(case)
        ran += 1
    assert ran >= 200


@pytest.mark.parametrize("mode", T.LARGE_MODES, ids=T.mode_name)
def test_scan_model_equals_the_walk_on_the_larger_sizes(mode):
    for case in T.cases(mode, large=True):
        _model_equals_the_walk(case)


# ---------------------------------------------------------------------------------------------- what the table covers
def test_table_covers_the_slice_sizes_and_the_full_queue():
    assert len(T.MODES) == 24 and {m & 7 for m in T.LARGE_MODES} == set(T.BASE_MODES)
    per = {n: T.slice_items(n) for n in T.SIZES + T.LARGE_SIZES}
    assert {16, 17, 18} <= set(per.values()) and max(per.values()) > 100
    assert (per[8192], T.slice_count(8192)) == (16, 512) and (per[8193], T.slice_count(8193)) == (17, 482)
    assert (per[8704], T.slice_count(8704)) == (17, 512) and (per[8705], T.slice_count(8705)) == (18, 484)
    assert (per[8208], T.slice_count(8208), 8208 % 17) == (17, 483, 14)                       # 16 * 513 items: a last slice that is short
    names = {name for name, _ in T.families(8192)}
    assert {"rand", "rand90C", "rand98C", "rand90none", "queue", "span-unmatched", "span-matched", "span-flush", "allS", "allC", "allE",
            "none", "sliceE", "sliceS", "empty-slice-last", "empty-slice-first", "empty-value-last", "empty-single"} <= names
    # the queue family: in continue + end every slice but the first queues a run, and the flush queues one more
    full = 0
    for n in T.SIZES + T.LARGE_SIZES:
        if n <= T.MIN_SLICE:
            continue
        large = n in T.LARGE_SIZES
        for mode in (6, 6 | ML.ML_FLUSH):
            case = T.find("queue", n, mode, large)
            recs, _ = W.walk(mode, case.flags & 7)
            queued, flush = T.queued_runs(recs, n)
            slices = T.slice_count(n)
            # exactly: every slice behind the first that reaches its 8th item (the one without the continue bit) ends a run.  That is
            # every slice but the first, except a LAST slice of fewer than 8 items (n = 17 and 257: one item)
            short_tail = 1 if 0 < n % per[n] < 8 else 0
            assert queued == slices - 1 - short_tail, (case.name, queued, slices)
            assert short_tail == (1 if n in (17, 257) else 0)
            assert queued >= slices - 1 or short_tail, (case.name, queued, slices)
            assert flush == (1 if mode & ML.ML_FLUSH and (n - 1) % per[n] != 7 else 0), case.name
            if slices == T.THREADS and T.slices_that_queue(recs, n) == set(range(1, T.THREADS)) and flush:
                full += 1                                           # 511 + 1 jobs: the whole queue jobs[kMlThreads + 1] but one entry
    assert full >= 2, full                                          # (n = 8192 and n = 8704)
    # the span family: ONE run inherited across every slice, ended unmatched (one queued run of n - 3 items), matched, or by the flush
    for n in (8192, 8705):
        recs, counts = W.walk(6, T.find("span-unmatched", n, 6).flags & 7)
        assert T.groups(recs)[-1][:3] == (3, n - 1, "unmatched") and T.queued_runs(recs, n) == (1, 0)
        recs, counts = W.walk(7, T.find("span-matched", n, 7).flags & 7)
        assert recs[-1] == (3, n - 3, W.REC_MATCHED)
        recs, counts = W.walk(3 | ML.ML_FLUSH, T.find("span-flush", n, 3 | ML.ML_FLUSH).flags & 7)
        assert recs[-1] == (3, n - 3, W.REC_MATCHED | W.REC_LAST) and counts[4:] == (1, 3)


# ---------------------------------------------------------------------------------------------- the table can fail
def _cases_that_differ(mode, sizes):
    """table cases (of the given sizes) on which the walk -- as patched by the caller -- and the scan's host model disagree"""
    out = []
    for case in T.cases(mode):
        if len(case.flags) not in sizes:
            continue
        for form, flags, off, nbytes in T.forms(case):
            recs, counts = T.walk_arrays(mode, flags, off, nbytes)
            got, got_counts = ML.bounds_model(mode, flags, off, nbytes, raw=True)
            if W.counts_of_library(got_counts) != counts or not np.array_equal(got, recs):
                out.append("%s %s" % (case.name, form))
    return out


def test_mutation_counting_the_empty_last_line_of_an_unmatched_range(monkeypatch):
    """a walk that lets HandleUnmatchLogs emit the empty last line of its range differs from the model on
    empty-slice-last/8193/CE bytes-terminated (and on others), and only on byte forms"""
    sizes = (257, 8193)
    assert _cases_that_differ(6, sizes) == []
    monkeypatch.setattr(W, "_unmatched_last", lambda flags, last, from_flush: last)
    differ = _cases_that_differ(6, sizes)
    assert "empty-slice-last/8193/CE bytes-terminated" in differ and "empty-slice-first/8193/CE bytes-unterminated" in differ
    assert "empty-single/257/CE bytes-terminated" in differ
    assert not [d for d in differ if d.endswith(" items")]


def test_mutation_forgetting_last_on_the_flush(monkeypatch):
    """a walk whose flush forgets LC_ML_LAST differs from the model on span-flush/8193/SC-flush items (and on others)"""
    sizes = (17, 8193)
    mode = 3 | ML.ML_FLUSH
    assert _cases_that_differ(mode, sizes) == []
    monkeypatch.setattr(W, "_last_bit", lambda emitter, n, tail: W.REC_LAST if (tail and emitter == n - 1) else 0)
    differ = _cases_that_differ(mode, sizes)
    assert "span-flush/8193/SC-flush items" in differ and "span-flush/17/SC-flush bytes-terminated" in differ
    assert "none/8193/SC-flush items" not in differ                # (nothing is under construction at the end: no flush)
