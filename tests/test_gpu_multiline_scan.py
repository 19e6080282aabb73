"""The record scan kernels of the multiline processors -- ml_flags_kernel and ml_bounds_kernel (csrc/multiline_kernel.hpp; the scan code is
csrc/multiline_scan.hpp) -- launched directly through lc_multiline_bounds_device on status bytes the tests choose: no match launches, no
regexes.  The case table (tests/helpers/multiline_scan_cases.py) comes from the scan's geometry: slices of 16, 17, 18, 32, 33 and 196
items, 512 busy threads, short last slices, a run queue jobs[kMlThreads + 1] with 511 + 1 entries, one run inherited across every slice,
the empty-line rule at slice and block borders.

Every comparison is bit-exact against tests/helpers/multiline_walk.walk -- one sequential pass, held against the oracle by
tests/test_multiline_walk.py -- never against the scan's host model alone.  Every tensor is GUARD entries longer than what the library is
told and pre-filled with a sentinel: status bytes behind the count hold LC_MATCH (a read past the count shows as records); d_flags behind
the count, records behind min(count, record_cap) and counts behind LC_ML_CNT_WORDS must keep theirs."""
import numpy as np
import pytest

from helpers import fresh_thread
from helpers import multiline_scan_cases as T
from helpers import multiline_walk as W
from loongcollector_amd import binding as B
from loongcollector_amd import multiline as ML

pytestmark = pytest.mark.gpu

GUARD = 64
SENT8 = 0xA5
SENT32 = -559038737               # 0xDEADBEEF as int32; no record word or counter of these tests has that value
PENDING_BYTE = 4                  # the transient byte of the backtracking launch (tests/test_gpu_bt_launch.py, bt_kernel.hpp kBtPending)
CNT_WORDS = 8                     # LC_ML_CNT_WORDS
CNT_RECORDS, CNT_OVERFLOW, CNT_GAVE_UP = 3, 4, 5


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert B.device_count() >= 1
    torch.cuda.set_device(0)
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def status_of(flags):
    """the three status arrays whose answers are the flag bits"""
    fl = np.asarray(flags, dtype=np.uint8)
    return np.stack([np.where(fl & (1 << k), B.LC_MATCH, B.LC_NOMATCH).astype(np.uint8) for k in range(3)])


class Inputs:
    """the device side of one launch: status bytes (3 x max_items, LC_MATCH behind them), the line table, the item count"""

    def __init__(self, torch, status, off=None, nbytes=0, n_dyn=None):
        self.torch = torch
        self.max_items = status.shape[1]
        host = np.full((3, self.max_items + GUARD), B.LC_MATCH, dtype=np.uint8)
        host[:, :self.max_items] = status
        self.d_status = torch.from_numpy(host).to("cuda:0")
        self.d_off = None
        if off is not None:
            table = np.full(len(off) + GUARD, SENT32, dtype=np.int32)
            table[:len(off)] = np.asarray(off, dtype=np.uint32).view(np.int32)
            self.d_off = torch.from_numpy(table).to("cuda:0")
        self.nbytes = nbytes
        self.n_dyn = n_dyn
        self.h_n = None
        if n_dyn is not None:
            self.h_n = np.full(4, SENT32, dtype=np.int32)
            self.h_n[:1] = np.array([n_dyn], dtype=np.uint32).view(np.int32)
        self.d_n = None if n_dyn is None else torch.from_numpy(self.h_n).to("cuda:0")
        self.n = self.max_items if n_dyn is None else min(n_dyn, self.max_items)      # the items the launch has to work on

    def run(self, mode, cap, pinned=False, null=(), counts=None, check=True):
        """one launch -> (status code, records written [min(count, cap), 3], counts[8], d_flags of the n items); the sentinels behind
        every extent are checked here"""
        torch = self.torch
        d_flags = torch.full((self.max_items + GUARD,), SENT8, dtype=torch.uint8, device="cuda:0")
        if pinned:
            recs = torch.empty((cap + GUARD, 3), dtype=torch.int32, pin_memory=True).fill_(SENT32)
        else:
            recs = torch.full((cap + GUARD, 3), SENT32, dtype=torch.int32, device="cuda:0")
        d_counts = torch.full((CNT_WORDS + GUARD,), SENT32, dtype=torch.int32, device="cuda:0") if counts is None else counts
        st = [None if k in null else self.d_status[k] for k in range(3)]
        rc = ML.bounds_device(mode, st[0], st[1], st[2], self.d_n, self.max_items, self.d_off, self.nbytes, d_flags, recs, cap, d_counts,
                              stream=_stream(torch), check=check)
        torch.cuda.synchronize()
        got_counts = d_counts.cpu().numpy()
        assert (got_counts[CNT_WORDS:] == SENT32).all(), "counts behind LC_ML_CNT_WORDS"
        got_counts = got_counts[:CNT_WORDS].view(np.uint32)
        flags = d_flags.cpu().numpy()
        assert (flags[self.n:] == SENT8).all(), "d_flags behind the item count"
        got = recs.cpu().numpy() if not pinned else recs.numpy().copy()
        written = min(int(got_counts[CNT_RECORDS]), cap)
        assert (got[written:] == SENT32).all(), "records behind min(count, record_cap)"
        if self.d_n is not None:
            assert np.array_equal(self.d_n.cpu().numpy(), self.h_n), "the item count is read, never written"
        return rc, got[:written].view(np.uint32), got_counts, flags[:self.n]


def _assert_equals_the_walk(got, got_counts, recs, counts, what, cap=None):
    assert W.counts_of_library(got_counts) == counts, (what, got_counts.tolist(), counts)
    want = recs if cap is None else recs[:cap]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, "first wrong record", int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def _run_case(torch, case):
    for form, flags, off, nbytes in T.forms(case):
        recs, counts = T.walk_arrays(case.mode, flags, off, nbytes)
        inp = Inputs(torch, status_of(flags), off, nbytes, case.n_dyn)
        cap = len(flags) + 1                                   # (no walk emits more than one record per item and one for the flush)
        for pinned in (False, True):
            rc, got, got_counts, d_flags = inp.run(case.mode, cap, pinned=pinned)
            what = (case.name, form, "pinned" if pinned else "device")
            assert rc == B.LC_OK, what
            _assert_equals_the_walk(got, got_counts, recs, counts, what)
            assert got_counts[CNT_OVERFLOW] == 0 and got_counts[CNT_GAVE_UP] == 0, what
            assert np.array_equal(d_flags, flags if off is not None else flags & 7), what     # ml_flags_kernel's own output


@pytest.mark.parametrize("mode", T.MODES, ids=T.mode_name)
def test_kernels_equal_the_walk_on_the_case_table(torch_dev, mode):
    """records in device memory and in pinned host memory, and all eight counters, for every case of the table up to 8 705 items in its
    three forms (item records; byte records of a terminated and of an unterminated value)"""
    ran = 0
    for case in T.cases(mode):
        _run_case(torch_dev, case)
        ran += 1
    assert ran >= 200


@pytest.mark.parametrize("mode", T.LARGE_MODES, ids=T.mode_name)
def test_kernels_equal_the_walk_on_the_larger_sizes(torch_dev, mode):
    """16 384, 16 385 and 100 003 items: slices of 32, 33 and 196"""
    for case in T.cases(mode, large=True):
        _run_case(torch_dev, case)


# ---------------------------------------------------------------------------------------------- the device-side count
CLAMP_CASES = [("rand", 257, 7 | ML.ML_FLUSH), ("rand90C", 8193, 6 | ML.ML_FLUSH), ("queue", 8192, 6 | ML.ML_FLUSH), ("span-flush", 8705, 3 | ML.ML_FLUSH),
               ("empty-value-last", 257, 6), ("rand", 17, 4 | ML.ML_FLUSH), ("allS", 1, 1 | ML.ML_FLUSH)]


@pytest.mark.parametrize("family,n,mode", CLAMP_CASES)
def test_device_side_count_below_equal_and_above_max_items(torch_dev, family, n, mode):
    """d_nitems NULL, equal to max_items, one below it, zero, and ABOVE it (clamped to max_items: the status bytes behind it all say
    "match" and would show as records).  The line table handed over ends with the counted items, as the split kernels leave it."""
    case = T.find(family, n, mode)
    for n_dyn in (None, n, n - 1, 0, n + 1, n + GUARD, 0xFFFFFFFF):
        n_eff = n if n_dyn is None else min(n_dyn, n)
        for form, flags, off, nbytes in T.forms(case, n_eff):
            recs, counts = T.walk_arrays(mode, flags, off, nbytes)
            inp = Inputs(torch_dev, status_of(case.flags), off, nbytes, n_dyn)         # max_items stays n
            assert inp.n == n_eff and inp.max_items == n
            rc, got, got_counts, d_flags = inp.run(mode, n + 1)
            assert rc == B.LC_OK
            _assert_equals_the_walk(got, got_counts, recs, counts, (case.name, form, n_dyn))
            assert np.array_equal(d_flags, flags if off is not None else flags & 7), (case.name, form, n_dyn)


def test_a_count_of_zero_under_257_items_of_status(torch_dev):
    """n_dyn = 0 with max_items = 257: two blocks of ml_flags_kernel and a scan that have nothing to do -- no flag byte, no record; "end
    alone" still reports its partial state"""
    for mode in T.MODES:
        inp = Inputs(torch_dev, np.full((3, 257), B.LC_MATCH, dtype=np.uint8), None, 0, 0)
        rc, got, got_counts, _ = inp.run(mode, 258)
        recs, counts = T.walk_arrays(mode, np.zeros(0, np.uint8))
        assert rc == B.LC_OK and counts == (0, 0, 0, 0, 1 if mode & 7 == 4 else 0, 0)
        _assert_equals_the_walk(got, got_counts, recs, counts, mode)
        assert got_counts[CNT_OVERFLOW] == 0 and got_counts[CNT_GAVE_UP] == 0


# ---------------------------------------------------------------------------------------------- record_cap
def test_record_cap_cuts_phase_c_phase_d_and_the_flush(torch_dev):
    """record_cap = 0, 1, count - 1, count, count + 1 on a queue case and on a span case: the first record_cap records are the walk's,
    nothing is written behind them, counts[LC_ML_CNT_RECORDS] still says the full number.  Over the cases, the first record that was cut
    belonged to a slice's own pass (phase C), to a queued run (phase D), to the flush's queued run and to the flush's matched record."""
    cut = set()
    for family, n, mode in (("queue", 8192, 6), ("queue", 8192, 6 | ML.ML_FLUSH), ("queue", 8704, 6 | ML.ML_FLUSH), ("span-unmatched", 8193, 6),
                            ("span-flush", 8705, 3 | ML.ML_FLUSH), ("span-flush", 257, 1 | ML.ML_FLUSH), ("span-matched", 8192, 7)):
        case = T.find(family, n, mode)
        item_recs, _ = W.walk(mode, case.flags & 7)
        for form, flags, off, nbytes in T.forms(case):
            recs, counts = T.walk_arrays(mode, flags, off, nbytes)
            count = counts[3]
            assert count == len(item_recs) >= 2
            inp = Inputs(torch_dev, status_of(flags), off, nbytes, None)
            for cap in (0, 1, count - 1, count, count + 1):
                for pinned in (False, True):
                    rc, got, got_counts, _ = inp.run(mode, cap, pinned=pinned)
                    assert rc == B.LC_OK
                    _assert_equals_the_walk(got, got_counts, recs, counts, (case.name, form, cap, pinned), cap=cap)
                if cap < count:
                    cut.add(T.writer_of(item_recs, cap, n))
    assert cut == {"C", "D", "flush-run", "flush-matched"}, cut


# ---------------------------------------------------------------------------------------------- status bytes
@pytest.mark.parametrize("family,n,mode", [("rand", 257, 7 | ML.ML_FLUSH), ("rand", 8193, 7 | ML.ML_FLUSH), ("rand90C", 8192, 6 | ML.ML_FLUSH),
                                           ("sliceS", 8705, 3 | ML.ML_FLUSH), ("sliceE", 8193, 5), ("rand", 256, 4 | ML.ML_FLUSH),
                                           ("rand", 255, 1)])
def test_a_null_status_array_answers_no_match(torch_dev, family, n, mode):
    """NULL for a pattern that is not in use changes nothing (what the processors pass); NULL for one that is in use behaves as "no item
    matches it\""""
    case = T.find(family, n, mode)
    unused = tuple(k for k in range(3) if not mode & (1 << k))
    for null in [unused] + [unused + (k,) for k in range(3) if mode & (1 << k)] + [(0, 1, 2)]:
        keep = np.uint8(0xFF)
        for k in null:
            if mode & (1 << k):
                keep &= np.uint8(~(1 << k) & 0xFF)
        for form, flags, off, nbytes in T.forms(case):
            recs, counts = T.walk_arrays(mode, flags & keep, off, nbytes)
            rc, got, got_counts, d_flags = Inputs(torch_dev, status_of(flags), off, nbytes, n).run(mode, n + 1, null=null)
            assert rc == B.LC_OK
            _assert_equals_the_walk(got, got_counts, recs, counts, (case.name, form, null))
            clear = np.uint8(0xFF)
            for k in null:
                clear &= np.uint8(~(1 << k) & 0xFF)
            assert np.array_equal(d_flags, (flags if off is not None else flags & 7) & clear), (case.name, form, null)


def _undecided(status, n):
    """LC_OVERFLOW / LC_GAVE_UP at items 0, 63, 64, 255, 256 and n - 1, in one, two or all three arrays of the same item -> the status
    bytes, the number of each"""
    st = status.copy()
    plan = [(0, {0: B.LC_OVERFLOW}), (63, {0: B.LC_GAVE_UP, 1: B.LC_GAVE_UP}), (64, {0: B.LC_OVERFLOW, 1: B.LC_OVERFLOW, 2: B.LC_OVERFLOW}),
            (255, {2: B.LC_GAVE_UP}), (256, {1: B.LC_OVERFLOW, 2: B.LC_GAVE_UP}), (n - 1, {0: B.LC_GAVE_UP, 1: B.LC_GAVE_UP, 2: B.LC_GAVE_UP})]
    placed = {}
    for item, rows in plan:
        if 0 <= item < n and item not in placed:
            placed[item] = rows
            for k, v in rows.items():
                st[k, item] = v
    over = sum(v == B.LC_OVERFLOW for rows in placed.values() for v in rows.values())
    gave = sum(v == B.LC_GAVE_UP for rows in placed.values() for v in rows.values())
    return st, over, gave


def _flags_of_status(st, empty_bits):
    return ((st[0] == B.LC_MATCH) * 1 + (st[1] == B.LC_MATCH) * 2 + (st[2] == B.LC_MATCH) * 4).astype(np.uint8) | empty_bits


@pytest.mark.parametrize("family,n,mode", [("allC", 257, 6 | ML.ML_FLUSH), ("rand", 8193, 7 | ML.ML_FLUSH), ("allS", 8192, 1 | ML.ML_FLUSH),
                                           ("allE", 8208, 4), ("rand", 17, 3), ("sliceE", 8705, 5 | ML.ML_FLUSH)])
def test_undecided_answers_are_counted_and_read_as_no_match(torch_dev, family, n, mode):
    case = T.find(family, n, mode)
    for form, flags, off, nbytes in T.forms(case):
        st, over, gave = _undecided(status_of(flags), n)
        assert over >= 1 and gave >= 2
        want_flags = _flags_of_status(st, flags & W.F_EMPTY if off is not None else np.uint8(0))
        recs, counts = T.walk_arrays(mode, want_flags, off, nbytes)
        rc, got, got_counts, d_flags = Inputs(torch_dev, st, off, nbytes, None).run(mode, n + 1)
        assert rc == B.LC_OK
        _assert_equals_the_walk(got, got_counts, recs, counts, (case.name, form))
        assert (int(got_counts[CNT_OVERFLOW]), int(got_counts[CNT_GAVE_UP])) == (over, gave), (case.name, form)
        assert np.array_equal(d_flags, want_flags)


def test_other_status_bytes_set_no_flag_and_no_counter(torch_dev):
    """the transient pending byte of the backtracking launch, and every other value a status byte can hold: no flag, no counter"""
    n, mode = 8193, 7 | ML.ML_FLUSH
    case = T.find("rand", n, mode)
    for form, flags, off, nbytes in T.forms(case):
        st = status_of(flags)
        rng = np.random.default_rng(11)
        others = np.array([PENDING_BYTE] + list(range(5, 256)), dtype=np.uint8)
        at = rng.random((3, n)) < 0.3
        at[:, [0, 63, 64, 255, 256, n - 1]] = True
        fill = others[rng.integers(0, len(others), size=(3, n))]
        fill[:, [0, 63, 64, 255, 256, n - 1]] = PENDING_BYTE
        st[at] = fill[at]
        want_flags = _flags_of_status(st, flags & W.F_EMPTY if off is not None else np.uint8(0))
        recs, counts = T.walk_arrays(mode, want_flags, off, nbytes)
        rc, got, got_counts, d_flags = Inputs(torch_dev, st, off, nbytes, n).run(mode, n + 1)
        assert rc == B.LC_OK
        _assert_equals_the_walk(got, got_counts, recs, counts, form)
        assert got_counts[CNT_OVERFLOW] == 0 and got_counts[CNT_GAVE_UP] == 0
        assert np.array_equal(d_flags, want_flags)


def test_counters_of_a_second_launch_hold_nothing_of_the_first(torch_dev):
    """two launches back to back on one stream into ONE counts tensor (no synchronisation between them): the first with undecided
    items, the second without"""
    torch = torch_dev
    n, mode = 8193, 6 | ML.ML_FLUSH
    first = T.find("allC", n, mode)
    second = T.find("none", n, mode)
    st, over, gave = _undecided(status_of(first.flags), n)
    assert over and gave
    a, b = Inputs(torch, st), Inputs(torch, status_of(second.flags))
    d_counts = torch.full((CNT_WORDS + GUARD,), SENT32, dtype=torch.int32, device="cuda:0")
    bufs = []
    for inp in (a, b):
        d_flags = torch.full((n + GUARD,), SENT8, dtype=torch.uint8, device="cuda:0")
        recs = torch.full((n + 1 + GUARD, 3), SENT32, dtype=torch.int32, device="cuda:0")
        ML.bounds_device(mode, inp.d_status[0], inp.d_status[1], inp.d_status[2], None, n, None, 0, d_flags, recs, n + 1, d_counts,
                         stream=_stream(torch))
        bufs.append(recs)
    torch.cuda.synchronize()
    got_counts = d_counts.cpu().numpy()
    assert (got_counts[CNT_WORDS:] == SENT32).all()
    got_counts = got_counts[:CNT_WORDS].view(np.uint32)
    recs, counts = T.walk_arrays(mode, second.flags)
    assert counts == (n, n, 0, n, 0, 0)
    assert got_counts[CNT_OVERFLOW] == 0 and got_counts[CNT_GAVE_UP] == 0
    _assert_equals_the_walk(bufs[1].cpu().numpy()[:counts[3]].view(np.uint32), got_counts, recs, counts, "second launch")
    # (the first launch's records are whole too: all items continue, two of them undecided)
    first_recs, first_counts = T.walk_arrays(mode, _flags_of_status(st, np.uint8(0)))
    assert np.array_equal(bufs[0].cpu().numpy()[:first_counts[3]].view(np.uint32), first_recs)


def test_argument_errors_launch_nothing(torch_dev):
    """LC_ERR_ARG for NULL counts, for NULL d_flags with max_items > 0 and for NULL records with record_cap > 0 -- before any kernel"""
    torch = torch_dev
    n = 33
    st = torch.full((3, n + GUARD), B.LC_MATCH, dtype=torch.uint8, device="cuda:0")
    d_flags = torch.full((n + GUARD,), SENT8, dtype=torch.uint8, device="cuda:0")
    recs = torch.full((n + 1 + GUARD, 3), SENT32, dtype=torch.int32, device="cuda:0")
    counts = torch.full((CNT_WORDS + GUARD,), SENT32, dtype=torch.int32, device="cuda:0")
    B.launched_kernels()
    for fl, rec, cap, cnt in ((d_flags, recs, n + 1, None), (None, recs, n + 1, counts), (d_flags, None, 1, counts), (None, None, n, None)):
        rc = ML.bounds_device(1 | ML.ML_FLUSH, st[0], None, None, None, n, None, 0, fl, rec, cap, cnt, stream=_stream(torch), check=False)
        assert rc == B.LC_ERR_ARG
        assert B.launched_kernels() == ""
    torch.cuda.synchronize()
    assert (d_flags == SENT8).all() and (recs == SENT32).all() and (counts == SENT32).all()
    # the arguments that ARE allowed to be NULL: no d_flags for no items, no records for no capacity
    rc = ML.bounds_device(1 | ML.ML_FLUSH, None, None, None, None, 0, None, 0, None, None, 0, counts, stream=_stream(torch), check=False)
    torch.cuda.synchronize()
    assert rc == B.LC_OK and B.launched_kernels().count("ml_bounds_kernel") == 1
    assert counts.cpu().numpy()[:CNT_WORDS].tolist() == [0] * CNT_WORDS and (counts[CNT_WORDS:] == SENT32).all()
    rc = ML.bounds_device(1 | ML.ML_FLUSH, st[0], None, None, None, n, None, 0, d_flags, None, 0, counts, stream=_stream(torch), check=False)
    torch.cuda.synchronize()
    kernels = B.launched_kernels()
    assert rc == B.LC_OK and "ml_flags_kernel" in kernels and "ml_bounds_kernel" in kernels
    want = W.walk(1 | ML.ML_FLUSH, [W.F_START] * n)[1]            # all start: n - 1 logs closed by the next start, the last by the flush
    assert want == (n, 0, n, n, 1, n - 1)
    assert W.counts_of_library(counts.cpu().numpy()[:CNT_WORDS]) == want and counts.cpu().numpy()[4:6].tolist() == [0, 0]
    assert (recs == SENT32).all() and (d_flags[:n] == W.F_START).all() and (d_flags[n:] == SENT8).all()


# ---------------------------------------------------------------------------------------------- the whole trip
def test_second_attempt_of_the_split_trip_when_the_first_record_guess_is_too_small():
    """boundsAndFetch (csrc/multiline_device.hip) starts a runner thread with room for 1 024 records; 3 000 unmatched one-byte lines need
    3 000, so the first split launches the scan twice, the second -- with the guess learned -- once"""
    from oracle.multiline_oracle import MultilineOracle
    cfg = {"StartPattern": "BEGIN"}
    val = b"\n".join([b"x"] * 3000)
    m = ML.Multiline(**cfg)

    def body():
        B.launched_kernels()
        first = m.split_raw(val)
        k1 = B.launched_kernels()
        second = m.split_raw(val)
        k2 = B.launched_kernels()
        return first, k1, second, k2, m.split(val)

    first, k1, second, k2, plain = fresh_thread.run(body)
    # (the launch log folds duplicate names; boundsAndFetch notes the repeated scan under a name of its own)
    assert k1.count("ml_bounds_kernel") == 2 and "ml_bounds_kernel[second attempt]" in k1 and k1.count("ml_flags_kernel") == 1, k1
    assert k2.count("ml_bounds_kernel") == 1 and "second attempt" not in k2 and k2.count("ml_flags_kernel") == 1, k2
    o = MultilineOracle(**cfg)
    exp_recs, exp_counters = o.split(val)
    assert len(exp_recs) == 3000 and plain == (exp_recs, exp_counters)
    mode, flags, off = W.flags_and_table(o, val)
    walk_recs, _ = W.walk(mode, flags, off, len(val))
    assert first == second == walk_recs
    assert [(b, l, f & 1) for b, l, f in first] == exp_recs


@pytest.mark.parametrize("config", W.SCAN_CONFIGS)
def test_device_trip_past_the_slice_switches(config):
    """the whole trip (upload, split kernels, status launches, flags, scan) on one buffer of 8 193 lines (slices of 17) and one of 8 705
    (slices of 18), against the oracle and the walk"""
    import random
    from oracle.multiline_oracle import MultilineOracle
    rng = random.Random(78)
    o = MultilineOracle(**config)
    m = ML.Multiline(**config)
    for k, n in enumerate((8193, 8705)):
        bias = W.BIASES[(k + W.SCAN_CONFIGS.index(config)) % len(W.BIASES)]
        val = W.biased_buffer(rng, n, bias)
        assert m.split(val) == o.split(val), (config, n, bias)
        mode, flags, off = W.flags_and_table(o, val)
        walk_recs, _ = W.walk(mode, flags, off, len(val))
        assert m.split_raw(val) == walk_recs, (config, n, bias)
