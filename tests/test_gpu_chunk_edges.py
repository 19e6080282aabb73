"""The engines that walk one value per wavefront (nfa_match_kernel, nfa_wide_kernel, tdfa_wave_kernel) and their lane-per-value
neighbours (tdfa_l2_kernel, nfa_decide_kernel, nfa_dfs_kernel, bt_match_kernel) at 256-byte chunk edges and result edges: the corpus of
tests/helpers/chunk_edges.py -- values in which a run ends, the value ends, a capture is stamped, the value dies, the automaton
absorbs, a search starts or resumes on a chosen byte, for every alignment of the value's first byte -- through every row of its
instantiation table, against the oracle, bit for bit.  Each of those decisions is a comparison against a chunk border, the end of
the value or the start offset: a slip in one of them misparses only the values whose event sits on that byte for that alignment.
tests/test_chunk_edges.py says on the CPU that the corpus holds those values and that the tables are right.

The lazy rows put a partial automaton in front of a thread-list program (both walks): the `lazy` family's `miss` cases leave it on a
chosen byte and must come back with the thread-list kernels' answer, `log` and `threads` run the decided path alone.  The GLOBAL
instantiation of nfa_match_kernel runs in one child process (LC_NFA_GLOBAL_KB is read once per process).

The chain rows put the 65th / 129th live thread on a chosen byte (families over64 / over128 / over64s): nfa_match_kernel hands the
value to nfa_wide_kernel, that one to nfa_decide_kernel, the `at_cap` controls in the same workgroups stay where they are, and
lc_decide_stats counts exactly the values that had to be sent on.  Rows nfa-ns64 / 128 / 320 run the log family with 64, 128 and 320
capture slots, rows runcap-* put the end of a run capture (run_capture_kernel) on a chosen byte for all 16 residues.  The handles of
lazy-wave and lazy-lane are launched, trained again on their misses and launched once more: a rebuilt automaton behind one handle.

Row nfa-atomic-edges puts the atomic instantiation's ordered commit pass (nfaAtomicStep) on chosen bytes (families alog, acommit, aquasi),
rows achain-* each of its overflow exits -- the 65th survivor, the vector step's 65th thread, the 7th membership, the 65th closed
segment, the 11th work entry -- with controls exactly at the cap, as `at_cap` variants or as a sibling family in the same row:
nfa_decide_kernel takes what is given up, no wide kernel runs, lc_decide_stats counts exactly the values sent on.  Two tests of the
bounds: values of 2^17 - 3, 2^17 - 2 and 2^17 bytes, and a pattern with 255 atomic instances whose last one commits.

Every launch keeps four sentinel rows in front of and behind the capture table and the status bytes (tests/helpers/guarded_launch.py)
and runs in both forms: (off, len), where filler gives each line its residue, and off[n + 1] with a separator byte."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from loongcollector_amd import binding as B
from tests.helpers import chunk_edges as ce
from tests.helpers.chunk_edge_launch import batch_of, cut as _cut, decide_stats, differing, launch as _launch, make_batches, rows as _rows
from tests.helpers.guarded_launch import STATUS_SENTINEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def batches(torch_dev):
    """(family, walk, copies) -> the corpus on the device in both forms and the oracle's rows for it (tests/helpers/chunk_edge_launch.py)"""
    return make_batches(torch_dev)


def _copies(row, n0):
    return -(-row.min_n // n0) if row.min_n else 1


def _compare(batch, got_caps, got_status, exp_caps, exp_status, where, listed=None, status_fill=STATUS_SENTINEL):
    """the rows of the `listed` values (default: all) against the oracle's; every other row still holds its sentinels"""
    n, first = differing(batch, got_caps, got_status, exp_caps, exp_status, where, listed, status_fill)
    if n:
        pytest.fail(first)


def _ran(row, names, where, family=None):
    assert ce.ran(row, names), (where, names)                                  # (the instantiation the row names is what ran)
    if row.id == "nfa-wide-first":
        assert "nfa_match_kernel" not in names, (where, names)
    if row.id == "l2-lane":
        assert "tdfa_l2_kernel:wave" not in names, (where, names)
    has, has_not = ce.CHAIN.get((row.id, family), ((), ()))                    # the chain's hand-offs: who took part, who did not
    assert set(has) <= set(names) and not set(has_not) & set(names), (where, names)


def _sent_on(row, family, batch, names, where, listed=None):
    """lc_decide_stats right behind a launch of a chain row: nfa_decide_kernel settled exactly the values of the launch in which a
    thread list outgrows the last thread-list kernel -- an `at_cap` value sent on would be counted -- and gave none up.  A row whose
    program cannot outgrow it queues no decide launch at all (asserted by _ran): nothing was sent on."""
    if (row.id, family) not in ce.CHAIN:
        return
    c, fam = batch["corpus"], batch["corpus"].family
    over = [fam.overflows(c.cases[int(i) % batch["n0"]]) for i in (range(batch["n"]) if listed is None else listed)]
    if family in ce.SIBLING:                                                   # (the cap is the pattern's: the controls are the sibling family's)
        assert sum(over) == len(over), where
    elif family in ce.SIBLING.values():
        assert sum(over) == 0, where
    else:
        assert 0 < sum(over) < len(over), where                                # (overflowing values and controls in every launch)
    if (row.id, family) in ce.DECIDES:
        assert decide_stats() == (sum(over), 0), (where, decide_stats(), sum(over))
    else:
        assert "nfa_decide_kernel" not in names, (where, names)


@pytest.mark.parametrize("row", ce.ROWS, ids=[r.id for r in ce.ROWS])
def test_corpus_through_each_engine(torch_dev, monkeypatch, batches, row):
    ce.set_env(monkeypatch, row)
    for family in row.families:
        rx = ce.compile_row(row, family)
        batch = batches(family, row.walk, _copies(row, len(ce.generate(family, row.walk).cases)))
        assert rx.groups == batch["G"] and (not row.min_n or ce.UNSTAGED_ABOVE < batch["n"] <= 65536)
        for form in ("len", "sep"):
            where = "%s, %s, %s form" % (row.id, family, form)
            caps, status, names = _launch(torch_dev, row, rx, batch, form)
            _ran(row, names, where, family)
            _compare(batch, caps, status, batch["caps"], batch["status"], where)
            _sent_on(row, family, batch, names, where)


@pytest.mark.parametrize("row", ce.SEARCH_ROWS, ids=[r.id for r in ce.SEARCH_ROWS])
def test_resumed_searches_at_chunk_edges(torch_dev, monkeypatch, batches, row):
    """every value of the search families, each search resumed at its own offset (the resume cases: p - 1, p, p + 1; all others: 0),
    against OracleRegex.search(line, from)"""
    ce.set_env(monkeypatch, row)
    for family in (f for f in row.families if ce.FAMILIES[f].search):
        rx = ce.compile_row(row, family)
        batch = batches(family, row.walk)
        c, o = batch["corpus"], batch["oracle"]
        frm = c.frm()
        assert (frm > 0).sum() > 1000
        exp_caps, exp_status = _rows(c.family, [o.search(k.line, int(f)) for k, f in zip(c.cases, frm)], batch["G"])
        for form in ("len", "sep"):
            where = "%s, %s, resumed, %s form" % (row.id, family, form)
            caps, status, names = _launch(torch_dev, row, rx, batch, form, frm=frm)
            _ran(row, names, where)
            _compare(batch, caps, status, exp_caps, exp_status, where)


@pytest.mark.parametrize("row", ce.ROWS, ids=[r.id for r in ce.ROWS])
def test_result_edges(torch_dev, monkeypatch, batches, row):
    """The result writes of each kernel, on one family: 0 groups (status only), 1, the pattern's own count and 3 more (the extra slots
    read -1) with the capture table 0, 4, 8 and 12 bytes into an aligned allocation; n = 4k + 1 and 4k + 3 (tdfa_wave_kernel and the
    NFA kernels take four values per workgroup) and 64k + 1 (the lane-per-value kernels); a permuted subset of the lines (rows of
    unlisted lines keep their sentinels); a count on the device that is smaller than n (rows from it on keep their sentinels); the
    length-scheduled entry for the engines it serves.  All against the same oracle rows."""
    ce.set_env(monkeypatch, row)
    family = ce.EDGE_FAMILY[row.id]
    rx = ce.compile_row(row, family)
    batch = batches(family, row.walk, _copies(row, len(ce.generate(family, row.walk).cases)))
    N, G = batch["n"], batch["G"]
    base = ce.UNSTAGED_ABOVE if row.min_n else 0                               # (the unstaged launch stays unstaged)
    # (the chain rows that leave values to nfa_decide_kernel -- one lane walks a value of 800 bytes for milliseconds --: the same
    # shapes of n at a quarter of the size, the shuffled corpus's first values)
    small = (row.id, family) in ce.DECIDES
    cuts = (129, 131, 193) if small else (base + 513, base + 515, base + 577)
    assert [x % 4 for x in cuts] == [1, 3, 1] and cuts[2] % 64 == 1 and cuts[2] < N
    # (the depth-first kernels: a part of the corpus per launch)
    full = 257 if small else base + 1025 if row.id in ("decide", "dfs") else N
    assert row.id not in ce.NS_ROWS or 2 * G == ce.NS_ROWS[row.id]              # (G + 3 groups below: past the instantiation's NS slots)

    def check(where, ngroups=G, listed=None, **kw):
        caps, status, names = _launch(torch_dev, row, rx, batch, ngroups=ngroups, **kw)
        if not kw.get("ragged"):
            _ran(row, names, where, family)
        _compare(batch, caps, status, _cut(batch["caps"], ngroups), batch["status"], "%s, %s, %s" % (row.id, family, where), listed=listed)

    for shift in (0, 1, 2, 3):
        for ngroups in (0, 1, G, G + 3):
            check("table %d bytes off, %d groups" % (4 * shift, ngroups), ngroups=ngroups, form="len" if shift % 2 else "sep", caps_shift=shift,
                  n=full, listed=range(full))
    for k, cut in enumerate(cuts):
        check("%d values" % cut, form="len", caps_shift=k % 2, n=cut, listed=range(cut))
    rng = np.random.default_rng(7)
    subset = rng.permutation(N)[:cuts[1]]                                       # a permuted subset, 4k + 3 of them
    check("a permuted subset of %d" % len(subset), form="len", n=len(subset), lines=subset, listed=subset)
    check("a permuted subset of %d, separator form" % len(subset), form="sep", caps_shift=1, n=len(subset), lines=subset, listed=subset)
    check("%d of %d values by the count on the device" % (cuts[0], full), form="sep", n=full, nlines=cuts[0], listed=range(cuts[0]))
    check("%d of the subset by the count on the device" % cuts[2], form="len", n=len(subset), lines=subset, nlines=cuts[2], listed=subset[:cuts[2]])
    if row.launch_engine in (B.LC_ENGINE_TDFA, B.LC_ENGINE_NFA) and not row.dfs:
        for shift in (0, 2):
            check("length-scheduled, table %d bytes off" % (4 * shift), form="len", caps_shift=shift, n=full, listed=range(full), ragged=True)


STALE = [(r, f) for r in ce.ROWS for f in r.families if (r.id, f) in ce.CHAIN]


@pytest.mark.parametrize("row,family", STALE, ids=["%s-%s" % (r.id, f) for r, f in STALE])
def test_stale_overflow_bytes_of_unlisted_rows_are_left_alone(torch_dev, monkeypatch, batches, row, family):
    """The second chance and the decide kernels take the values whose status byte says LC_OVERFLOW -- of the values the launch
    LISTS.  The permuted-subset and device-count launches of test_result_edges once more, every status byte pre-filled with
    LC_OVERFLOW instead of the sentinel (what an earlier launch into the same buffer may have left): the launch raises its own
    overflow flag, and the rows it does not list come back untouched, capture rows and status bytes."""
    assert B.LC_OVERFLOW == 2
    ce.set_env(monkeypatch, row)
    rx = ce.compile_row(row, family)
    batch = batches(family, row.walk)
    N, G = batch["n"], batch["G"]
    cuts = (513, 515, 577)
    subset = np.random.default_rng(7).permutation(N)[:cuts[1]]
    assert cuts[2] < N and len(subset) < N

    def check(what, listed, **kw):
        where = "%s, %s, stale LC_OVERFLOW, %s" % (row.id, family, what)
        caps, status, names = _launch(torch_dev, row, rx, batch, status_fill=B.LC_OVERFLOW, **kw)
        _ran(row, names, where, family)
        _compare(batch, caps, status, batch["caps"], batch["status"], where, listed=listed, status_fill=B.LC_OVERFLOW)
        _sent_on(row, family, batch, names, where, listed=listed)

    check("a permuted subset of %d" % len(subset), subset, form="len", n=len(subset), lines=subset)
    check("a permuted subset of %d, separator form" % len(subset), subset, form="sep", caps_shift=1, n=len(subset), lines=subset)
    check("%d of %d values by the count on the device" % (cuts[0], N), range(cuts[0]), form="sep", n=N, nlines=cuts[0])
    check("257 of the subset by the count on the device", subset[:257], form="len", n=len(subset), lines=subset, nlines=257)


@pytest.mark.parametrize("row", [r for r in ce.ROWS if r.train == "family"], ids=lambda r: r.id)
def test_a_lazy_automaton_rebuilt_between_two_launches(torch_dev, monkeypatch, batches, row):
    """gpu_runtime.hip ensureLazyUploaded: a handle whose automaton was rebuilt since its last launch gets a new header and a new device
    copy.  The row's handle, trained as the row says, is launched; lazy_train gets the family's `miss` lines (tests/test_chunk_edges.py:
    all of them missed, now none does, the blob has grown); the SAME handle is launched again, in both forms.  Both launches give the
    oracle's rows.  Known limit: a device copy that stayed stale TOGETHER WITH its old header would still give right rows, because
    the misses fall back to the thread-list kernels; what this catches is a new header over old tables and a torn upload."""
    ce.set_env(monkeypatch, row)
    rx = ce.compile_row(row, "lazy")
    batch = batches("lazy", row.walk)
    words = len(rx.table(B.LC_TABLE_LAZY_TDFA_BLOB, np.uint32))
    for when in ("trained once", "trained again on its misses"):
        for form in ("len", "sep"):
            where = "%s, lazy, %s, %s form" % (row.id, when, form)
            caps, status, names = _launch(torch_dev, row, rx, batch, form)
            _ran(row, names, where)
            _compare(batch, caps, status, batch["caps"], batch["status"], where)
        if when == "trained once":
            r = rx.lazy_train(ce.miss_lines(row.walk))
            assert r["in_use"] == 1 and len(rx.table(B.LC_TABLE_LAZY_TDFA_BLOB, np.uint32)) > words, r


def test_the_atomic_instantiation_gives_up_values_of_131070_bytes_and_more(torch_dev, monkeypatch):
    """nfa_match_kernel<ATOMIC> hands a value of L >= 2^17 - 2 bytes to nfa_decide_kernel before it looks at it (a segment id is
    (offset << 6 | thread) in 23 bits).  Values of 2^17 - 3, 2^17 - 2 and 2^17 bytes -- a [^;] run and the tail ";12 x" -- among
    short ones, in both forms: every row is the oracle's, and lc_decide_stats counts exactly the two at or above the bound."""
    row = next(r for r in ce.ROWS if r.id == "nfa-atomic-edges")
    ce.set_env(monkeypatch, row)
    lines = ce.length_lines()
    assert sorted(len(x) for x in lines)[-3:] == [(1 << 17) - 3, (1 << 17) - 2, 1 << 17] == [ce.LENGTH_BOUND - 1, ce.LENGTH_BOUND, ce.LENGTH_BOUND + 2]
    assert all(x.endswith(ce.LENGTH_TAIL) and b";" not in x[:-5] for x in lines if len(x) > 1000)
    batch = batch_of(torch_dev, ce.explicit_corpus(ce.LENGTH_FAMILY, lines))
    assert batch["status"].sum() >= 7 and (batch["status"] == 0).sum() >= 3    # (the long ones match; some short ones do not)
    rx = B.GpuRegex(ce.LENGTH_FAMILY.pattern, engine=row.compile_engine)
    assert rx.atomic_groups()[0] == 1
    for form in ("len", "sep"):
        where = "length bound, %s form" % form
        caps, status, names = _launch(torch_dev, row, rx, batch, form)
        assert "nfa_match_kernel<atomic>" in names and "nfa_decide_kernel" in names and not [n for n in names if n.startswith("nfa_wide")], names
        _compare(batch, caps, status, batch["caps"], batch["status"], where)
        assert decide_stats() == (2, 0), (where, decide_stats())


def test_the_255th_atomic_instance_commits(torch_dev, monkeypatch):
    """A lineage key has 8 bits for the group instance.  A pattern with 255 instances compiles and its last one, index 254, decides:
    the `commits` value fails only because that group gives nothing back (tests/test_chunk_edges.py says so on the CPU); 256
    instances are refused.  Every byte of these values is a commit pass."""
    row = next(r for r in ce.ROWS if r.id == "nfa-atomic-edges")
    ce.set_env(monkeypatch, row)
    with pytest.raises(B.RegexUnsupportedError, match="more than 255 atomic group instances"):
        B.GpuRegex(ce.instance_pattern(256), engine=row.compile_engine)
    rx = B.GpuRegex(ce.INSTANCE_FAMILY.pattern, engine=row.compile_engine)
    assert rx.atomic_groups() == (255, 0)
    lines = [x for x, _ in ce.instance_lines()]
    batch = batch_of(torch_dev, ce.explicit_corpus(ce.INSTANCE_FAMILY, lines))
    what = [w for _, w in ce.instance_lines()]
    assert batch["status"][what.index("first")] == 1 and batch["status"][what.index("commits")] == 0
    for form in ("len", "sep"):
        caps, status, names = _launch(torch_dev, row, rx, batch, form)
        assert "nfa_match_kernel<atomic>" in names, names
        _compare(batch, caps, status, batch["caps"], batch["status"], "255 instances, %s form" % form)
        assert "nfa_decide_kernel" not in names or decide_stats() == (0, 0), (names, decide_stats())


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_global_memory_nfa_kernel_in_a_process_of_its_own(torch_dev):
    """nfa_match_kernel<..., GLOBAL=true> runs where a program exceeds 52 KB, and LC_NFA_GLOBAL_KB, which moves that bound, is read
    once per process: ONE child process with LC_NFA_GLOBAL_KB=0 (every non-empty batch takes the GLOBAL instantiation) runs rows `nfa`
    and `nfa-atomic` in both forms, the resumed searches and the result edges on `log`, family `alog` of row `nfa-atomic-edges` and row
    `achain-kept64` (with lc_decide_stats exact) in both forms, and rows `nfa-ns64`, `nfa-ns128` and `nfa-ns320`
    (64, 128 and 320 capture slots) in both forms (tests/helpers/global_nfa_child.py) and reports
    per launch how many values differ from the oracle's rows.  A child that faults, aborts or runs out of time fails the test with
    its stderr; nothing is started afterwards."""
    env = dict(os.environ)
    for k in ce.ENV_KEYS + ("LC_NFA_DFS", "LC_NFA_NO_WIDE"):
        env.pop(k, None)
    env.update(LC_NFA_GLOBAL_KB="0", LC_LAZY_TDFA="0")
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, "-c", "from tests.helpers.global_nfa_child import main; main()"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, "the child ended with status %d\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print("GLOBAL nfa_match_kernel child: %.1f s wall, of which imports %.1f s, launches and oracle %.1f s; %d launches" % (
        wall, res["seconds"]["imports"], res["seconds"]["work"], len(res["launches"])))
    bad = [x for x in res["launches"] if x["differ"] or not x["ran"]]
    assert not bad, "%d of %d launches differ; first: %s" % (len(bad), len(res["launches"]), bad[0])
    # 4 + 1 families in both forms, 3 search families resumed in both forms, 16 + 2 + 4 result-edge launches, alog and akept64 in both forms,
    # 3 slot widths in both forms
    assert len(res["launches"]) == 2 * 5 + 2 * 3 + 22 + 2 * 2 + 2 * 3, len(res["launches"])
    assert [x["launch"] for x in res["launches"][-10:-6]] == ["%s, %s, %s form" % (r, f, form) for r, f in (
        ("nfa-atomic-edges", "alog"), ("achain-kept64", "akept64")) for form in ("len", "sep")]
    assert "nfa_decide_kernel" in res["kernels"], res["kernels"]         # (the child checks per launch that no wide kernel took part)
    assert [x["launch"] for x in res["launches"][-6:]] == ["%s, %s, %s form" % (r, f, form) for r, f in (
        ("nfa-ns64", "log64"), ("nfa-ns128", "log128"), ("nfa-ns320", "log320")) for form in ("len", "sep")]
    assert "nfa_match_kernel" in res["kernels"] and "nfa_match_kernel<atomic>" in res["kernels"], res["kernels"]
