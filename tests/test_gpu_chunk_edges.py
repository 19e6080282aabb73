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
from tests.helpers.chunk_edge_launch import cut as _cut, differing, launch as _launch, make_batches, rows as _rows

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


def _compare(batch, got_caps, got_status, exp_caps, exp_status, where, listed=None):
    """the rows of the `listed` values (default: all) against the oracle's; every other row still holds its sentinels"""
    n, first = differing(batch, got_caps, got_status, exp_caps, exp_status, where, listed)
    if n:
        pytest.fail(first)


def _ran(row, names, where):
    assert row.kernel in names, (where, names)                                 # (the instantiation the row names is what ran)
    if row.id == "nfa-wide-first":
        assert "nfa_match_kernel" not in names, (where, names)
    if row.id == "l2-lane":
        assert "tdfa_l2_kernel:wave" not in names, (where, names)


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
            _ran(row, names, where)
            _compare(batch, caps, status, batch["caps"], batch["status"], where)


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
    cuts = (base + 513, base + 515, base + 577)
    assert [x % 4 for x in cuts] == [1, 3, 1] and cuts[2] % 64 == 1 and cuts[2] < N
    full = base + 1025 if row.id in ("decide", "dfs") else N                    # (the depth-first kernels: a part of the corpus per launch)

    def check(where, ngroups=G, listed=None, **kw):
        caps, status, names = _launch(torch_dev, row, rx, batch, ngroups=ngroups, **kw)
        if not kw.get("ragged"):
            _ran(row, names, where)
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


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_global_memory_nfa_kernel_in_a_process_of_its_own(torch_dev):
    """nfa_match_kernel<..., GLOBAL=true> runs where a program exceeds 52 KB, and LC_NFA_GLOBAL_KB, which moves that bound, is read
    once per process: ONE child process with LC_NFA_GLOBAL_KB=0 (every non-empty batch takes the GLOBAL instantiation) runs rows `nfa`
    and `nfa-atomic` in both forms, the resumed searches and the result edges on `log` (tests/helpers/global_nfa_child.py) and reports
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
    # 4 + 1 families in both forms, 3 search families resumed in both forms, 16 + 2 + 4 result-edge launches
    assert len(res["launches"]) == 2 * 5 + 2 * 3 + 22, len(res["launches"])
    assert "nfa_match_kernel" in res["kernels"] and "nfa_match_kernel<atomic>" in res["kernels"], res["kernels"]
