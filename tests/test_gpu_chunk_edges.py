"""The engines that walk one value per wavefront (nfa_match_kernel, nfa_wide_kernel, tdfa_wave_kernel) and their lane-per-value
neighbours (tdfa_l2_kernel, nfa_decide_kernel, nfa_dfs_kernel, bt_match_kernel) at 256-byte chunk edges and result edges: the corpus of
tests/helpers/chunk_edges.py -- values in which a run ends, the value ends, a capture is stamped, the value dies, the automaton
absorbs, a search starts or resumes on a chosen byte, for every alignment of the value's first byte -- through every row of its
instantiation table, against the oracle, bit for bit.  Each of those decisions is a comparison against a chunk border, the end of
the value or the start offset: a slip in one of them misparses only the values whose event sits on that byte for that alignment.
tests/test_chunk_edges.py says on the CPU that the corpus holds those values and that the tables are right.

Every launch keeps four sentinel rows in front of and behind the capture table and the status bytes (tests/helpers/guarded_launch.py)
and runs in both forms: (off, len), where filler gives each line its residue, and off[n + 1] with a separator byte."""
import ctypes

import numpy as np
import pytest

from loongcollector_amd import binding as B
from oracle.oracle import OracleRegex
from tests.helpers import chunk_edges as ce
from tests.helpers.guarded_launch import CAPS_SENTINEL, STATUS_SENTINEL, GuardedResults

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return torch


def _rows(fam, results, G):
    """oracle results -> (caps[n, 2G], status[n]) as a kernel writes them: a value that does not match reads -1 everywhere"""
    caps = np.full((len(results), 2 * G), -1, np.int32)
    status = np.zeros(len(results), np.uint8)
    for i, r in enumerate(results):
        if r is not None:
            caps[i] = [v for be in (r if fam.search else r[1:]) for v in be]
            status[i] = 1
    return caps, status


def _tile(data, off, length, form, copies, M=16):
    """the packed corpus `copies` times over: every copy of a line keeps its residue in the (off, len) form (copies start at multiples
    of M); in the separator form the copies follow each other without a gap, as off[n + 1] demands"""
    if copies == 1:
        return data, off, length
    n = len(length)
    body = data[:len(data) - ce.GUARD_BYTES]
    step = len(body) if form == "sep" else (len(body) + M - 1) // M * M
    block = np.zeros(step, np.uint8)
    block[:len(body)] = body
    big = np.concatenate([np.tile(block, copies), np.zeros(ce.GUARD_BYTES, np.uint8)])
    offs = np.concatenate([off[:n] + np.uint32(k * step) for k in range(copies)] + ([np.array([copies * step], np.uint32)] if form == "sep" else []))
    return big, offs.astype(np.uint32), np.tile(length, copies)


@pytest.fixture(scope="module")
def batches(torch_dev):
    """(family, walk, copies) -> the corpus on the device in both forms and the oracle's rows for it: computed once, shared by every
    test, left unchanged"""
    torch = torch_dev
    dev = torch.device("cuda:0")
    made = {}

    def get(name, walk, copies=1):
        key = (name, walk, copies)
        if key not in made:
            c = ce.generate(name, walk)
            fam = c.family
            o = OracleRegex(fam.pattern)
            G = o.groups + (1 if fam.search else 0)
            caps, status = _rows(fam, [(o.search if fam.search else o.fullmatch)(k.line) for k in c.cases], G)
            batch = dict(corpus=c, oracle=o, G=G, n0=len(c.cases), n=copies * len(c.cases), caps=np.tile(caps, (copies, 1)), status=np.tile(status, copies))
            for form in ("len", "sep"):
                data, off, length, _ = c.pack(form)
                data, off, length = _tile(data, off, length, form, copies)
                d_data = torch.from_numpy(data.copy()).to(dev)
                assert d_data.data_ptr() % 16 == 0                              # a line's residue is its offset's
                batch[form] = dict(d_data=d_data, d_off=torch.from_numpy(off.view(np.int32).copy()).to(dev),
                                   d_len=torch.from_numpy(length.view(np.int32).copy()).to(dev) if form == "len" else None)
            made[key] = batch
        return made[key]
    return get


def _copies(row, n0):
    return -(-row.min_n // n0) if row.min_n else 1


def _launch(torch, row, rx, batch, form, ngroups=None, caps_shift=0, n=None, lines=None, nlines=None, frm=None, ragged=False):
    """One launch of `row` -> (caps[N, 2 * ngroups], status[N], kernel names): rows for ALL N values of the batch, of which the launch
    takes the first n, or those `lines` lists, or as many as `nlines` says on the device.  Asserts the sentinels around the results."""
    dev = torch.device("cuda:0")
    N = batch["n"]
    n = N if n is None else n
    ngroups = batch["G"] if ngroups is None else ngroups
    res = GuardedResults(torch, N, ngroups, caps_shift)
    io = batch[form]
    sep = 0 if form == "len" else 1
    stream = torch.cuda.current_stream().cuda_stream
    i32 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).to(dev)
    L = B.load()
    L.lc_nfa_set_dfs.argtypes = [ctypes.c_int]
    B.launched_kernels()
    try:
        if row.dfs:
            L.lc_nfa_set_dfs(1)
        if ragged:
            d_scratch = torch.empty((B.sched_scratch_bytes(n) // 4 + 1,), dtype=torch.int32, device=dev)
            rx.match_device_ragged(io["d_data"], io["d_off"], io["d_len"], n, res.d_caps, res.d_status, d_scratch, ngroups=ngroups, sep_bytes=sep,
                                   engine=row.launch_engine, stream=stream)
        elif lines is not None or nlines is not None or frm is not None:
            rx.match_device_from(io["d_data"], io["d_off"], io["d_len"], n, res.d_caps, res.d_status, d_lines=i32(lines),
                                 d_nlines=i32(None if nlines is None else [nlines]), d_from=i32(frm), ngroups=ngroups, sep_bytes=sep, stream=stream,
                                 engine=row.launch_engine)
        else:
            rx.match_device(io["d_data"], io["d_off"], io["d_len"], n, res.d_caps, res.d_status, ngroups=ngroups, sep_bytes=sep, stream=stream,
                            engine=row.launch_engine)
        torch.cuda.synchronize()
    finally:
        if row.dfs:
            L.lc_nfa_set_dfs(-1)
    names = B.launched_kernels().split(", ")
    caps, status = res.read((row.id, form, n, ngroups, caps_shift))
    return caps, status, names


def _cut(caps, ngroups):
    """the oracle's rows at ngroups output groups: fewer groups cut the row, further ones read -1"""
    G = caps.shape[1] // 2
    if ngroups <= G:
        return caps[:, :2 * ngroups]
    return np.concatenate([caps, np.full((len(caps), 2 * (ngroups - G)), -1, np.int32)], axis=1)


def _compare(batch, got_caps, got_status, exp_caps, exp_status, where, listed=None):
    """the rows of the `listed` values (default: all) against the oracle's; every other row still holds its sentinels"""
    N = batch["n"]
    took = np.ones(N, bool) if listed is None else np.zeros(N, bool)
    if listed is not None:
        took[np.asarray(listed, np.int64)] = True
    wrong = (got_status != exp_status) | (got_caps != exp_caps).any(axis=1)
    untouched = (got_status == STATUS_SENTINEL) & (got_caps == CAPS_SENTINEL).all(axis=1)
    bad = np.nonzero(np.where(took, wrong, ~untouched))[0]
    if bad.size:
        c, i = batch["corpus"], int(bad[0])
        k = i % batch["n0"]
        pytest.fail("%s: %d values differ, by kind %s; first: %s%s%s\n  expected status %d row %s\n  actual   status %d row %s" % (
            where, bad.size, c.kinds_of(bad % batch["n0"]), c.label(k), "" if i == k else ", copy %d" % (i // batch["n0"]),
            "" if took[i] else " (NOT LISTED: its row must keep the sentinels)", int(exp_status[i]), exp_caps[i].tolist(), int(got_status[i]), got_caps[i].tolist()))


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
