"""Test-only: the launches of tests/test_gpu_chunk_edges.py -- the chunk-edge corpus on the device in both input forms, the oracle's
rows for it, one guarded launch of a row of the instantiation table, and the comparison of what came back.  Shared with
tests/helpers/global_nfa_child.py, which runs the same launches in a process of its own.  Not part of the product."""
import ctypes

import numpy as np

from loongcollector_amd import binding as B
from oracle.oracle import OracleRegex
from tests.helpers import chunk_edges as ce
from tests.helpers.guarded_launch import CAPS_SENTINEL, STATUS_SENTINEL, GuardedResults


def rows(fam, results, G):
    """oracle results -> (caps[n, 2G], status[n]) as a kernel writes them: a value that does not match reads -1 everywhere"""
    caps = np.full((len(results), 2 * G), -1, np.int32)
    status = np.zeros(len(results), np.uint8)
    for i, r in enumerate(results):
        if r is not None:
            caps[i] = [v for be in (r if fam.search else r[1:]) for v in be]
            status[i] = 1
    return caps, status


def tile(data, off, length, form, copies, M=16):
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


def batch_of(torch, c, copies=1):
    """a Corpus on the device in both forms and the oracle's rows for it"""
    dev = torch.device("cuda:0")
    fam = c.family
    o = OracleRegex(fam.pattern)
    G = o.groups + (1 if fam.search else 0)
    caps, status = rows(fam, [(o.search if fam.search else o.fullmatch)(k.line) for k in c.cases], G)
    batch = dict(corpus=c, oracle=o, G=G, n0=len(c.cases), n=copies * len(c.cases), caps=np.tile(caps, (copies, 1)), status=np.tile(status, copies))
    for form in ("len", "sep"):
        data, off, length, _ = c.pack(form)
        data, off, length = tile(data, off, length, form, copies)
        d_data = torch.from_numpy(data.copy()).to(dev)
        assert d_data.data_ptr() % 16 == 0                                      # a line's residue is its offset's
        batch[form] = dict(d_data=d_data, d_off=torch.from_numpy(off.view(np.int32).copy()).to(dev),
                           d_len=torch.from_numpy(length.view(np.int32).copy()).to(dev) if form == "len" else None)
    return batch


def make_batches(torch):
    """-> get(family, walk, copies): the corpus on the device in both forms and the oracle's rows for it: computed once, shared by
    every caller, left unchanged"""
    made = {}

    def get(name, walk, copies=1):
        key = (name, walk, copies)
        if key not in made:
            made[key] = batch_of(torch, ce.generate(name, walk), copies)
        return made[key]
    return get


def launch(torch, row, rx, batch, form, ngroups=None, caps_shift=0, n=None, lines=None, nlines=None, frm=None, ragged=False,
           status_fill=STATUS_SENTINEL):
    """One launch of `row` -> (caps[N, 2 * ngroups], status[N], kernel names): rows for ALL N values of the batch, of which the launch
    takes the first n, or those `lines` lists, or as many as `nlines` says on the device.  Asserts the sentinels around the results.
    status_fill: what every status byte holds before the launch instead of its sentinel."""
    dev = torch.device("cuda:0")
    N = batch["n"]
    n = N if n is None else n
    ngroups = batch["G"] if ngroups is None else ngroups
    res = GuardedResults(torch, N, ngroups, caps_shift, status_fill)
    io = batch[form]
    sep = 0 if form == "len" else 1
    stream = torch.cuda.current_stream().cuda_stream
    i32 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).to(dev)
    L = B.load()
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


def cut(caps, ngroups):
    """the oracle's rows at ngroups output groups: fewer groups cut the row, further ones read -1"""
    G = caps.shape[1] // 2
    if ngroups <= G:
        return caps[:, :2 * ngroups]
    return np.concatenate([caps, np.full((len(caps), 2 * (ngroups - G)), -1, np.int32)], axis=1)


def decide_stats():
    """lc_decide_stats -> (values the calling thread's last decide launches settled, values they gave up)"""
    L = B.load()
    stats = (ctypes.c_uint64 * 2)()
    assert L.lc_decide_stats(stats) == 0
    return int(stats[0]), int(stats[1])


def differing(batch, got_caps, got_status, exp_caps, exp_status, where, listed=None, status_fill=STATUS_SENTINEL):
    """the rows of the `listed` values (default: all) against the oracle's; every other row still holds its sentinels (its status byte:
    `status_fill`, what the launch found there).
    -> (number of values that differ, a description of the first or None)"""
    N = batch["n"]
    took = np.ones(N, bool) if listed is None else np.zeros(N, bool)
    if listed is not None:
        took[np.asarray(listed, np.int64)] = True
    wrong = (got_status != exp_status) | (got_caps != exp_caps).any(axis=1)
    untouched = (got_status == status_fill) & (got_caps == CAPS_SENTINEL).all(axis=1)
    bad = np.nonzero(np.where(took, wrong, ~untouched))[0]
    if not bad.size:
        return 0, None
    c, i = batch["corpus"], int(bad[0])
    k = i % batch["n0"]
    return int(bad.size), "%s: %d values differ, by kind %s; first: %s%s%s\n  expected status %d row %s\n  actual   status %d row %s" % (
        where, bad.size, c.kinds_of(bad % batch["n0"]), c.label(k), "" if i == k else ", copy %d" % (i // batch["n0"]),
        "" if took[i] else " (NOT LISTED: its row must keep the sentinels)", int(exp_status[i]), exp_caps[i].tolist(), int(got_status[i]), got_caps[i].tolist())
