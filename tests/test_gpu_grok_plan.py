"""Phase 1 of the speculative Grok matcher on the device, kernel by kernel, against the plain models of tests/helpers/grok_plan_model.py
(tied to the index blob and the regex oracle by tests/test_grok_plan_model.py).  Every kernel of the phase is a FILTER: a bit it
wrongly clears silently loses a match, a bit it wrongly leaves only costs time -- the end-to-end tests see the first by luck and the
second never.  Here whole mask arrays are compared bit for bit, through lc_grok_plan_masks_device (the function the matcher itself
runs), into buffers longer than n whose tail must keep its sentinel.

    literal pass   grok_literal_lds_kernel (default), grok_literal_chunk_kernel (LC_GROK_LITERAL_LDS=0), grok_literal_index_kernel (a batch
                   of 262 145 values): every literal length at every chunk / look-behind / lane-group edge, near misses, mixed quads
    mask halves    a 64-entry list (bits 32-63), lists without an index (grok_mask_fill_kernel)
    screens        grok_screen_all_kernel on the 50-entry list of configs[2]: every offset modulo 16 x every short length, neighbours
                   that would flip the verdict, walks that die / reach the sink at every byte of a 16-byte unit, slice edges; scaled,
                   unscaled, transposed or not, staged or (large batch) through L2
    counts         grok_count_kernel's perEntry / firstOf / shadowBy, bit 63 and a hot cell included"""
import json
import os
import random

import numpy as np
import pytest

from loongcollector_amd import binding as B
from loongcollector_amd.grok import Grok
from tests.helpers import grok_plan_cases as C
from tests.helpers import grok_plan_model as M

pytestmark = pytest.mark.gpu

BIG_N = 262145      # one more than the largest "small" batch (grok_device.hip kGrokSmallBatch)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert B.device_count() >= 1
    torch.cuda.set_device(0)
    return torch


def run_plan(torch, g, data, off, length, stage):
    """-> (masks uint64[n], counts uint32[PLAN_WORDS] or None, kernel names); the sentinels behind n / behind the count words checked"""
    dev = torch.device("cuda:0")
    n = len(off)
    assert len(data) % 16 == 0
    d_data = torch.from_numpy(np.array(data)).to(dev)
    assert d_data.data_ptr() % 16 == 0
    d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev)
    d_len = torch.from_numpy(length.view(np.int32).copy()).to(dev)
    d_masks = torch.full((n + 37,), C.SENTINEL64, dtype=torch.int64, device=dev)
    d_counts = torch.full((M.PLAN_WORDS + 19,), C.SENTINEL32, dtype=torch.int32, device=dev)
    d_scratch = torch.empty(g.scratch_bytes(n), dtype=torch.uint8, device=dev)
    B.launched_kernels()
    g.plan_masks_device(d_data, d_off, d_len, n, stage, d_masks, d_counts if stage == 2 else None, d_scratch)
    names = B.launched_kernels()
    masks = d_masks.cpu().numpy().view(np.uint64)
    counts = d_counts.cpu().numpy().view(np.uint32)
    assert (masks[n:] == np.uint64(C.SENTINEL64)).all(), "the mask array was written behind n"
    if stage == 2:
        assert (counts[M.PLAN_WORDS:] == C.SENTINEL32).all(), "the count words were written behind their end"
    else:
        assert (counts == C.SENTINEL32).all()
    return masks[:n].copy(), (counts[:M.PLAN_WORDS].copy() if stage == 2 else None), names


class Expect:
    """the models over a list, remembered per value"""

    def __init__(self, lits, screens=None):
        self.lits, self.always = lits, M.always_bits(lits)
        self.screens = screens or [None] * len(lits)
        self.memo = {}

    def masks(self, values, stage):
        out = np.empty(len(values), dtype=np.uint64)
        for i, v in enumerate(values):
            key = (stage, v)
            if key not in self.memo:
                self.memo[key] = (M.literal_mask(self.lits, self.always, v) if stage == 1
                                  else M.stage2_mask(self.lits, self.always, self.screens, v))
            out[i] = self.memo[key]
        return out


def same_masks(got, want, values, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), [(int(i), len(values[i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]])


def padded_to_big(batch):
    """the batch's arrays with fillers of 0 and 1 bytes behind the values, BIG_N values in all"""
    at = len(batch.buf)
    batch.buf += C.FILLER * 64
    data, off, length = batch.finish()
    k = BIG_N - len(off)
    fill_len = (np.arange(k) % 2).astype(np.uint32)
    fill_off = (at + np.arange(k) % 48).astype(np.uint32)
    values = batch.values + [C.FILLER * int(l) for l in fill_len]
    return data, np.concatenate([off, fill_off]), np.concatenate([length, fill_len]), values


LITERAL_MODES = {"lds": ("grok_literal_lds_kernel", None), "chunk": ("grok_literal_chunk_kernel", "0"), "big": ("grok_literal_index_kernel", None)}


def literal_mode(monkeypatch, mode):
    if LITERAL_MODES[mode][1] is not None:
        monkeypatch.setenv("LC_GROK_LITERAL_LDS", LITERAL_MODES[mode][1])
    return LITERAL_MODES[mode][0]


# ---- the literal pass ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lit7():
    lits = C.literal_list()
    g = Grok(Match=C.literal_match(lits))
    got = M.indexed_literals(C.required_literals(g))
    assert got == [l[-32:] for l in lits] and g.literal_index() is not None
    batch = C.literal_sweep(C.Batch(), lits)
    for n in C.QUAD_SIZES:      # (the quads travel with the sweep too: neighbours of every length around them)
        for v in C.quad_values(lits, n, seed=n):
            batch.add(v)
    return g, Expect(got), batch


@pytest.mark.parametrize("mode", ["lds", "chunk", "big"])
def test_literal_pass_at_every_chunk_and_look_behind_edge(torch_dev, lit7, monkeypatch, mode):
    """One occurrence of each literal (1, 2, 16, 31, 32, 33, 40 bytes; of the last two the final 32 are indexed) ending at c*64 + d in
    values of 63 .. 8193 bytes, at the value's first and last byte, and cut by either end of the value with the missing byte in the
    neighbour -- the 31-byte look-behind, the chunk's end, the 16 / 32 / 64-lane groups of the LDS kernel (1 KiB / 2 KiB / longer)
    and the second trip behind 4096 bytes.  A missed occurrence is a lost match; a found near miss is a read outside the value."""
    g, ex, batch = lit7
    kernel = literal_mode(monkeypatch, mode)
    if mode == "big":
        data, off, length, values = padded_to_big(_copy(batch))
    else:
        (data, off, length), values = _copy(batch).finish(), batch.values
    assert len(values) > 4000 and max(len(v) for v in values) == 8193
    got, _, names = run_plan(torch_dev, g, data, off, length, 1)
    assert kernel in names, names
    want = ex.masks(values, 1)
    same_masks(got, want, values, mode)
    assert sum(bin(int(m)).count("1") for m in want[:len(batch.values)]) > 3500


def _copy(batch):
    b = C.Batch()
    b.buf, b.off, b.len, b.values = bytearray(batch.buf), list(batch.off), list(batch.len), list(batch.values)
    return b


@pytest.mark.parametrize("mode", ["lds", "chunk"])
@pytest.mark.parametrize("n", C.QUAD_SIZES)
def test_literal_pass_quads_of_mixed_lane_groups(torch_dev, lit7, monkeypatch, mode, n):
    """Batches of 1 .. 9 values of 2049, 1025, 1024, 5, 0, 1 ... bytes: the length order puts a 64-lane value, a 32-lane value, 16-lane
    values and empty ones into the same and into neighbouring quads of the LDS kernel; every value carries another set of literals."""
    g, ex, _ = lit7
    kernel = literal_mode(monkeypatch, mode)
    for seed in (0, 3, 5):
        values = C.quad_values(ex.lits, n, seed=seed)
        b = C.Batch()
        for v in values:
            b.add(v)
        data, off, length = b.finish()
        got, _, names = run_plan(torch_dev, g, data, off, length, 1)
        assert kernel in names, names
        same_masks(got, ex.masks(values, 1), values, (mode, n, seed))
    assert len(set(ex.masks(C.quad_values(ex.lits, 9, seed=0), 1).tolist())) >= 6


# ---- bits 32-63, entries without a literal, lists without an index -------------------------------------------------------------------
@pytest.fixture(scope="module")
def lit64():
    lengths = [{0: 16, 31: 32, 32: 33, 63: 40}.get(i, 3 + i % 6) for i in range(64)]      # (short ones mostly: the index still fits LDS)
    lits = [b"" if i in (1, 33, 62) else C.synthetic_literal(i, k) for i, k in enumerate(lengths)]
    g = Grok(Match=C.literal_match(lits))
    got = M.indexed_literals(C.required_literals(g))
    assert got == [l[-32:] for l in lits]
    ex = Expect(got)
    assert ex.always == (1 << 1) | (1 << 33) | (1 << 62)
    return g, ex, lits


@pytest.mark.parametrize("mode", ["lds", "chunk", "big"])
def test_both_mask_halves_of_a_64_entry_list(torch_dev, lit64, monkeypatch, mode):
    """Literals at entries 0, 31, 32 and 63 (and most others), none at 1, 33 and 62: the always-bits of both halves, and bits 32-63
    through the two 32-bit halves the chunk kernels carry across the wavefront."""
    g, ex, lits = lit64
    kernel = literal_mode(monkeypatch, mode)
    b = C.Batch()
    for p in (0, 31, 32, 63, 2, 47):
        for L in (len(lits[p]), 65, 1025, 2049, 4097):
            for end in sorted({len(lits[p]), L, 64, 95, 96, 1024 + 31, 2048, 4096 + 31}):
                if end - len(lits[p]) >= 0 and end <= L:
                    b.add(C.placed(L, lits[p], end))
    for L in (300, 1500, 2500, 5000):     # several entries of both halves in one value, in different chunks
        v = bytearray(C.FILLER * L)
        for k, p in enumerate((63, 0, 32, 31, 40)):
            v[L - 41 - 57 * k:L - 41 - 57 * k + len(lits[p])] = lits[p]
        b.add(bytes(v))
    if mode == "big":
        data, off, length, values = padded_to_big(b)
    else:
        (data, off, length), values = b.finish(), b.values
    got, _, names = run_plan(torch_dev, g, data, off, length, 1)
    assert kernel in names, names
    want = ex.masks(values, 1)
    same_masks(got, want, values, mode)
    seen = int(np.bitwise_or.reduce(want))
    assert all((seen >> p) & 1 for p in (0, 1, 31, 32, 33, 62, 63)) and int(np.bitwise_and.reduce(want)) == ex.always


@pytest.mark.parametrize("entries, with_literal", [(1, 0), (1, 1), (63, 1), (64, 0), (64, 1)])
def test_lists_without_an_index_fill_every_bit(torch_dev, entries, with_literal):
    """fewer than two literals: no index, grok_mask_fill_kernel sets the bits of the whole list -- its nP >= 64 guard included"""
    lits = [C.synthetic_literal(i, 5) if i < with_literal else b"" for i in range(entries)]
    g = Grok(Match=C.literal_match(lits))
    assert g.literal_index() is None
    ex = Expect(M.indexed_literals(C.required_literals(g)))
    assert ex.always == (1 << entries) - 1
    b = C.Batch()
    for i in range(300):
        b.add(C.FILLER * (i % 70))
    data, off, length = b.finish()
    got, _, names = run_plan(torch_dev, g, data, off, length, 1)
    assert "grok_mask_fill_kernel" in names, names
    same_masks(got, ex.masks(b.values, 1), b.values, entries)


# ---- the screens -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config3(golden_dir):
    with open(os.path.join(golden_dir, "grok_config3.json"), encoding="utf-8") as f:
        cfg3 = json.load(f)
    g = Grok(Match=cfg3["match"], CustomPatterns=cfg3["custom_patterns"], AnchoredFirst=False)
    blobs = [g.screen_blob(i) for i in range(g.n_match)]
    screens = [None if sb is None else M.Screen(sb[0]) for sb in blobs]
    ex = Expect(M.indexed_literals(C.required_literals(g)), screens)
    return g, ex, blobs


def test_screen_classes_of_the_config3_list(config3):
    """Which walks the list's screens take.  A screen is staged into LDS up to 44 KiB of accept flags + table, and a staged table of up to
    64 KiB is staged SCALED: every staged screen is a scaled one (the screen compiler relaxes a pattern until its table can be staged,
    so the list has no screen that a small batch walks through L2 either).  The unscaled staged walk is therefore reached through
    LC_GROK_SCREEN_SCALED=0 and the walk through L2 through a large batch: test_screens_at_every_alignment_and_edge runs both."""
    _, ex, blobs = config3
    have = [(sc, sb[1]) for sc, sb in zip(ex.screens, blobs) if sc is not None]
    assert len(have) >= 30
    scaled = [sc for sc, lds in have if lds and sc.table_bytes <= 0xFFFF]
    assert len(scaled) >= 30 and all(lds == (sc.stage_bytes + 3) & ~3 for sc, lds in have if lds)
    assert [sc for sc, lds in have if lds and sc.table_bytes > 0xFFFF] == []      # (44 KiB < 64 KiB)
    assert all(sc.sink != M.NO_SINK for sc, _ in have)                             # (every one ends early on a certain match)


SCREEN_MODES = {"default": {}, "unscaled": {"LC_GROK_SCREEN_SCALED": "0"}, "not_transposed": {"LC_GROK_SCREEN_TRANSPOSED": "0"}, "big": {}}


@pytest.mark.parametrize("mode", list(SCREEN_MODES))
def test_screens_at_every_alignment_and_edge(torch_dev, config3, monkeypatch, mode):
    """grokScreenWalk / grokScreenWalkScaled read aligned 16-byte units around a value and test for sink / dead once per unit.  Values at
    every offset modulo 16 and of 0 .. 48 and 4096 bytes, derived from the screens' own automata: they stay alive to their last byte
    with neighbour bytes that would flip the verdict in front and behind; accepted strings cut by either end of the value; walks
    that die or reach the sink at every byte of a unit with a string behind that a restarted walk would accept."""
    g, ex, _ = config3
    for k, v in SCREEN_MODES[mode].items():
        monkeypatch.setenv(k, v)
    batch = C.config3_edge_values(ex.screens, ex.lits)
    assert {o % 16 for o in batch.off} == set(range(16)) and {0, 1, 15, 16, 17, 31, 32, 33, 48, 4096} <= set(batch.len)
    if mode == "big":
        data, off, length, values = padded_to_big(batch)
    else:
        (data, off, length), values = batch.finish(), batch.values
    got1, _, names1 = run_plan(torch_dev, g, data, off, length, 1)
    got2, counts, names2 = run_plan(torch_dev, g, data, off, length, 2)
    assert "grok_screen_all_kernel" in names2 and "grok_count_kernel" in names2 and "grok_screen_all_kernel" not in names1, (names1, names2)
    assert ("grok_literal_index_kernel" in names2) == (mode == "big")
    want1, want2 = ex.masks(values, 1), ex.masks(values, 2)
    same_masks(got1, want1, values, (mode, "stage 1"))
    same_masks(got2, want2, values, (mode, "stage 2"))
    assert np.array_equal(counts, M.plan_counts(want2, g.n_match))
    rejected = sum(bin(int(a & ~b)).count("1") for a, b in zip(want1[:len(batch.values)], want2[:len(batch.values)]))
    passed = sum(bin(int(b)).count("1") for p, b in enumerate(want2[:len(batch.values)]))
    assert rejected > 1000 and passed > 500, (rejected, passed)


def slice_batch(n, sc, lit, every):
    """n values whose order by length bucket (32 bytes a bucket, longest first: sched_kernel.hpp) is known: the carriers of the
    entry's bit -- values that contain its literal -- sit alone in their buckets at the first and the last place of every slice of 256
    (every = False), or everywhere (True)"""
    places = sorted({s for s in range(0, n, 256)} | {min(s + 256, n) - 1 for s in range(0, n, 256)})
    acc = C.accepted(sc)
    b, q, at, k = C.Batch(), 40, 0, 0

    def carrier(L):
        nonlocal k
        k += 1
        body = (acc if k % 2 else lit + b"\x01")      # one that passes, one the screen rejects
        return body + b"x" * (L - len(body))
    for p in places + [n]:
        run = p - at
        for _ in range(run):
            b.add(carrier(32 * q + 7) if every else b"x" * (32 * q + 7))
        if run:
            q -= 1
        if p < n:
            b.add(carrier(32 * q + 3))
            q -= 1
        at = p + 1
    assert len(b.values) == n and q >= 0
    return b


@pytest.mark.parametrize("mode", ["default", "unscaled", "not_transposed"])
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_screen_slices_and_their_edges(torch_dev, config3, monkeypatch, n, mode):
    """grok_screen_all_kernel compacts the carriers of a bit per slice of 256 values in length order (ballot prefix, one atomic per
    wavefront) before it walks them: carriers only at the first and last place of each slice, then every value a carrier."""
    g, ex, _ = config3
    for k, v in SCREEN_MODES[mode].items():
        monkeypatch.setenv(k, v)
    p = 9                                             # NAGIOSLOGLINE: literal "[", a ten-state screen with a sink
    assert ex.lits[p] == b"[" and ex.screens[p] is not None
    for every in (False, True):
        b = slice_batch(n, ex.screens[p], ex.lits[p], every)
        data, off, length = b.finish()
        got, counts, names = run_plan(torch_dev, g, data, off, length, 2)
        assert "grok_screen_all_kernel" in names
        want = ex.masks(b.values, 2)
        same_masks(got, want, b.values, (n, every))
        assert np.array_equal(counts, M.plan_counts(want, g.n_match))
        carriers = sum(ex.lits[p] in v for v in b.values)
        assert carriers == (n if every else len({s for s in range(0, n, 256)} | {min(s + 256, n) - 1 for s in range(0, n, 256)}))
        assert 0 < sum((int(m) >> p) & 1 for m in want) < carriers


# ---- the counts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_candidate_counts(torch_dev, lit64, n):
    """grok_count_kernel: perEntry, firstOf and shadowBy (from which the host carves the entries' arrays and orders the levels) against
    a count in numpy -- bit 63, the always-bits, and at n = 70 001 one cell of shadowBy that more than a thousand values hit."""
    g, ex, lits = lit64
    rng = random.Random(n)
    templates = [lits[0] + b"." + lits[63], lits[63], lits[5] + lits[31] + b".." + lits[32], b"", lits[63] + lits[40] + lits[0]]
    templates += [b".".join(lits[p] for p in rng.sample(range(64), rng.randint(1, 6)) if lits[p]) for _ in range(12)]
    b = C.Batch()
    for t in templates:
        b.add(t)
    data, t_off, t_len = b.finish()
    pick = np.array([0 if rng.random() < 0.3 else rng.randrange(len(templates)) for _ in range(n)])
    pick[0] = 0
    got, counts, names = run_plan(torch_dev, g, data, t_off[pick], t_len[pick], 2)
    assert "grok_count_kernel" in names, names
    want = ex.masks([templates[i] for i in pick], 2)
    assert np.array_equal(got, want)
    model = M.plan_counts(want, 64)
    assert np.array_equal(counts, model), np.nonzero(counts != model)[0][:10]
    assert model[63] >= 1 and model[64 + 0] >= 1 and model[128 + 63 * 64 + 0] >= 1
    if n == 70001:
        assert model[128 + 63 * 64 + 0] > 1000 and model[128 + 33 * 64 + 0] > 1000


def test_first_candidates_in_the_high_half(torch_dev):
    """A list whose low half has no always-bit: values whose FIRST candidate is entry 2 .. 63 -- firstOf and shadowBy's f index across the
    two 32-bit halves of the mask."""
    lits = [C.synthetic_literal(i, 4 + i % 3) for i in range(64)]
    g = Grok(Match=C.literal_match(lits))
    ex = Expect(M.indexed_literals(C.required_literals(g)))
    assert ex.always == 0
    rng = random.Random(9)
    b = C.Batch()
    for f in range(64):
        for _ in range(5):
            b.add(b".".join(lits[p] for p in [f] + rng.sample(range(f, 64), min(3, 64 - f))))
    data, off, length = b.finish()
    got, counts, names = run_plan(torch_dev, g, data, off, length, 2)
    assert "grok_count_kernel" in names
    want = ex.masks(b.values, 2)
    same_masks(got, want, b.values, "high half")
    model = M.plan_counts(want, 64)
    assert np.array_equal(counts, model)
    assert all(model[64 + f] >= 5 for f in range(64))
    assert sum(int(model[128 + p * 64 + f]) for p in range(33, 64) for f in range(32, p)) > 50


# ---- a small batch that stages some screens and walks others through L2 ----------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_screens(golden_dir):
    """LC_RELAX_BUDGET=1600 (regex_handle.cpp: relaxed screens start from this budget) leaves three CISCOFW formats of configs[2] a
    relaxed screen of 47 .. 131 KB -- more than the 44 KiB that are staged -- next to entries whose screens are staged"""
    with open(os.path.join(golden_dir, "grok_config3.json"), encoding="utf-8") as f:
        cfg3 = json.load(f)
    idx = [3, 4, 21, 23, 25, 26, 45]
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LC_RELAX_BUDGET", "1600")
        g = Grok(Match=[cfg3["match"][i] for i in idx], CustomPatterns=cfg3["custom_patterns"], AnchoredFirst=False)
    g.config = dict(Match=[cfg3["match"][i] for i in idx], CustomPatterns=cfg3["custom_patterns"])
    blobs = [g.screen_blob(i) for i in range(g.n_match)]
    screens = [None if sb is None else M.Screen(sb[0]) for sb in blobs]
    from loongcollector_amd.grok_corpus import grok_lines
    ex = Expect(M.indexed_literals(C.required_literals(g)), screens)
    # (the values once for all modes; the automata have up to 1 471 states, so few synthetic walks and many log lines)
    rng = random.Random(21)
    b = C.Batch()
    for p in [p for p, sb in enumerate(blobs) if sb is not None and sb[1] == 0]:
        C.screen_edge_values(b, screens[p], ex.lits[p], rng, lengths=(31, 33, 300), splice=1.0)
    for i, line in enumerate(grok_lines(1500, seed=5)):
        b.add(line, before=b"]", after=b"[", align=i % 16)
    return g, ex, blobs, b


@pytest.mark.parametrize("mode", ["default", "unscaled", "not_transposed"])
def test_staged_and_unstaged_screens_in_one_launch(torch_dev, mixed_screens, monkeypatch, mode):
    """screens with lds_bytes == 0 (their tables are walked in global memory) beside staged ones in the launch of a SMALL batch"""
    g, ex, blobs, batch = mixed_screens
    unstaged = [p for p, sb in enumerate(blobs) if sb is not None and sb[1] == 0]
    staged = [p for p, sb in enumerate(blobs) if sb is not None and sb[1] != 0]
    assert len(unstaged) >= 2 and len(staged) >= 2, blobs
    assert all(ex.screens[p].stage_bytes > 44 * 1024 for p in unstaged)
    for k, v in SCREEN_MODES[mode].items():
        monkeypatch.setenv(k, v)
    b = batch
    data, off, length = b.finish()
    got, counts, names = run_plan(torch_dev, g, data, off, length, 2)
    assert "grok_screen_all_kernel" in names and "grok_literal_index_kernel" not in names
    want1, want2 = ex.masks(b.values, 1), ex.masks(b.values, 2)
    same_masks(got, want2, b.values, mode)
    assert np.array_equal(counts, M.plan_counts(want2, g.n_match))
    for p in unstaged:
        seen = sum((int(m) >> p) & 1 for m in want1)
        kept = sum((int(m) >> p) & 1 for m in want2)
        assert 0 < kept < seen, (p, kept, seen)


# ---- the remainder kernels, end to end -------------------------------------------------------------------------------------------------
REMAINDERS = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097)
# (entry, a first match at the head, a further match, the byte that makes the further match's leading assertion hold / fail in front of it)
REM_ENTRIES = [
    (r"Zxq(?P<a>[0-9Z]+)", b"Zxq1", b"Zxq22", b".", None),
    (r"\bkey(?P<b>\d+)", b"key1", b"key22", b".", b"_"),
    (r"\Bkez(?P<c>\d+)", b"akez1", b"kez22", b"_", b"."),
    (r"(?<=x)kew(?P<d>\d+)", b"xkew1", b"kew22", b"x", b"."),
    (r"(?<![0-9])7q(?P<e>[a-c]+)", b"7qa", b"7qbb", b".", b"3"),
]


def remainder_values():
    values = []
    for _, head, more, ok, bad in REM_ENTRIES:
        for R in REMAINDERS:
            fill = lambda n: b"." * n
            h = head                                              # (3 .. 5 bytes: `from` is never 16-aligned inside the value)
            m = ok + more
            values.append(h + fill(R))                            # nothing behind the first match
            if len(more) <= R:
                values.append(h + more + fill(R - len(more)))     # a further match exactly at `from`: the byte in front of it is the first match's
            if len(m) <= R:
                values.append(h + fill(R - len(m)) + m)           # ... ending at the value's last byte
                if bad is not None:
                    values.append(h + fill(R - len(m)) + bad + more)   # the assertion fails on the byte in front
                for c in (64, 128, 1024, 4032):                   # its literal across chunk boundaries counted from `from` (the second trip's,
                                                                  # at 4096, lies behind the longest remainder)
                    at = c - 2 - len(ok)
                    if at >= 0 and at + len(m) <= R:
                        values.append(h + fill(at) + m + fill(R - at - len(m)))
        # the further match's literal straddles `from`: the first match has eaten its first byte
    values += [b"Zxq1Zxq2" + b"." * r for r in (0, 1, 15, 61, 4090)]
    return values


@pytest.mark.parametrize("remainder_literal", [None, "0"])
def test_remainders_behind_a_first_match(torch_dev, monkeypatch, remainder_literal):
    """grok_remainder_literal_kernel / grok_remainder_all_kernel decide which values are searched again behind their first match
    (FindNextMatch).  A first match at the head, then 1 .. 4097 bytes with a further match at `from`, at the last byte, with its literal
    across the chunk boundaries counted from `from`, straddling `from`; entries that begin with an assertion on the byte before
    `from`.  Pattern ids, first rows and extra rows equal the sequential walk's, the fields the oracle's, on every value."""
    from oracle.grok_oracle import GrokOracle
    from tests.helpers.grok_device_rows import device_rows
    if remainder_literal is not None:
        monkeypatch.setenv("LC_GROK_REMAINDER_LITERAL", remainder_literal)
    match = [e[0] for e in REM_ENTRIES]
    values = remainder_values()
    spec, seq = Grok(Match=match), Grok(Match=match, Speculative=False)
    B.launched_kernels()
    p1, f1, x1, s1 = device_rows(torch_dev, spec, values)
    names = B.launched_kernels()
    p2, f2, x2, s2 = device_rows(torch_dev, seq, values)
    assert s1["speculative"] and not s2["speculative"]
    # (these entries have no screen: of grok_remainder_all_kernel only the pass-through runs here; its walk: the next test)
    assert "grok_remainder_literal_kernel" in names and all(spec.screen_blob(i) is None for i in range(spec.n_match)), names
    assert np.array_equal(p1, p2) and np.array_equal(f1, f2) and np.array_equal(x1, x2)
    assert len(x1) > 100 and (p1 >= 0).all()
    o = GrokOracle(match)
    pattern, fields = spec.match_host(values)
    assert np.array_equal(np.asarray(pattern), p1)
    twice = 0
    for v, f in zip(values, fields):
        assert f == o.process_value(v)[1], v[:40]
        twice += len(f) >= 2
    assert twice > 100


def remainder_screen_values(o, screens, lits, entries):
    """For the entries whose match ends where the format ends (not with a GREEDYDATA tail): a matched log line A at the head, then the
    remainders.  -> (values in which no remainder passes its entry's screen, values with a further match)"""
    from loongcollector_amd.grok_corpus import grok_lines
    quiet, more = [], []
    fill = lambda n: b"." * n
    for p in entries:
        rx = o.compiled[p]
        heads = []
        for l in grok_lines(3000, seed=5):
            c = rx.search(l, 0)
            if c is not None and c[0][0] == 0:
                a = l[:c[0][1]]
                c2 = rx.search(a + a, 0)
                if c2 is not None and c2[0] == (0, len(a)) and len(a) % 16 != 0:
                    heads.append(a)
            if len(heads) == 8:
                break
        a = min(heads, key=len)
        assert len(a) < 4000
        for R in REMAINDERS:
            quiet.append(a + fill(R))
            if len(lits[p]) <= R:
                quiet.append(a + fill(R - len(lits[p])) + lits[p])      # the literal alone: the literal pass lets it through, the screen decides
        quiet.append(a + a[1:-1])                                        # a further match without its first and last byte
        for extra in (0, 1, 2, 15, 16, 17):
            more.append(a + a + fill(extra))                             # a further match exactly at `from` ...
            more.append(a + fill(extra) + a)                             # ... and ending at the value's last byte
        for R in (4095, 4096, 4097):
            more.append(a + a + fill(R - len(a)))
            more.append(a + fill(R - len(a)) + a)
            more.append(a + fill(R - 2 * len(a) - 7) + a + fill(7) + a)
    # the model's verdicts: a value of `quiet` stays only if every entry's screen rejects what is left behind that entry's first match
    def survivors(v):
        n = 0
        for q, rx in enumerate(o.compiled):
            c = rx.search(v, 0)
            if c is not None and screens[q] is not None:
                b0, e0 = c[0]
                nxt = e0 if e0 > b0 else e0 + 1
                n += nxt < len(v) and screens[q].passes(v[nxt:])
        return n
    kept = [v for v in quiet if survivors(v) == 0]
    assert len(kept) >= len(quiet) * 3 // 4 and all(survivors(v) >= 1 for v in more), (len(kept), len(quiet))
    return kept, more


@pytest.mark.parametrize("scaled", [None, "0"])
def test_remainder_screens_walk_from_the_first_match(torch_dev, mixed_screens, monkeypatch, scaled):
    """grok_remainder_all_kernel's walk: entries WITH a screen -- staged ones and ones walked through L2 -- whose first match ends inside
    the value, at an offset that is not 16-aligned.  With a further match at `from`, at the last byte and in between, the rows are the
    sequential walk's and the fields the oracle's (a walk that starts a byte late, or over the wrong table, loses the match).  And
    where the model's walk over exactly [from, len) rejects every remainder, nothing survives: the batch ends after its third host
    synchronisation (include/lc_grok.h: a fourth when a remainder passes its entry's screen) -- a walk that runs on into the next
    value, which begins with a whole match, would pass.  The literal pass in front is switched off so that the screens decide."""
    from oracle.grok_oracle import GrokOracle
    from tests.helpers.grok_device_rows import device_rows
    g, ex, blobs, _ = mixed_screens
    monkeypatch.setenv("LC_GROK_REMAINDER_LITERAL", "0")
    if scaled is not None:
        monkeypatch.setenv("LC_GROK_SCREEN_SCALED", scaled)
    o = GrokOracle(g.config["Match"], custom_patterns=g.config["CustomPatterns"])
    entries = [1, 2, 4, 5]          # CRONLOG and CISCOFW106100 (staged), CISCOFW106014 and CISCOFW106100_2_3 (through L2)
    assert [blobs[p][1] != 0 for p in entries] == [True, False, False, True]
    quiet, more = remainder_screen_values(o, ex.screens, ex.lits, entries)
    seq = Grok(Speculative=False, AnchoredFirst=False, **g.config)
    tail = [b"." * 8192]            # (no entry matches it: every value with a remainder has 8 KiB of the batch behind it)
    for values, survive in ((more + tail, True), (quiet + tail, False), (quiet + more + tail, True)):
        device_rows(torch_dev, g, values)                      # (the entries learn how many rounds to queue ahead)
        B.launched_kernels()
        p1, f1, x1, s1 = device_rows(torch_dev, g, values)
        names = B.launched_kernels()
        p2, f2, x2, s2 = device_rows(torch_dev, seq, values)
        assert s1["speculative"] and "grok_remainder_all_kernel" in names and "grok_remainder_literal_kernel" in names, (s1, names)
        assert np.array_equal(p1, p2) and np.array_equal(f1, f2) and np.array_equal(x1, x2)
        assert (p1[:-1] >= 0).all() and p1[-1] == -1
        if survive:
            assert len(x1) >= len(more)
        else:
            assert s1["host_syncs"] == 3 and len(x1) == 0, s1
    pattern, fields = g.match_host(quiet + more)
    for v, f in zip(quiet + more, fields):
        assert f == o.process_value(v)[1], v[:60]
