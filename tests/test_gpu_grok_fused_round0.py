"""The Grok plan's fused round 0 (csrc/grok_device.hip phase 2a) at its own edges.  tdfa_wave_multi_kernel shares its walk with the
pinned tdfa_wave_kernel; what is its own is the binary search of a workgroup's number over firstBlock[64], the per-job values, tables,
outputs and miss words, ONE LDS size for jobs with different register counts (staged and not), and the one grok_post_kernel launch
behind it with a skip mask for the entries in between that are not in the launch.  tests/helpers/fused_round0.py builds Match lists
whose entries are a tag and a chunk-edge family's body, and values -- the chunk-edge cases with the tag in front, each at its residue
-- that are candidates of ONE entry each, so that every job's rows show:

  mixed     log as a search (junk in front of some tags), the 8 000-state automaton, a run capture BETWEEN two fused entries (its bit
            is in the post launch's skip mask), the pattern that does not determinise behind its lazy automaton -- with the values that
            MISS, which come back LC_OVERFLOW and go to the second chance --, two untagged searches, an entry without candidates
  borders   1, 2, 3, 63 and 64 entries with 1, 3, 4, 5, 8, 9, 2, 7, ... candidates: every pattern of full and ragged last workgroups

Per list: the default path's rows equal those with LC_GROK_FUSED_ROUND0=0, those of the sequential walk and those of the same values
packed without gaps; the fields equal the oracle's on EVERY value; the kernels that ran and the number of pairs are what the list says."""
import collections

import numpy as np
import pytest

from loongcollector_amd import binding as B
from loongcollector_amd.grok import Grok
from oracle.grok_oracle import GrokOracle
from tests.helpers import fused_round0 as F
from tests.helpers import grok_plan_cases as C
from tests.helpers import grok_plan_model as M
from tests.helpers.grok_device_rows import device_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return torch


def _candidates(g, values):
    """per value the entries it is a candidate of (tests/helpers/grok_plan_model.py over the handle's own literals and screens:
    tests/test_gpu_grok_plan.py pins the kernels to that model)"""
    lits = M.indexed_literals(C.required_literals(g))
    always = M.always_bits(lits)
    screens = [None if sb is None else M.Screen(sb[0]) for sb in (g.screen_blob(i) for i in range(g.n_match))]
    return [M.stage2_mask(lits, always, screens, v.bytes) for v in values]


def _same(got, want, what):
    for k, name in enumerate(("pattern", "first", "extra")):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), "%s: %s differs" % (what, name)


def _through_every_path(torch, monkeypatch, match, values, training=(), **config):
    """-> (kernel names of the default path's batch, its stats, the candidate masks, the pattern per value in batch order, values in
    batch order).  Asserts what every list asserts."""
    monkeypatch.delenv("LC_GROK_FUSED_ROUND0", raising=False)
    monkeypatch.delenv("LC_LAZY_TDFA", raising=False)
    values, data, off, length = F.pack(values)
    assert all(int(o) % 4 == v.head for o, v in zip(off, values)) and len({v.bytes for v in values}) > 0.9 * len(values)
    g = Grok(Match=match, **config).wait_ready()
    if training:                                                              # the lazy automaton: batches of training lines, a settled trainer
        for _ in range(3):
            device_rows(torch, g, [t.bytes for t in training])
            assert g.lazy_settle(120000)
        assert g.lazy_stats()["automata_in_use"] >= 1, g.lazy_stats()
    masks = _candidates(g, values)
    d_scratch = torch.empty(g.scratch_bytes(len(values)), dtype=torch.uint8, device=torch.device("cuda:0"))
    B.launched_kernels()
    got = device_rows(torch, g, None, packed=(data, off, length), scratch_fill=0xA5, d_scratch=d_scratch)
    names = B.launched_kernels().split(", ")
    stats = got[3]
    assert stats["speculative"] and "tdfa_wave_multi_kernel" in names, (stats, names)
    assert stats["pairs"] == sum(bin(m).count("1") for m in masks), stats
    # one launch per entry
    monkeypatch.setenv("LC_GROK_FUSED_ROUND0", "0")
    B.launched_kernels()
    unfused = device_rows(torch, g, None, packed=(data, off, length), scratch_fill=0x5A)
    assert "tdfa_wave_multi_kernel" not in B.launched_kernels()
    monkeypatch.delenv("LC_GROK_FUSED_ROUND0")
    _same(unfused, got, "LC_GROK_FUSED_ROUND0=0")
    # the sequential walk of the list
    seq = Grok(Match=match, Speculative=False, **config).wait_ready()
    walked = device_rows(torch, seq, None, packed=(data, off, length))
    assert not walked[3]["speculative"]
    _same(walked, got, "Speculative=False")
    # the same values without gaps (offsets in a row are the value's own), and once more as they were
    _same(device_rows(torch, g, [v.bytes for v in values], scratch_fill=0xA5), got, "packed without gaps")
    # ... and as they were, in the scratch area as the first batch left it: every status and capture row of that batch is still there
    _same(device_rows(torch, g, None, packed=(data, off, length), d_scratch=d_scratch), got, "the default path again, same scratch area")
    # the oracle, on every value
    o = GrokOracle(match)
    pattern, fields = g.match_host([v.bytes for v in values])
    assert np.array_equal(np.asarray(pattern), got[0])
    matched = 0
    for i, (v, p, f) in enumerate(zip(values, pattern, fields)):
        res, want = o.process_value(v.bytes)
        assert f == want and (p >= 0) == (res == 0) and p != -2, (i, v, p, f, want)
        assert p < 0 or p == v.entry, (i, v, p)                                # (a value is its own entry's)
        matched += p >= 0
    return names, stats, masks, np.asarray(pattern), values, matched


@pytest.mark.parametrize("anchored_first", [True, False], ids=["anchored-first", "searches-only"])
def test_mixed_list_every_kind_of_job_in_one_launch(torch_dev, monkeypatch, anchored_first):
    """anchored-first (the default): round 0 of an entry is its anchored search where the warm-up thread has delivered one -- the `^Tkk:`
    jobs carry no resume offsets, and the `{14}` entry, whose search does not determinise, runs its ANCHORED form, a complete automaton
    of 32 000 states.  searches-only (AnchoredFirst=False): every job is the entry's search and carries the offsets to resume at, and the
    `{14}` entry is a thread-list program behind its lazy automaton: its `miss` values come back LC_OVERFLOW from the fused launch."""
    match, values, training = F.mixed_list()
    assert not {t.bytes for t in training} & {v.bytes for v in values}
    g = Grok(Match=match)
    assert [g.engine(k) for k in range(g.n_match)] == [B.LC_ENGINE_TDFA] * 3 + [B.LC_ENGINE_NFA] + [B.LC_ENGINE_TDFA] * 3
    # the 8 000-state automaton's register programs: whether they fit the share of LDS the launch stages them in (gpu_runtime.hip lcWaveJobPrepare)
    big = B.GpuRegex(g.expanded(1).encode(), syntax_flags=C.GROK_SYNTAX)
    blob = big.table(B.LC_TABLE_TDFA_L2_BLOB, np.uint32)
    prog_bytes = (int(blob[9]) - int(blob[7]) + 3) & ~3
    assert big.info()["states"] > 8000 and 0 < prog_bytes <= 40 * 1024 and int(blob[3]) * 4 * 4 + prog_bytes <= 60 * 1024, prog_bytes
    counts = collections.Counter((v.family, v.kind) for v in values)
    assert {f for f, _ in counts} == {"log", "big", "run", "lazy", "quasi", "look"} and 2500 <= len(values) <= 4000
    for fam in ("log", "big", "lazy", "quasi", "look"):
        kinds = set(F.ce.FAMILIES[fam].kinds) - {"resume"}
        assert {k for f, k in counts if f == fam} == kinds and all(counts[fam, k] >= 34 for k in kinds), (fam, counts)
    misses = [v for v in values if v.kind == "miss"]
    assert collections.Counter(v.variant for v in misses) == {v: 34 for v in ("last", "far", "no_match", "needy")}
    assert sum(v.bytes[:1] != b"T" for v in values if v.family == "log") >= 200                      # junk in front of the search entry's tag
    anchored = B.GpuRegex(g.expanded(3).encode(), syntax_flags=C.GROK_SYNTAX | B.LC_SYNTAX_PREFIX)
    assert anchored.info()["engine"] == B.LC_ENGINE_TDFA and anchored.info()["states"] > 30000
    names, stats, masks, pattern, packed, matched = _through_every_path(torch_dev, monkeypatch, match, values, training,
                                                                        AnchoredFirst=anchored_first)
    per_entry = [sum((m >> p) & 1 for m in masks) for p in range(len(match))]
    assert all(bin(m).count("1") <= 1 for m in masks) and per_entry[6] == 0 and min(per_entry[:6]) >= 40, per_entry
    assert "tdfa_l2_kernel:wave" in names, names              # the run-capture entry: a launch of its own, its bit in the post launch's skip mask
    if not anchored_first:
        assert any(n.startswith("nfa_") for n in names), names    # the misses went to the thread-list program's second chance
        assert "tdfa_l2_kernel:wave:lazy" not in names, names     # ... from the one launch: the lazy automaton had no launch of its own
    # every value that misses and matches is its entry's, with the oracle's fields (asserted above on every value)
    won = {v.bytes for v, p in zip(packed, pattern) if p == 3}
    assert all((v.bytes in won) == (v.variant in ("last", "far")) for v in misses)
    assert matched >= 2000


@pytest.mark.parametrize("n_entries", [1, 2, 3, 63, 64])
def test_job_borders(torch_dev, monkeypatch, n_entries):
    match, values = F.border_list(n_entries)
    assert len(match) == n_entries
    names, stats, masks, pattern, packed, matched = _through_every_path(torch_dev, monkeypatch, match, values)
    # candidates per entry, from the packed corpus: 1, 3, 4, 5, 8, 9, 2, 7 in turn
    per_entry = [sum((m >> p) & 1 for m in masks) for p in range(n_entries)]
    assert per_entry == [F.BORDER_COUNTS[k % 8] for k in range(n_entries)] and all(bin(m).count("1") == 1 for m in masks), per_entry
    assert stats["pairs"] == len(values) == sum(per_entry)
    # every entry was in the one launch: none had a launch of its own
    assert "tdfa_l2_kernel:wave" not in names and "tdfa_l2_kernel:wave:lazy" not in names and not any(n.startswith("nfa_") for n in names), names
    assert matched > 0 and (n_entries < 63 or matched < len(values))                                # (matches and failures among the jobs' values)
