"""The Grok plan's own first and second chance (csrc/grok_device.hip runFirst / runSecond, the overflow list, the count on the device,
grokOverflowSeen switching an entry to nfa_wide_kernel:first) on values whose 65th / 129th live thread appears on a chosen byte.
tests/helpers/fused_round0.py overflow_list(): entries `^T00:` + over64 and `^T01:` + over128 (tests/helpers/chunk_edges.py: the overflow
families with named groups) beside a log entry that stays a tagged DFA and an entry nobody is a candidate of; the values are those
families' cases with the tag in front, the event still on W256_P of the tagged value, at residues 0..3.

An entry's round 0 is its ANCHORED form (79 / 149 positions): on it an over64 `at_cap` value peaks at exactly 64 threads and an over64
overflow variant at 65, so which values nfa_match_kernel gives up shows from outside -- a batch of controls alone never raises the
entry's GC_WIDE word, and the entry never goes wide first.  Every over128 value needs more than 64 threads, its overflow variants more
than 128: those walk first chance -> overflow list -> nfa_wide_kernel -> nfa_decide_kernel.

LazyTdfa=False keeps the lazy automata out of the way, so that the history rules are alone (as tests/test_gpu_grok.py does); the last
test gives them their turn.  Expectations: the sequential walk's rows (Speculative=False) and GrokOracle's fields on every value."""
import collections

import numpy as np
import pytest

from loongcollector_amd import binding as B
from loongcollector_amd.grok import Grok
from oracle.grok_oracle import GrokOracle
from tests.helpers import fused_round0 as F
from tests.helpers.grok_device_rows import device_rows

pytestmark = pytest.mark.gpu
KNOBS = ("LC_GROK_WIDE_FIRST", "LC_GROK_FUSED_ROUND0", "LC_LAZY_TDFA")


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def chain(torch_dev):
    """the list, the full batch and the quiet one (over64's controls and the log values) packed at their residues, the sequential
    walk's rows for both, GrokOracle's verdict on every value -- computed once, left unchanged"""
    match, values = F.overflow_list()
    out = {"match": match}
    o = GrokOracle(match)
    seq = Grok(Match=match, Speculative=False, LazyTdfa=False).wait_ready()
    assert [seq.engine(k) for k in range(seq.n_match)] == [B.LC_ENGINE_NFA, B.LC_ENGINE_NFA, B.LC_ENGINE_TDFA, B.LC_ENGINE_NFA]
    for name, vals in (("full", values), ("quiet", [v for v in values if not F.needs_wide(v)])):
        packed, data, off, length = F.pack(vals)
        assert all(int(a) % 4 == v.head for a, v in zip(off, packed)) and {v.head for v in packed if v.family != "log"} == {0, 1, 2, 3}
        want = device_rows(torch_dev, seq, None, packed=(data, off, length))
        assert not want[3]["speculative"]
        pattern, fields = seq.match_host([v.bytes for v in packed])
        assert np.array_equal(np.asarray(pattern), want[0])
        for i, (v, p, f) in enumerate(zip(packed, pattern, fields)):
            res, exp = o.process_value(v.bytes)
            assert f == exp and (p >= 0) == (res == 0) and p != -2 and (p < 0 or p == v.entry), (i, v, p, f, exp)
        out[name] = dict(values=packed, packed=(data, off, length), want=want, pattern=np.asarray(pattern))
    # what the batches hold: the overflow variants match where the label says (a Grok entry is a search: one byte too many behind the
    # run still matches), the controls all match, and the quiet batch has no value that needs more than 64 threads
    full = out["full"]
    won = collections.Counter((v.family, v.variant) for v, p in zip(full["values"], full["pattern"]) if p >= 0 and v.family != "log")
    per = collections.Counter((v.family, v.variant) for v in full["values"] if v.family != "log")
    assert set(per.values()) == {34} and len(per) == 12
    assert won == {(f, v): 34 for f in ("over64", "over128") for v in ("match", "far", "one_more", "at_cap_match", "at_cap_far")}, won
    quiet = collections.Counter(v.family for v in out["quiet"]["values"])
    assert quiet["over64"] == 68 and quiet["log"] >= 500 and set(quiet) == {"over64", "log"}
    assert {v.variant for v in out["quiet"]["values"] if v.family == "over64"} == {"at_cap_match", "at_cap_far"}
    return out


def _clean(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _batch(torch, g, b, what):
    """one batch through the plan -> kernel names; the rows are the sequential walk's"""
    B.launched_kernels()
    got = device_rows(torch, g, None, packed=b["packed"], scratch_fill=0xA5)
    names = B.launched_kernels().split(", ")
    assert got[3]["speculative"], what
    for k, part in enumerate(("pattern", "first", "extra")):
        assert got[k].shape == b["want"][k].shape and np.array_equal(got[k], b["want"][k]), "%s: %s differs from the sequential walk's" % (what, part)
    return names


FIRST = "nfa_wide_kernel:first"


def test_first_chance_overflow_list_wide_and_decide_then_wide_first_by_history(torch_dev, monkeypatch, chain):
    _clean(monkeypatch)
    g = Grok(Match=chain["match"], LazyTdfa=False).wait_ready()
    names = _batch(torch_dev, g, chain["full"], "batch 1")
    # no history: the first chance is nfa_match_kernel, the overflow list goes to nfa_wide_kernel, what outgrows that to nfa_decide_kernel
    assert {"nfa_match_kernel", "nfa_wide_kernel", "nfa_decide_kernel"} <= set(names) and FIRST not in names, names
    for k in (2, 3):
        names = _batch(torch_dev, g, chain["full"], "batch %d" % k)
        assert FIRST in names and "nfa_decide_kernel" in names, (k, names)       # (over128's overflow variants are still the decide kernel's)


def test_a_batch_of_values_at_exactly_64_threads_leaves_no_history(torch_dev, monkeypatch, chain):
    """over64's controls peak at exactly 64 threads: nfa_match_kernel decides them, the wide kernel has nothing to do, GC_WIDE stays 0
    and the entry's next batch is NOT wide first.  A control given up one thread early would show as nfa_wide_kernel:first."""
    _clean(monkeypatch)
    g = Grok(Match=chain["match"], LazyTdfa=False).wait_ready()
    for k in (1, 2):
        names = _batch(torch_dev, g, chain["quiet"], "quiet batch %d" % k)
        assert "nfa_match_kernel" in names and FIRST not in names, (k, names)
    # ... and the same handle on the full batch: still no history when it is queued, history behind it
    names = _batch(torch_dev, g, chain["full"], "the full batch behind the quiet ones")
    assert FIRST not in names and "nfa_wide_kernel" in names, names
    assert FIRST in _batch(torch_dev, g, chain["full"], "the full batch again")


@pytest.mark.parametrize("knob,value", [("LC_GROK_WIDE_FIRST", "0"), ("LC_GROK_WIDE_FIRST", "2"), ("LC_GROK_FUSED_ROUND0", "0")])
def test_plan_knobs_give_the_same_rows(torch_dev, monkeypatch, chain, knob, value):
    _clean(monkeypatch)
    monkeypatch.setenv(knob, value)
    g = Grok(Match=chain["match"], LazyTdfa=False).wait_ready()
    for k in (1, 2):
        names = _batch(torch_dev, g, chain["full"], "%s=%s, batch %d" % (knob, value, k))
        if knob == "LC_GROK_WIDE_FIRST":
            assert (FIRST in names) == (value == "2"), (k, names)                 # never / from the first batch on
        else:
            assert "tdfa_wave_multi_kernel" not in names and (FIRST in names) == (k == 2), (k, names)


def test_lazy_automata_in_front_of_the_chain_give_the_same_rows(torch_dev, monkeypatch, chain):
    """the default handle: batches of the values themselves train the entries' lazy automata (as tests/test_gpu_grok_fused_round0.py
    trains: batches, then a settled trainer); whatever they decide and whatever they hand back, the rows stay the sequential walk's"""
    _clean(monkeypatch)
    g = Grok(Match=chain["match"]).wait_ready()
    for k in range(3):
        _batch(torch_dev, g, chain["full"], "training batch %d" % k)
        assert g.lazy_settle(120000)
    assert g.lazy_stats()["automata_in_use"] >= 1, g.lazy_stats()
    _batch(torch_dev, g, chain["full"], "behind the trained automata")
    _batch(torch_dev, g, chain["quiet"], "the quiet batch behind the trained automata")
