"""The plain models of the Grok plan's phase 1 (tests/helpers/grok_plan_model.py) tied down without a GPU: the literal model against the
Aho-Corasick blob the device walks, the expected masks (literal model + byte-by-byte screen walk) against the regex oracle -- a bit
the model clears is a pair the oracle never matches --, the counts against a direct count.  tests/test_gpu_grok_plan.py then holds
the kernels to these models bit for bit."""
import json
import os
import random

import numpy as np
import pytest

from loongcollector_amd.grok import Grok
from oracle.grok_oracle import GrokOracle
from tests.helpers import grok_plan_cases as C
from tests.helpers import grok_plan_model as M

required_literals, config3_edge_values = C.required_literals, C.config3_edge_values


@pytest.fixture(scope="module")
def plan(golden_dir):
    from loongcollector_amd.grok_corpus import grok_lines
    with open(os.path.join(golden_dir, "grok_config3.json"), encoding="utf-8") as f:
        cfg3 = json.load(f)
    g = Grok(Match=cfg3["match"], CustomPatterns=cfg3["custom_patterns"], AnchoredFirst=False)
    lits = M.indexed_literals(required_literals(g))
    screens = [None if sb is None else M.Screen(sb[0]) for sb in (g.screen_blob(i) for i in range(g.n_match))]
    values = grok_lines(600) + config3_edge_values(screens, lits).values
    return cfg3, g, lits, screens, values


def test_literal_model_equals_the_blob_walk(plan):
    """bit p = `lits[p][-32:] in v` (Python's `in`) = what a byte-by-byte walk of the index blob collects (grok_literal_layout.h; the
    walk of tests/test_grok_host.py::test_literal_index_of_the_match_list)"""
    _, g, lits, _, values = plan
    blob = g.literal_index()
    raw = blob.view(np.uint8)
    nstates, ncls, off_masks, off_table, always_lo, always_hi = [int(x) for x in blob[:6]]
    cmap = bytes(raw[32:288])
    out = raw[off_masks:off_masks + 8 * nstates].view(np.uint64).tolist()
    table = raw[off_table:off_table + 2 * nstates * ncls].view(np.uint16).tolist()
    always = M.always_bits(lits)
    assert always == always_lo | (always_hi << 32)
    set_bits = 0
    for v in values:
        state, mask = 0, always
        for c in v.translate(cmap):
            e = table[state * ncls + c]
            state = e & 0x7FFF
            if e & 0x8000:
                mask |= out[state]
        assert mask == M.literal_mask(lits, always, v), v[:80]
        set_bits += bin(mask & ~always).count("1")
    assert set_bits > 1000


def test_expected_masks_are_necessary_for_an_oracle_match(plan):
    """Whenever the oracle finds a contributing match of entry p in v (a match with a non-empty named capture: processGrok's rule), the
    model's stage-2 bit p is set.  And the values do exercise both sides: pairs that match, pairs a screen rejects."""
    cfg3, g, lits, screens, values = plan
    o = GrokOracle(cfg3["match"], custom_patterns=cfg3["custom_patterns"])
    always = M.always_bits(lits)
    assert sum(sc is not None for sc in screens) >= 30
    matched = screened = 0
    for v in values:
        m1 = M.literal_mask(lits, always, v)
        m2 = M.stage2_mask(lits, always, screens, v)
        assert m2 & ~m1 == 0
        screened += bin(m1 & ~m2).count("1")
        for p, (rx, fields) in enumerate(zip(o.compiled, o.fields)):
            start, hit = 0, False
            while start <= len(v) and not hit:
                caps = rx.search(v, start)
                if caps is None:
                    break
                hit = any(caps[gi][0] >= 0 and caps[gi][1] > caps[gi][0] for _, groups in fields for gi in groups)
                b0, e0 = caps[0]
                start = e0 if e0 > b0 else e0 + 1
            if hit:
                matched += 1
                assert (m2 >> p) & 1, (p, cfg3["match"][p], v[:120])
    assert matched >= 1000 and screened >= 1000, (matched, screened)


def test_counts_model_against_a_direct_count():
    rng = random.Random(3)
    masks = [0, 1 << 63, (1 << 63) | 1, 0xFFFFFFFFFFFFFFFF] + [rng.getrandbits(64) & rng.getrandbits(64) for _ in range(500)]
    got = M.plan_counts(np.array(masks, dtype=np.uint64), 64)
    want = np.zeros(M.PLAN_WORDS, dtype=np.uint32)
    for m in masks:
        bits = [p for p in range(64) if (m >> p) & 1]
        for p in bits:
            want[p] += 1
        if bits:
            want[64 + bits[0]] += 1
            for p in bits[1:]:
                want[128 + p * 64 + bits[0]] += 1
    assert np.array_equal(got, want) and got[63] >= 4 and got[128 + 63 * 64 + 0] >= 2
    assert M.plan_counts(np.array([7], dtype=np.uint64), 2).tolist()[:3] == [1, 1, 0]     # (bits at or above the list's length are not counted per entry)


def test_the_overflow_chain_list_puts_thread_65_and_129_where_it_says():
    """What tests/test_gpu_grok_overflow_chain.py rests on (tests/helpers/fused_round0.py overflow_list).  Both overflow entries are
    thread-list programs with AnchoredFirst on and off, beside a log entry that stays a tagged DFA.  On the ANCHORED form the plan
    runs first (79 / 149 positions) the walk with nfa_match_kernel's 64 threads overflows exactly on the values needs_wide() names --
    over64's overflow variants and every over128 value; over64's controls peak at 64 and are decided -- and with nfa_wide_kernel's 128
    exactly on over128's overflow variants.  GrokOracle matches the overflow values (a Grok entry is a search: all but `ends`)."""
    import collections

    from loongcollector_amd import binding as B
    from tests.helpers import fused_round0 as F
    from tests.helpers.table_interp import NfaInterp
    match, values = F.overflow_list()
    for anchored_first in (True, False):
        g = Grok(Match=match, AnchoredFirst=anchored_first)
        assert [g.engine(k) for k in range(g.n_match)] == [B.LC_ENGINE_NFA, B.LC_ENGINE_NFA, B.LC_ENGINE_TDFA, B.LC_ENGINE_NFA]
    per = collections.Counter((v.family, v.variant) for v in values if v.family != "log")
    assert len(per) == 12 and set(per.values()) == {34} and sum(v.family == "log" for v in values) >= 500
    assert {(v.family, v.head) for v in values} == {(f, h) for f in ("over64", "over128", "log") for h in range(4)}
    o = GrokOracle(match)
    for k, family, npos in ((0, "over64", 79), (1, "over128", 149)):
        it = NfaInterp(B.GpuRegex(g.expanded(k).encode(), syntax_flags=C.GROK_SYNTAX | B.LC_SYNTAX_PREFIX, engine=B.LC_ENGINE_NFA))
        assert it.npos == npos and it.nslots <= 8
        for v in values:
            if v.entry != k:
                continue
            assert v.family == family and v.p in F.ce.W256_P and v.bytes[v.p:v.p + 1] == b"a" and v.bytes[v.p + 1:v.p + 2] != b"a", v
            over = not v.variant.startswith("at_cap")
            assert (it.fullmatch(v.bytes, max_threads=64) == "overflow") == F.needs_wide(v) == (over or family == "over128"), v
            assert (it.fullmatch(v.bytes, max_threads=128) == "overflow") == (over and family == "over128"), v
            res, fields = o.process_value(v.bytes)
            assert (res == 0) == (v.variant != "ends") and it.fullmatch(v.bytes, max_threads=4096) != "overflow", v
