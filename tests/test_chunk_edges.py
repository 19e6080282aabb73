"""The chunk-edge corpus of tests/helpers/chunk_edges.py, without a GPU: that every case does what its label says (conditions on the
INPUTS of tests/test_gpu_chunk_edges.py, so that test cannot pass on a degenerate corpus), that every (offset, residue) pair is there
for every kind, that the instantiation table runs what the families declare, and that the product's own compiled tables -- walked by
the host interpreters (tests/helpers/table_interp.py, tests/helpers/nfa_atomic_interp.py, the backtracking program's host walk of
tests/native/bt_host_check.cpp) -- give the oracle's answer on every line.  A mismatch on the GPU is then a kernel's, not the tables'.
For run_stop the tables' own quiet / steady masks say that the run bytes are quiet and byte p is not: the kernels' run scans are on
the path."""
import collections
import json
import os

import numpy as np
import pytest

from loongcollector_amd import binding as B
from oracle.oracle import OracleRegex
from tests.helpers import chunk_edges as ce
from tests.helpers import nfa_atomic_interp as nai
from tests.helpers.nfa_atomic_interp import AtomicNfaInterp, exit_of
from tests.helpers.table_interp import NfaInterp, TdfaInterp, TdfaL2BlobInterp
from tests.test_backref import host_vm  # noqa: F401  (fixture: builds tests/_build/libbt_host_check.so)

CORPORA = sorted({(f, r.walk) for r in ce.ROWS for f in r.families})
_cache = {}


def _flat(fam, res):
    """an oracle result as the row a kernel writes: groups 1..G of a full match, groups 0..G of a search"""
    return None if res is None else [v for be in (res if fam.search else res[1:]) for v in be]


def _oracle(name, walk="w256"):
    """(corpus, oracle handle, expected row per case) -- computed once"""
    if (name, walk) not in _cache:
        c = ce.generate(name, walk)
        o = OracleRegex(c.family.pattern)
        run = o.search if c.family.search else o.fullmatch
        _cache[name, walk] = (c, o, [_flat(c.family, run(k.line)) for k in c.cases])
    return _cache[name, walk]


@pytest.mark.parametrize("name,walk", CORPORA)
def test_every_offset_and_residue_is_there_for_every_kind(name, walk):
    c, o, exp = _oracle(name, walk)
    fam = c.family
    offsets, M = ce.WALKS[walk]
    assert (offsets, M) == {"w256": (ce.W256_P, 4), "w16": (ce.W16_P, 16), "w16r": (ce.W16R_P, 16)}[walk]
    # (w16r: the 16-byte walk and 16 consecutive offsets with room for a run of 40 bytes in front -- two whole 16-byte loads and a tail)
    assert set(ce.W16R_P) >= set(ce.W16_P) | set(range(42, 58)) and max(ce.RunCaptureFamily.BACK) + 2 == 42
    # 6 below .. 6 behind the first two chunk borders of the aligned view (line offset 256k - head), and the start of the value
    assert set(ce.W256_P) >= {b - h + d for b in (256, 512) for h in range(4) for d in range(-6, 7)} | set(range(6))
    seen = collections.defaultdict(set)
    needy = set()
    for k in c.cases:
        seen[k.kind].add((k.p, k.head))
        if k.kind == "run_to_end" and "needy" in k.variant:
            needy.add((k.p, k.head))
    assert set(seen) == set(fam.kinds)
    for kind, min_p in fam.kinds.items():
        assert seen[kind] == {(p, h) for p in offsets if p >= min_p for h in range(M)}, (name, kind)
    if fam.needy_min is not None:
        assert needy == {(p, h) for p in offsets if p >= fam.needy_min for h in range(M)}
    # both input forms give every kind every residue: by filler in the (off, len) form, from the lengths in the separator form
    for form in ("len", "sep"):
        data, off, length, residue = c.pack(form)
        assert len(off) == len(c.cases) + (form == "sep") and len(data) == int(off[-1]) + (int(length[-1]) + 1 if form == "len" else 0) + ce.GUARD_BYTES
        by_kind = collections.defaultdict(set)
        for i, k in enumerate(c.cases):
            assert bytes(data[int(off[i]):int(off[i]) + int(length[i])]) == k.line
            assert bytes(data[int(off[i]) + int(length[i]):][:1]) == (k.after or fam.after)               # the byte behind the line
            assert form == "sep" or int(residue[i]) == k.head
            by_kind[k.kind].add(int(residue[i]))
        assert all(v == set(range(M)) for v in by_kind.values()), (name, form, {k: sorted(v) for k, v in by_kind.items()})
    # (two corpora of the 16-byte walk hold more: log, whose size the screen test's figures fix, and lazy, the big family plus the misses)
    assert len(c.cases) <= (11000 if (name, walk) in (("log", "w16"), ("lazy", "w16")) else 9000) and max(len(s) for s in c.lines) <= 1100
    if name.startswith("over") or name in ("akept64", "avector64"):
        # the seeded shuffle mixes controls and overflowing values: some workgroup of four values holds both, and each alone
        groups = [{fam.overflows(k) for k in c.cases[i:i + 4]} for i in range(0, len(c.cases), 4)]
        assert {True, False} in groups and {True} in groups and {False} in groups, name


@pytest.mark.parametrize("name,walk", CORPORA)
def test_cases_do_what_their_label_says(name, walk):
    c, o, exp = _oracle(name, walk)
    fam = c.family
    run = o.search if fam.search else o.fullmatch
    counts = collections.Counter()
    for k, e in zip(c.cases, exp):
        what = (name, k.kind, k.variant, k.p)
        counts[k.kind, k.variant] += 1
        if name == "runcap" and k.kind == "run_stop":
            back = int(k.variant.rsplit("_", 1)[1])                                                   # the run [p - back, p) ends on the FIRST '|'
            assert e is not None and e[2:4] == [k.p - back, k.p] and k.line.index(b"|") == k.p, what
            assert k.line[k.p - back - 1:k.p - back] == b"!" and (back < 2 or e[5] < k.p), what        # (the next field ends inside the run)
        elif k.kind == "absent":
            assert e is not None and e[2:4] == [-1, -1] and e[1] == k.p - 1 and k.line[k.p:k.p + 1] != b"!" and b"|" in k.line, what
        elif k.kind == "overflow" and isinstance(fam, ce.LineageFamily):
            # (the exit families whose cap is the pattern's; that the step on byte p is the one: test_each_exit_is_taken_on_byte_p)
            v = k.variant[7:] if k.variant.startswith("at_cap_") else k.variant
            assert fam.overflows(k) == fam.over == (not k.variant.startswith("at_cap_")) == (name in ce.SIBLING), what
            assert k.line[k.p - (2 if isinstance(fam, ce.WorkFamily) else 1):k.p].endswith(b";a" if isinstance(fam, ce.WorkFamily) else b";"), what
            if isinstance(fam, ce.ClosedFamily):
                assert e is not None and (k.line[k.p:k.p + 1] == b",") == (v != "one_more"), what     # (a comma follows at once, or a run first)
            else:
                assert (e is not None) == (v in ("match", "far")) and k.line[k.p:k.p + 1] == (b"h" if isinstance(fam, ce.WorkFamily) else b"a"), what
            assert v != "far" or (len(k.line) - k.p > 300 and (isinstance(fam, ce.ClosedFamily) or e[-1] - e[-2] >= 300 or e[3] - e[2] >= 300)), what
            assert v != "ends" or len(k.line) == k.p + 1, what
        elif k.kind == "commit":
            n = int(k.variant.rsplit("_", 1)[1])
            assert k.line[k.p - n - 1:k.p - n] == b";" and all(97 <= b <= 122 for b in k.line[k.p - n:k.p]), what   # the run [p - n, p)
            if k.variant.startswith("match"):
                assert e is not None and e[4:6] == [k.p - n, k.p] and k.line[k.p:k.p + 1] == b"-", what
            elif k.variant.startswith("ends"):
                assert len(k.line) == k.p and e is not None and e[4:] == [k.p - n, k.p] + [-1] * 6 and run(k.line + k.after) is None, what
            else:                                                                                     # noback: the plain form gives "zabd" back
                pl = OracleRegex(fam.PLAIN).fullmatch(k.line)
                assert e is None and k.line[k.p - 4:k.p + 1] == b"zabd-" and pl is not None and pl[3] == (k.p - n, k.p - 4), what
        elif k.kind == "enter":
            assert e is not None and e[4] == k.p and k.line[k.p - 1:k.p] == b";", what                 # the group begins at p
            back = k.variant.split("_")[1] if "_" in k.variant else None
            assert back is None or k.line[k.p - 1 - int(back):k.p - int(back)] == b",", what           # field 2 is the steady run in front
        elif k.kind == "alt":
            pl = OracleRegex(fam.PLAIN).fullmatch(k.line)
            if k.variant == "first":
                assert e is not None and e[6:10] == [k.p - 2, k.p, k.p, k.p + 1], what
            elif k.variant == "second":
                assert e is not None and e[6:10] == [k.p - 1, k.p, k.p, k.p + 1], what
            elif k.variant == "second_would":
                assert e is None and pl is not None and pl[4] == (k.p - 2, k.p - 1) and pl[5] == (k.p - 1, k.p + 1), what
            else:
                assert k.variant == "ends" and e is None and len(k.line) == k.p and run(k.line + k.after) is not None, what
        elif k.kind == "doomed":
            assert b" " not in k.line[:k.p] and k.line[k.p:k.p + 1] == b" ", what                       # the first space is at p
            if k.variant == "hit":
                assert e is not None and e[:2] == [0, k.p], what
            elif k.variant in ("doomed", "doomed_S", "doomed_far"):
                assert k.line[k.p + 1:k.p + 3] != b"SA" and e is not None and e[1] >= k.p + {"doomed": 4, "doomed_S": 3, "doomed_far": 300}[k.variant], what
            else:
                assert e is None and (k.variant != "last_byte" or len(k.line) == k.p + 1), what
        elif k.kind == "overflow":
            m = fam.cap - (1 if k.variant.startswith("at_cap") else 0)
            assert k.line[k.p - m + 1:k.p + 1] == b"a" * m and k.line[k.p - m - 3:k.p - m + 1] == b";bbb" and fam.overflows(k) == (m == fam.cap), what
            v = k.variant[7:] if k.variant.startswith("at_cap") else k.variant
            assert (e is not None) == (v in ("match", "far")), what
            assert v != "match" or (e[-2] == k.p + 1 and e[-1] == len(k.line)), what                    # the run's last 'a' is the one
            assert v != "far" or (e[-2] >= k.p + 300 and len(k.line) - k.p > 300), what                # ... or one a chunk further on
            assert v != "ends" or len(k.line) == k.p + 1, what
            assert v != "one_more" or run(k.line[:-1]) is not None, what
            assert v != "match" or run(k.line + fam.after) is None, what                              # (the byte behind it, read, would refuse it)
        elif k.kind in ("run_stop", "stamp"):
            assert e is not None and k.p in e, what                                                  # a capture begins or ends at p
            if k.variant.startswith("one_byte"):
                assert any(e[2 * g] == k.p and e[2 * g + 1] == k.p + 1 for g in range(len(e) // 2)), what
            if k.variant.startswith("empty"):
                assert any(e[2 * g] == k.p == e[2 * g + 1] for g in range(len(e) // 2)), what
        elif k.kind == "run_to_end":
            assert len(k.line) == k.p, what
            if name == "runcap":                                                                      # the run reaches the end of the value; the byte behind belongs to its set
                assert e is not None and e[2] >= 2 and e[3] == k.p and b"|" not in k.line[e[2]:] and k.after == b"u", what
            if "needy" in k.variant:                                                                  # the byte behind it changes the result
                assert _flat(fam, run(k.line + k.after)) != e, what
        elif k.kind == "dead":
            assert e is None and run(k.line[:k.p] + k.line[k.p + 1:]) is not None, what              # ... and matches without byte p
            assert run(k.line[:k.p] + k.line[k.p + 1:k.p + 2] + k.line[k.p + 1:]) is not None, what   # (byte p is what kills it: another one there matches)
        elif k.kind == "absorb":
            assert e is not None and e[-2] == k.p and e[-1] == len(k.line) >= k.p + 300, what
        elif k.kind == "threads":
            if k.variant.endswith("to_end"):
                assert e is None and len(k.line) == k.p and run(k.line + k.after) is not None, what
            else:
                live = int(k.variant[4:])
                g = 8 - live                                                                          # the first alternative still alive
                assert e is not None and e[2 * g:2 * g + 2] == [0, k.p] and e[-2] == k.p + 1, what
        elif k.kind == "search_start":
            v = k.variant
            if v != "d_behind":
                assert fam.START not in k.line[:k.p] and k.line[k.p:k.p + 1] == fam.START, what       # the first start byte is at p
            if v.startswith("a_match"):
                assert e is not None and e[0] == k.p, what
                assert v != "a_match_at_end" or e[1] == len(k.line), what
            elif v == "b_doomed":
                assert k.line[k.p:k.p + 2] == fam.DOOMED and e is not None and e[0] == k.p + 4, what
            elif v == "b_doomed_far":
                assert e is not None and e[0] == k.p + 302, what                                      # the match begins in a later chunk
            elif v in ("b_doomed_alone", "c_last_byte"):
                assert e is None and (v != "c_last_byte" or len(k.line) == k.p + 1), what
            elif v == "d_behind":
                assert k.line[k.p - 1:k.p] == fam.BEHIND and k.line[k.p:].startswith(fam.HIT) and e is not None and e[0] > k.p, what
            elif v == "needy":
                assert e is None and _flat(fam, run(k.line + k.after))[0] == k.p, what
            else:
                raise AssertionError(what)
        elif k.kind == "miss":
            # alternating up to p - 2, a 'b' there and a second one at p - 1; what comes of it is the variant's.  That the partial
            # automaton's walk ends on byte p is said by test_the_lazy_family_misses_where_it_says_and_nowhere_else
            assert k.line[:2] == b",;" and k.line[k.p - 2:k.p] == b"bb", what
            assert all(x != y and {x, y} == set(b"ab") for x, y in zip(k.line[2:k.p - 2], k.line[3:k.p - 1])), what
            assert (e is not None) == (k.variant in ("last", "far")), what
            assert k.variant != "last" or (k.line[k.p] == ord("c") and e[4] == k.p), what              # the second 'b' is the stretch's last byte
            assert k.variant != "far" or e[4] >= k.p + 300, what
            assert k.variant != "no_match" or (k.line[k.p] == ord("Z") and run(k.line[:k.p] + k.line[k.p + 1:]) is not None), what
            assert k.variant != "needy" or (len(k.line) == k.p + 2 and run(k.line + k.after) is not None), what
        elif k.kind == "resume":
            assert k.frm in (k.p - 1, k.p, k.p + 1), what
            r = _flat(fam, o.search(k.line, k.frm))
            gap = {"at_from": 0, "at_from1": 1, "next_chunk": 300}[k.variant.split("_", 1)[1]]
            assert r is None or r[0] >= k.frm, what
            if k.frm > len(fam.HIT):                                             # (the line's first hit lies in front)
                assert r is not None and r[0] == k.frm + gap and e[0] == 0, what
        else:
            raise AssertionError(what)
    assert all(n >= len(ce.WALKS[walk][0]) for n in counts.values()) or name in ("threads",), counts  # no variant is a rarity
    for kind in fam.kinds:
        assert sum(n for (kd, _), n in counts.items() if kd == kind) >= 100, (name, kind)


def test_the_instantiation_table_runs_what_the_families_declare():
    """every family is run by some row, every row runs every kind of its families (>= 90 % is the cap the table must meet; a case
    set a row leaves out would be an entry of the table), search rows have search families, the edge families belong to their rows"""
    assert {f for r in ce.ROWS for f in r.families} == set(ce.FAMILIES)
    assert len({r.id for r in ce.ROWS}) == len(ce.ROWS) == 29
    assert {r.kernel for r in ce.ROWS} == {"nfa_match_kernel", "nfa_match_kernel<atomic>", "nfa_wide_kernel:first", "tdfa_l2_kernel:wave",
                                           "tdfa_l2_kernel", "nfa_decide_kernel", "nfa_dfs_kernel", "bt_match_kernel",
                                           "tdfa_l2_kernel:wave:lazy", "tdfa_l2_kernel:lazy", "nfa_wide_kernel", "tdfa_stream_kernel*"}
    for r in ce.ROWS:
        for f in r.families:
            c = ce.generate(f, r.walk)
            ran = {k.kind for k in c.cases}                                                           # a row runs the whole corpus
            assert len(ran) >= 0.9 * len(ce.FAMILIES[f].kinds) and ran == set(ce.FAMILIES[f].kinds), (r.id, f)
        assert ce.EDGE_FAMILY[r.id] in r.families
        assert set(r.env) <= set(ce.ENV_KEYS)
    lazy = [r for r in ce.ROWS if r.train]
    assert [(r.id, r.walk, r.train, r.families) for r in lazy] == [
        ("lazy-wave", "w256", "family", ("lazy",)), ("lazy-lane", "w16", "family", ("lazy",)),
        ("lazy-wave-decided", "w256", "corpus", ("log", "threads")), ("lazy-lane-decided", "w16", "corpus", ("log", "threads"))]
    assert all(r.compile_engine == r.launch_engine == B.LC_ENGINE_NFA and "LC_LAZY_TDFA" not in r.env for r in lazy)
    assert all((r.env.get("LC_TDFA_WAVE_MAX") == "0") == (r.walk == "w16") for r in lazy)              # the lane walk is the one with 16-byte pieces
    unstaged = [r for r in ce.ROWS if r.min_n]
    assert [r.id for r in unstaged] == ["wave-unstaged"] and unstaged[0].min_n == ce.UNSTAGED_ABOVE + 1 and unstaged[0].families == ("big",)
    n = len(ce.generate("big").cases)
    copies = -(-unstaged[0].min_n // n)
    assert ce.UNSTAGED_ABOVE < copies * n <= 65536                                                    # still a wave launch (LC_TDFA_WAVE_MAX)
    assert {r.id for r in ce.SEARCH_ROWS} == {"nfa", "nfa-atomic", "nfa-wide-first", "wave-small-staged", "decide", "dfs"}
    # the rows of the chain's hand-offs, of the slot widths and of the run capture: one family each, the plain NFA launch
    by_id = {r.id: r for r in ce.ROWS}
    new = {"chain64": ("nfa_wide_kernel", "over64"), "chain128": ("nfa_decide_kernel", "over128"), "chain-slots": ("nfa_decide_kernel", "over64s"),
           "nfa-ns64": ("nfa_match_kernel", "log64"), "nfa-ns128": ("nfa_match_kernel", "log128"), "nfa-ns320": ("nfa_match_kernel", "log320"),
           "runcap-nfa": ("nfa_match_kernel", "runcap")}
    for rid, (kernel, family) in new.items():
        r = by_id[rid]
        assert (r.kernel, r.families, ce.EDGE_FAMILY[rid]) == (kernel, (family,), family), rid
        assert (r.compile_engine, r.launch_engine, r.env, r.wave, r.dfs, r.min_n, r.train) == (B.LC_ENGINE_NFA, B.LC_ENGINE_NFA, {"LC_LAZY_TDFA": "0"},
                                                                                           False, False, 0, None), rid
        assert r.walk == ("w16r" if family == "runcap" else "w256")
    assert [(r.id, r.kernel, r.families, r.walk, r.compile_engine, r.launch_engine, r.wave) for r in ce.ROWS if r.id in ("runcap-wave", "runcap-lds")] == [
        ("runcap-wave", "tdfa_l2_kernel:wave", ("runcap",), "w16r", B.LC_ENGINE_AUTO, B.LC_ENGINE_TDFA, True),
        ("runcap-lds", "tdfa_stream_kernel*", ("runcap",), "w16r", B.LC_ENGINE_AUTO, B.LC_ENGINE_TDFA, False)]
    # nfa_wide_kernel<64> as the first chance: the 64-slot family, not the wider ones (NS > 64 never goes wide first)
    assert by_id["nfa-wide-first"].families == ("log", "quasi", "look", "threads", "over64", "over128", "log64")
    # the atomic instantiation: one row of ordinary families, one row per overflow exit (a family and its sibling control share it)
    atomic = {"nfa-atomic-edges": ("alog", "acommit", "aquasi"), "achain-kept64": ("akept64",), "achain-vector64": ("avector64",),
              "achain-lineage6": ("alineage6", "alineage6c"), "achain-closed64": ("aclosed64", "aclosed64c"), "achain-work10": ("awork10", "awork10c")}
    for rid, families in atomic.items():
        r = by_id[rid]
        assert (r.kernel, r.families, r.walk, ce.EDGE_FAMILY[rid]) == ("nfa_match_kernel<atomic>", families, "w256", families[0]), rid
        assert (r.compile_engine, r.launch_engine, r.env, r.wave, r.dfs, r.min_n, r.train) == (B.LC_ENGINE_NFA, B.LC_ENGINE_NFA, {"LC_LAZY_TDFA": "0"},
                                                                                           False, False, 0, None), rid
    assert [r.id for r in ce.ROWS if r.kernel == "nfa_match_kernel<atomic>"] == ["nfa-atomic"] + list(atomic)
    achain = {(rid, f) for rid, fs in atomic.items() if rid.startswith("achain-") for f in fs}
    assert set(ce.ACHAIN) == achain and all(ce.CHAIN[k] == (("nfa_match_kernel<atomic>", "nfa_decide_kernel"),
                                                            ("nfa_wide_kernel", "nfa_wide_kernel:first", "nfa_match_kernel")) for k in achain)
    assert {f for _, f in achain} == set(ce.ATOMIC_EXITS) | set(ce.SIBLING.values()) and set(ce.SIBLING) < set(ce.ATOMIC_EXITS)
    assert set(ce.AT_CAP) == (set(ce.ATOMIC_EXITS) - set(ce.SIBLING)) | set(ce.SIBLING.values())
    assert set(ce.CHAIN) == {("chain64", "over64"), ("chain128", "over128"), ("chain-slots", "over64s"), ("nfa-wide-first", "over64"),
                             ("nfa-wide-first", "over128")} | achain and set(ce.DECIDES) == {k for k, (has, _) in ce.CHAIN.items() if "nfa_decide_kernel" in has}
    for (rid, family), (has, has_not) in ce.CHAIN.items():
        assert family in by_id[rid].families and by_id[rid].kernel in has and not set(has) & set(has_not)
        assert "nfa_wide_kernel:first" in (has if rid == "nfa-wide-first" else has_not)
    assert set(ce.NS_ROWS) == {rid for rid in new if rid.startswith("nfa-ns")}


# ---- the product's tables on the host

def _check(c, exp, walkers, label):
    """every case through every walker (name, fn(line) -> row or None) against the oracle's row"""
    for name, fn in walkers:
        bad = [i for i, (k, e) in enumerate(zip(c.cases, exp)) if fn(k.line) != e]
        assert not bad, "%s, %s: %d cases differ %s; first: %s" % (label, name, len(bad), c.kinds_of(bad), c.label(bad[0]))


def _l2_trace(it, s):
    """[(state before byte i, quiet in that state: stays without a program and its class is in the state's QUIET mask)] of the L2 blob"""
    out, state = [], it.start
    for b in s:
        if state == 0 or state == it.absorb:
            break
        cls = int(it.cmap[b])
        t = int(it.trans[state * it.ncls + cls])
        masked = cls < 64 and bool((int(it.quiet[state]) >> cls) & 1)
        assert masked == ((t >> 16) == 0 and (t & 0xFFFF) == state), (state, cls)                     # the mask says what the table says
        out.append((state, masked))
        state = t & 0xFFFF
    return out


def _run_of(k):
    """the bytes [first, p) of a run_stop case that the run scan must find quiet: behind the run's first byte, which may enter the state"""
    tail = k.variant.rsplit("_", 1)[1]
    return (k.p - int(tail) if tail.isdigit() else 0) + 1


@pytest.mark.parametrize("name,walk", [(f, w) for f, w in CORPORA if any(r.launch_engine == B.LC_ENGINE_TDFA and f in r.families for r in ce.ROWS)])
def test_global_memory_tdfa_tables_give_the_oracles_rows(name, walk):
    c, o, exp = _oracle(name, walk)
    fam = c.family
    rx = B.GpuRegex(fam.pattern, syntax_flags=fam.flags)
    assert rx.info()["engine"] == B.LC_ENGINE_TDFA
    if name == "big":
        assert rx.info()["states"] > 1000 and rx.table(B.LC_TABLE_TDFA_BLOB, np.uint32) is None       # no LDS kernel can run it
    else:
        assert rx.prefer_wave_tdfa()
    it = TdfaL2BlobInterp(rx)
    assert it.miss == 0 and (fam.search or it.absorb != 0)
    # the register programs fit the share of LDS a launch of up to 32 768 values stages them in (gpu_runtime.hip launchTdfaL2Family):
    # the rows named "staged" are, and the row above that count is the same walk with the programs in global memory
    blob = rx.table(B.LC_TABLE_TDFA_L2_BLOB, np.uint32)
    prog_bytes = (int(blob[9]) - int(blob[7]) + 3) & ~3                                               # TL_OFF_FINALID - TL_OFF_OPSSTART
    assert 0 < prog_bytes <= 40 * 1024 and it.nregs * 4 * 4 + prog_bytes <= 60 * 1024, (name, prog_bytes)
    _check(c, exp, (("tdfa_wave_kernel's walk", it.fullmatch_wave), ("tdfa_l2_kernel's walk", it.fullmatch)), name)
    ends_quiet = 0
    for k in c.cases:
        if name == "runcap":
            continue                                                                                  # (its events are run_capture_kernel's, not the automaton's)
        if k.kind == "run_stop":
            tr = _l2_trace(it, k.line)
            first = _run_of(k)
            assert all(q for _, q in tr[first:k.p]) and not tr[k.p][1], (name, k.variant, k.p)        # quiet up to p, not at p
            assert k.p - first < 1 or len({s for s, _ in tr[first:k.p + 1]}) == 1
        elif k.kind == "run_to_end" and k.p >= 2:
            tr = _l2_trace(it, k.line)
            # the value ends inside a quiet run (or on the byte that enters it)
            assert len(tr) == k.p and (tr[-1][1] or it.cmap[k.line[-1]] != it.cmap[k.line[-2]]), (name, k.variant, k.p)
            ends_quiet += tr[-1][1]
        elif k.kind == "absorb":
            tr = _l2_trace(it, k.line)
            # (byte p carries the program that stamps the begin of (.*); the absorbing state is what it leads to)
            assert len(tr) == k.p + 1 and tr[k.p][0] != it.absorb, (name, k.p)
        elif k.kind == "dead":
            assert len(_l2_trace(it, k.line)) == k.p + 1, (name, k.p)                                 # the dead state behind byte p
        elif k.kind == "resume":
            want = _flat(fam, o.search(k.line, k.frm))
            assert it.fullmatch_wave(k.line, start=k.frm) == want and it.fullmatch(k.line, start=k.frm) == want, c.label(c.cases.index(k))
    assert fam.search or name == "runcap" or ends_quiet >= 0.8 * sum(k.kind == "run_to_end" and k.p >= 2 for k in c.cases)
    if name == "runcap":
        # the run group survives in the tagged DFA, inside the optional branch: the tables stamp its begin, the end is the run kernel's
        assert [g for g, _ in rx.run_captures()] == [1] and rx.run_captures()[0][1] == frozenset(range(256)) - {ord("|")}
        assert rx.table(B.LC_TABLE_TDFA_BLOB, np.uint32) is not None                                  # (the LDS kernels can run it: row runcap-lds)


def _nfa_trace(it, s, start=0, end=False):
    """NfaInterp's walk once more, step by step: [(live threads, every one of them steady on this byte)] per byte; end: and the
    threads the step on the last byte leaves, as (count, None)"""
    threads, prev = ([it.npos], it.ncls) if not start else ([0], int(it.cmap[s[start - 1]]))
    out = []
    for pos in range(start, len(s)):
        if it.search_suffix >= 0 and threads == [it.search_suffix]:
            break
        cls = int(it.cmap[s[pos]])
        nxt = int(it.cmap[s[pos + 1]]) if pos + 1 < len(s) else -1

        def quiet(p):
            if (it.stable[p] >> cls) & 1:
                return True
            if nxt < 0 or it.quasi_idx is None or p >= len(it.quasi_idx) or not int(it.quasi_idx[p]):
                return False
            return bool((it.quasi_rows[int(it.quasi_idx[p]) - 1][cls] >> nxt) & 1)
        steady = all(quiet(p) for p in threads)
        out.append((len(threads), steady))
        if not steady:
            holds = it.behind[prev] | it.ahead[cls]
            new = []
            for p in threads:
                for tgt, cond, _ in it.follow[p]:
                    if tgt >= 0 and tgt not in new and (it.posmask[tgt] >> cls) & 1 and not (cond & ~holds):
                        new.append(tgt)
            if it.search_suffix in new:
                new = new[:new.index(it.search_suffix) + 1]
            threads = new
        prev = cls
        if not threads:
            break
    if end:
        out.append((len(threads), None))
    return out


# (the lazy family's program: test_the_lazy_family_misses_where_it_says_and_nowhere_else walks it on the values the kernels hand it)
OVER = ("over64", "over128", "over64s")
# (... and the atomic instantiation's: test_atomic_walks_give_the_oracles_rows_and_the_gates_are_sound and the tests behind it)
ATOMIC_NEW = ("alog", "acommit", "aquasi") + tuple(ce.ATOMIC_EXITS) + tuple(ce.SIBLING.values())


# (... and the overflow families': test_the_overflow_families_exceed_each_cap_by_the_step_on_byte_p, with the caps the kernels have)
@pytest.mark.parametrize("name", sorted({f for r in ce.ROWS if r.compile_engine == B.LC_ENGINE_NFA for f in r.families} - {"lazy"} - set(OVER) - set(ATOMIC_NEW)))
def test_nfa_program_gives_the_oracles_rows(name):
    walk = "w16r" if name == "runcap" else "w256"
    c, o, exp = _oracle(name, walk)
    fam = c.family
    rx = B.GpuRegex(fam.pattern, syntax_flags=fam.flags, engine=B.LC_ENGINE_NFA)
    assert (rx.atomic_groups()[0] > 0) == (name == "atomic")
    it = (AtomicNfaInterp if name == "atomic" else NfaInterp)(rx)
    assert (it.search_suffix >= 0) == fam.search
    if name == "quasi":
        assert it.quasi_rows                                                                          # doomed-spawn rows exist for this shape
    if isinstance(fam, ce.NestedLogFamily):
        # nesting d deep: 4 d groups and 8 d slots on the log family's 7 positions -- each instantiation at its exact fit
        assert (o.groups, it.nslots, it.npos) == (4 * fam.depth, 8 * fam.depth, 7) and it.nslots == int(name[3:]) in (64, 128, 320)
        assert B.GpuRegex(fam.pattern).info()["engine"] == (B.LC_ENGINE_NFA if fam.depth == 40 else B.LC_ENGINE_TDFA)
        assert ce.NS_ROWS[ce.ROWS[[r.families for r in ce.ROWS].index((name,))].id] == it.nslots
    if name == "runcap":
        assert [g for g, _ in rx.run_captures()] == [1]                                               # the run group survives, inside the optional branch
    _check(c, exp, (("the thread-list walk", it.fullmatch),), name)
    for k in c.cases:
        if name == "runcap":
            continue                                                                                  # (its events are run_capture_kernel's, not the program's)
        if k.kind == "run_stop":
            tr = _nfa_trace(it, k.line)
            first = _run_of(k)
            assert all(q and n <= 6 for n, q in tr[first:k.p]) and not tr[k.p][1], (name, k.variant, k.p)   # steady up to p, not at p
        elif k.kind == "threads":
            tr = _nfa_trace(it, k.line)
            live = int(k.variant.split("_")[0][4:])
            first = 8 - live + 1
            assert all(t == (live, True) for t in tr[first:k.p]), (k.variant, k.p, tr[first:first + 3])
            assert k.p >= len(k.line) or not tr[k.p][1]
        elif k.kind == "search_start" and k.variant in ("a_match", "b_doomed", "c_last_byte"):
            tr = _nfa_trace(it, k.line)
            assert all(t == (1, True) for t in tr[1:k.p]), (name, k.variant, k.p)                      # the prefix thread alone, steady up to p
            if k.variant == "b_doomed" and name in ("quasi", "look") and k.p >= 1:
                assert tr[k.p] == (1, True)                                                           # ... and on the doomed start: its rows say so
            if k.variant == "a_match":
                assert not tr[k.p][1]
        elif k.kind == "resume" and name != "atomic":
            assert it.fullmatch(k.line, start=k.frm) == _flat(fam, o.search(k.line, k.frm)), c.label(c.cases.index(k))
    kinds = {k.kind for k in c.cases}
    assert name != "threads" or {int(k.variant.split("_")[0][4:]) for k in c.cases} >= {8, 7, 6, 1}    # beyond, at and below kNfaSteadyScanThreads


@pytest.mark.parametrize("depth,slots,engine", [(6, 48, B.LC_ENGINE_TDFA), (12, 96, B.LC_ENGINE_TDFA), (20, 160, B.LC_ENGINE_TDFA), (40, 320, B.LC_ENGINE_NFA)])
def test_nesting_the_log_family_gives_eight_slots_a_level(depth, slots, engine):
    """nesting d gives 4 d groups and 8 d slots on 7 positions; AUTO takes the tagged DFA up to depth 20 and the thread-list program at 40"""
    fam = ce.NestedLogFamily(depth)
    it = NfaInterp(B.GpuRegex(fam.pattern, engine=B.LC_ENGINE_NFA))
    assert (OracleRegex(fam.pattern).groups, it.nslots, it.npos) == (4 * depth, slots, 7)
    assert B.GpuRegex(fam.pattern).info()["engine"] == engine
    line = b"xy,12;uv w z"
    want = [v for be in OracleRegex(fam.pattern).fullmatch(line)[1:] for v in be]
    assert it.fullmatch(line) == want == [v for be in ((0, 2), (3, 5), (6, 8), (9, 12)) for _ in range(depth) for v in be]


@pytest.mark.parametrize("name", OVER)
def test_the_overflow_families_exceed_each_cap_by_the_step_on_byte_p(name):
    """What rows chain64 / chain128 / chain-slots rest on.  The programs have 74 / 144 / 74 positions and 6 / 6 / 66 slots.  On every
    case the thread list first exceeds the family's cap BY THE STEP ON BYTE p (cap threads behind byte p - 1, cap + 1 behind byte p)
    and the `at_cap` controls peak at exactly the cap, behind byte p, and exceed it nowhere.  The walk with nfa_match_kernel's 64
    threads says "overflow" exactly on over64's overflow variants (and on every over128 case from its 65th thread on), with
    nfa_wide_kernel's 128 it decides all of over64 and says "overflow" exactly on over128's overflow variants, and with room for
    every thread it gives the oracle's row everywhere."""
    c, o, exp = _oracle(name)
    fam = c.family
    rx = B.GpuRegex(fam.pattern, engine=B.LC_ENGINE_NFA)
    assert rx.info()["engine"] == B.LC_ENGINE_NFA and rx.atomic_groups()[0] == 0
    it = NfaInterp(rx)
    assert (it.npos, it.nslots, fam.cap) == {"over64": (74, 6, 64), "over128": (144, 6, 128), "over64s": (74, 66, 64)}[name]
    assert it.search_suffix < 0 and not it.quasi_rows
    over = [fam.overflows(k) for k in c.cases]
    assert collections.Counter((k.variant, v) for k, v in zip(c.cases, over)) == dict(
        [((v, True), 136) for v in ("match", "far", "ends", "one_more")] + [((v, False), 136) for v in ("at_cap_match", "at_cap_far")])
    walked = set()
    for k, e, ov in zip(c.cases, exp, over):
        what = (name, k.variant, k.p)
        if k.line in walked:
            continue                                                                                  # (the same bytes at another residue)
        walked.add(k.line)
        counts = [n for n, _ in _nfa_trace(it, k.line, end=True)]                                     # counts[i]: live threads in front of byte i
        assert counts[k.p] == fam.cap - (0 if ov else 1) and counts[k.p + 1] == counts[k.p] + 1, what  # the step on byte p adds the last one
        assert max(counts[:k.p + 1]) <= fam.cap and max(counts) == fam.cap + (1 if ov else 0), what
        for cap in (64, 128, 4096):
            got = it.fullmatch(k.line, max_threads=cap)
            assert got == ("overflow" if ov and fam.cap >= cap or fam.cap > cap else e), what + (cap,)
    assert len(walked) == len(c.cases) // 4


def test_backtracking_program_gives_the_oracles_rows(host_vm):  # noqa: F811
    c, o, exp = _oracle("backref")
    rx = B.GpuRegex(c.family.pattern)
    assert rx.info()["engine"] == B.LC_ENGINE_BT                                                      # only the backtracking engine runs it

    def walk(line):
        r, caps = host_vm(rx, line)
        assert r >= 0
        return caps[2:] if r else None
    _check(c, exp, (("btRun on the host", walk),), "backref")


# ---- the lazy front: conditions on the corpus and on the training lines

LAZY_ROWS = [r for r in ce.ROWS if r.train]


def _lazy_walks(rx):
    it = TdfaL2BlobInterp(rx, B.LC_TABLE_LAZY_TDFA_BLOB)
    assert it.miss != 0
    return it, (("tdfa_wave_kernel's walk", it.fullmatch_wave), ("tdfa_l2_kernel's walk", it.fullmatch))


@pytest.mark.parametrize("walk", ["w256", "w16"])
def test_the_lazy_family_misses_where_it_says_and_nowhere_else(walk):
    """The `{14}` pattern is a thread-list program; trained once on the family's training lines (none of them a case) its partial
    automaton decides every training line and every case but the `miss` ones as the oracle does, and every `miss` case steps on an
    uncomputed transition ON BYTE p: the value cut behind byte p - 1 is decided, cut behind byte p it is a miss.  The thread-list
    program, which the kernels hand those values to, gives the oracle's row on each of them."""
    c, o, exp = _oracle("lazy", walk)
    fam = c.family
    assert B.GpuRegex(fam.pattern).info()["engine"] == B.LC_ENGINE_NFA                                 # it does not determinise
    row = next(r for r in LAZY_ROWS if r.walk == walk and r.train == "family")
    rx = B.GpuRegex(fam.pattern, engine=row.compile_engine)
    training = ce.training_lines(row, "lazy")
    assert len(training) == len(set(training)) >= 300 and not set(training) & set(c.lines)
    assert max(len(t) for t in training) >= max(ce.WALKS[walk][0]) + 80                                # stretch lengths span the offsets
    r = rx.lazy_train(training)
    assert r["in_use"] == 1 and r["sample_misses"] == 0 and 50 <= r["states"] <= 1000, r
    it, walks = _lazy_walks(rx)
    counts = collections.Counter((k.kind, k.variant) for k in c.cases if k.kind == "miss")
    per = len([p for p in ce.WALKS[walk][0] if p >= fam.kinds["miss"]]) * ce.WALKS[walk][1]
    assert counts == {("miss", v): per for v in ("last", "far", "no_match", "needy")} and per == {"w256": 136, "w16": 272}[walk], counts
    for name, fn in walks:
        assert not [t for t in training if fn(t) == it.MISS], name
        bad = [i for i, (k, e) in enumerate(zip(c.cases, exp)) if (fn(k.line) == it.MISS) != (k.kind == "miss")]
        assert not bad, "%s: %d cases miss or fail to %s; first: %s" % (name, len(bad), c.kinds_of(bad), c.label(bad[0]))
        bad = [i for i, (k, e) in enumerate(zip(c.cases, exp)) if k.kind != "miss" and fn(k.line) != e]
        assert not bad, "%s: %d decided cases differ %s; first: %s" % (name, len(bad), c.kinds_of(bad), c.label(bad[0]))
        for k in c.cases:
            if k.kind == "miss":
                assert fn(k.line[:k.p]) is None and fn(k.line[:k.p + 1]) == it.MISS, (name, k.variant, k.p)   # decided up to p, gone on byte p
    nfa = NfaInterp(rx)
    missed = {k.line: e for k, e in zip(c.cases, exp) if k.kind == "miss"}
    assert all(nfa.fullmatch(line) == e for line, e in missed.items())


@pytest.mark.parametrize("walk", ["w256", "w16"])
def test_a_lazy_automaton_trained_again_on_its_misses_is_another_automaton(walk):
    """tests/test_gpu_chunk_edges.py launches rows lazy-wave and lazy-lane, hands the family's `miss` lines to lazy_train and launches
    the SAME handle again (gpu_runtime.hip ensureLazyUploaded: a new version, a new header, a new device copy).  Here: before the
    second call exactly the `miss` cases miss (544 of the 256-byte walk's corpus), after it no case does, every case is decided as the
    oracle decides it, and the blob has grown (1640 -> 1796 words for the 256-byte walk's lines): the second launch walks different
    tables."""
    c, o, exp = _oracle("lazy", walk)
    row = next(r for r in LAZY_ROWS if r.walk == walk and r.train == "family")
    rx = ce.compile_row(row, "lazy")
    it, walks = _lazy_walks(rx)
    words = len(rx.table(B.LC_TABLE_LAZY_TDFA_BLOB, np.uint32))
    missed = [i for i, k in enumerate(c.cases) if it.fullmatch(k.line) == it.MISS]
    assert missed == [i for i, k in enumerate(c.cases) if k.kind == "miss"] and len(missed) == {"w256": 544, "w16": 1088}[walk]
    again = ce.miss_lines(walk)
    assert len(again) == len(missed) // ce.WALKS[walk][1] and set(again) == {c.cases[i].line for i in missed}
    r = rx.lazy_train(again)
    assert r["in_use"] == 1 and r["sample_misses"] == 0, r
    it, walks = _lazy_walks(rx)
    grown = len(rx.table(B.LC_TABLE_LAZY_TDFA_BLOB, np.uint32))
    assert grown > words and (walk != "w256" or (words, grown) == (1640, 1796)), (words, grown)
    for name, fn in walks:
        assert not [k for k in c.cases if fn(k.line) == it.MISS], name
    _check(c, exp, walks, "lazy, trained again")


@pytest.mark.parametrize("row", [r for r in LAZY_ROWS if r.train == "corpus"], ids=lambda r: r.id)
def test_small_families_trained_on_their_first_lines_decide_the_rest(row):
    """log and threads as thread-list programs, trained on the first 200 lines of their corpus: the partial automaton is complete
    for what the corpus holds -- no case misses, every case is decided as the oracle decides it.  These rows run the decided path."""
    for family in row.families:
        c, o, exp = _oracle(family, row.walk)
        rx = B.GpuRegex(c.family.pattern, syntax_flags=c.family.flags, engine=row.compile_engine)
        training = ce.training_lines(row, family)
        assert training == c.lines[:ce.TRAIN_CORPUS] and len(training) == 200
        assert rx.lazy_train(training)["in_use"] == 1
        it, walks = _lazy_walks(rx)
        for name, fn in walks:
            assert not [k for k in c.cases if fn(k.line) == it.MISS], (family, name)
        _check(c, exp, walks, "%s, lazy" % family)


# ---- dfa_screen_kernel's corpus

def _screen(name):
    """(corpus, oracle's yes/no per case, the screen's walk) -- computed once"""
    if ("screen", name) not in _cache:
        c = ce.screen_corpus(name)
        base, o, exp = _oracle(name, "w16")
        assert c.cases[:len(base.cases)] == base.cases                                                # the w16 corpus, whole, and the cuts behind it
        run = o.search if c.family.search else o.fullmatch
        scr = ce.compile_screen(name)
        want = [e is not None for e in exp] + [run(k.line) is not None for k in c.cases[len(base.cases):]]
        _cache["screen", name] = (c, want, ce.ScreenWalk(TdfaInterp(scr)), TdfaInterp(scr))
    return _cache["screen", name]


@pytest.mark.parametrize("name", ce.SCREEN_FAMILIES)
def test_relaxed_screens_say_what_the_oracle_says_on_the_w16_corpus(name):
    """What tests/test_gpu_screen_edges.py expects is TdfaInterp(screen).fullmatch over the screen's tables: on this corpus that is
    the oracle's answer on EVERY case (the relaxation gives nothing away here), neither all yes nor all no, and the walk as the kernel
    does it -- leaving on the sink -- says the same."""
    c, want, walk, it = _screen(name)
    o = OracleRegex(c.family.pattern)
    run = o.search if c.family.search else o.fullmatch
    got = [it.fullmatch(k.line) is not None for k in c.cases]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, "%s: %d cases differ %s; first: %s" % (name, len(bad), c.kinds_of(bad), c.label(bad[0]))
    assert 0.20 <= 1 - sum(got) / len(got) <= 0.60, (name, sum(got), len(got))
    # accepted of all; the search families: 544 values that end with their match, each cut twice, on top of the w16 corpus -- without
    # them 19 %, 13 % and 19 % of quasi, look and atomic are rejected, with them 28 %, 22 % and 28 %
    cuts = [k for k in c.cases if k.kind == "cut"]
    assert len(cuts) == (2 * 544 if c.family.search else 0) and not any(w for k, w in zip(c.cases, want) if k.kind == "cut")
    assert all(run(k.line + k.after) is not None for k in cuts if k.variant == "needy_1")             # the byte behind it would complete the match
    assert {"log": (7552, 10672), "big": (6048, 8704), "quasi": (7024, 8656 + 1088), "look": (7552, 8640 + 1088), "atomic": (7024, 8656 + 1088),
            "threads": (2512, 5024)}[name] == (sum(got), len(got))
    assert [walk.walk(k.line)[0] for k in c.cases] == got
    assert it.fullmatch(b"") is None                                                                  # a value of length 0 is never accepted


def test_screen_events_fall_on_both_sides_of_the_first_two_piece_borders():
    """(kind, border, head) for border = 16, 32 of the aligned view and every head 0..15: a value that ENDS exactly on the border
    (head + L = border) in every family; the sink reached on the LAST byte of a piece (the walk must not fetch the next) in the
    families together, and in `threads` alone.  A screen is a search: none of the six has a transition to the dead state, so the
    kernel's `state != 0` never decides here and there is no such triple to ask for."""
    every = {(b, h) for b in ce.SCREEN_BORDERS for h in range(16)}
    absorbed = collections.defaultdict(set)
    for name in ce.SCREEN_FAMILIES:
        c, want, walk, it = _screen(name)
        assert walk.sink is not None and walk.dead_transitions == 0, name
        seen = collections.defaultdict(set)
        sides = collections.defaultdict(set)
        for k in c.cases:
            ok, kind, at = walk.walk(k.line)
            assert kind != "dead"
            if len(k.line):
                seen[kind].add((k.head + at, k.head))
                for b in ce.SCREEN_BORDERS:
                    if abs(k.head + at - b) <= 1:
                        sides[kind, b].add(k.head + at - b)
        assert seen["end"] >= every, (name, sorted(every - seen["end"]))
        assert all(sides["end", b] == {-1, 0, 1} for b in ce.SCREEN_BORDERS), (name, dict(sides))      # one short of, on and one past the border
        absorbed[name] = (seen["absorb"], sides)
    assert absorbed["threads"][0] >= every and set().union(*(a for a, _ in absorbed.values())) >= every
    for name in ("log", "look", "atomic", "threads"):
        assert all(absorbed[name][1]["absorb", b] == {-1, 0, 1} for b in ce.SCREEN_BORDERS), name


# ---- nfa_match_kernel<ATOMIC>: the faithful host walk (tests/helpers/nfa_atomic_interp.py walk), its gates, and the events of the
# atomic families on byte p

ATOMIC_FAMILIES = ("atomic",) + ATOMIC_NEW


def _atomic(name):
    """(corpus, expected rows, interpreter, walks) -- computed once.  walks[case index] = (result, trace, gate faults) of the
    faithful walk at the case's own head.  The head reaches the walk through the doomed-spawn look-ahead alone (walk(): `nxt`), so
    a program without such rows is walked once per line."""
    if ("atomic", name) not in _cache:
        c, o, exp = _oracle(name)
        rx = B.GpuRegex(c.family.pattern, syntax_flags=c.family.flags, engine=B.LC_ENGINE_NFA)
        it = AtomicNfaInterp(rx)
        assert rx.atomic_groups()[0] > 0 and it.atomic
        done, walks = {}, []
        for k in c.cases:
            key = (k.line, k.head if it.quasi_rows is not None else 0)
            if key not in done:
                faults = []
                got, trace = it.walk(k.line, key[1], faults=faults)
                done[key] = (got, trace, faults)
            walks.append(done[key])
        _cache["atomic", name] = (c, exp, it, walks, rx)
    return _cache["atomic", name]


def _at(trace, i):
    """the trace's entry for byte i (None: the walk did not look at it)"""
    return next((t for t in trace if t.i == i), None)


def test_the_helper_quotes_the_kernels_constants():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "loongcollector_amd", "csrc", "nfa_kernel.hpp")).read()
    assert "constexpr int kNfaLineage = %d;" % nai.MAX_LINEAGE in src and "constexpr int kNfaLineageWork = %d;" % nai.LINEAGE_WORK in src
    assert "if (nClosed == %d) return" % nai.MAX_CLOSED in src and "if (nKept == %d) {" % nai.MAX_THREADS in src
    assert "totalWins + nWins > %d" % nai.MAX_THREADS in src and "L >= (1u << 17) - 2" in src and nai.MAX_LENGTH == ce.LENGTH_BOUND == (1 << 17) - 2
    packer = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "loongcollector_amd", "csrc", "regex_handle.cpp")).read()
    assert "if (nfa.atomicCount > %d) throw" % nai.MAX_INSTANCES in packer and "return (e >> 23) & 0xFFu;" in src     # 8 bits of a key
    assert nai.EXITS == ("long", "vector64", "kept64", "closed64", "work10", "lineage6") and set(ce.ATOMIC_EXITS.values()) == set(nai.EXITS) - {"long"}


def test_atomic_walks_give_the_golden_rows_and_the_gates_are_sound(golden_dir):
    """tests/golden/regex_atomic_golden.json: faithful walk == uncapped plain walk == the golden row, for head 0..3; and wherever the
    faithful walk skipped a byte or took the vector step, the plain commit pass on the same thread list leaves the same threads
    (a skipped thread keeps the memberships it holds; the vector step is only taken where nobody holds one)."""
    with open(os.path.join(golden_dir, "regex_atomic_golden.json")) as f:
        d = json.load(f)
    walked = skipped = vector = with_rows = 0
    for kind, flags in (("full", 0), ("search", B.LC_SYNTAX_SEARCH)):
        for c in d[kind]:
            try:
                rx = B.GpuRegex(c["p"].encode("latin-1"), syntax_flags=flags, engine=B.LC_ENGINE_NFA)
            except B.RegexUnsupportedError:
                continue
            if not rx.has_nfa_program() or not rx.atomic_groups()[0]:
                continue
            it = AtomicNfaInterp(rx)
            with_rows += it.quasi_rows is not None
            for subj, flat in c["subs"]:
                s = subj.encode("latin-1")
                exp = flat if kind == "search" or flat is None else flat[2:]
                assert it.fullmatch(s, capped=False) == exp, (c["p"], subj)
                for head in range(4):
                    faults = []
                    got, trace = it.walk(s, head, faults=faults)
                    assert got == exp and not faults and exit_of(trace) is None, (c["p"], subj, head, got, exp, faults[:2])
                    walked += 1
                    skipped += sum(t.what == "skip" for t in trace)
                    vector += sum(t.what == "vector" for t in trace)
    # (the set is not degenerate for this check: thousands of walks, skips and vector steps among them, programs with doomed-spawn rows)
    assert walked > 6000 and skipped > 300 and vector > 2000 and with_rows >= 10, (walked, skipped, vector, with_rows)


@pytest.mark.parametrize("name", ATOMIC_FAMILIES)
def test_atomic_families_walks_give_the_oracles_rows(name):
    """every case of the atomic families: the faithful walk at the case's head gives the oracle's row or leaves through an exit, the
    uncapped plain walk gives the oracle's row on EVERY line (the overflowing ones too), no gate is unsound; the resumed searches of
    `atomic` included"""
    c, exp, it, walks, rx = _atomic(name)
    fam = c.family
    plain = {}
    for i, (k, e, (got, trace, faults)) in enumerate(zip(c.cases, exp, walks)):
        assert not faults, (c.label(i), faults[:2])
        assert got == ("overflow" if exit_of(trace) else e), (c.label(i), got, e)
        if k.line not in plain:
            plain[k.line] = it.fullmatch(k.line, capped=False)
        assert plain[k.line] == e, c.label(i)
        if k.kind == "resume":
            want = _flat(fam, OracleRegex(fam.pattern).search(k.line, k.frm))
            faults = []
            assert it.walk(k.line, k.head, start=k.frm, faults=faults)[0] == want and not faults, c.label(i)
            assert it.fullmatch(k.line, start=k.frm, capped=False) == want, c.label(i)
    over = [bool(exit_of(w[1])) for w in walks]
    assert any(over) == (name in ce.ATOMIC_EXITS), name
    assert (it.quasi_rows is not None) == (name == "aquasi")


def test_alog_keeps_three_groups_and_commits_on_every_byte_of_its_fields():
    c, exp, it, walks, rx = _atomic("alog")
    log = _oracle("log")
    assert [k.line for k in c.cases] == [k.line for k in log[0].cases] and exp == log[2]               # the log family's lines and rows
    assert rx.atomic_groups() == (3, 0) and (it.npos, it.nslots) == (7, 8)
    borders = collections.Counter()
    for k, e, (got, trace, _) in zip(c.cases, exp, walks):
        last = k.line.find(b" ", k.line.find(b";") + 1) if b";" in k.line and b"," in k.line[:k.line.find(b";")] else -1
        for t in trace:
            if t.what in ("end", "end_plain"):
                continue
            if e is not None:                                                                        # a matching line: fields 1 to 3 in front of `last`
                assert (t.what == "commit") == (t.i <= last), (k.variant, k.p, t)
                assert t.i >= last or t.lineage >= 1 or k.line[t.i:t.i + 1] in (b",", b";"), (k.variant, k.p, t)
            for b in (256, 512):
                if t.what == "commit" and t.lineage >= 1 and k.head + t.i + 1 == b and _at(trace, t.i + 1) is not None and _at(trace, t.i + 1).what == "commit":
                    borders[b, k.head] += 1                                                          # a membership carried over the reload
    assert all(borders[b, h] >= 20 for b in (256, 512) for h in range(4)), borders


def test_acommit_and_aquasi_put_their_events_on_byte_p():
    c, exp, it, walks, rx = _atomic("acommit")
    assert rx.atomic_groups() == (2, 0)
    for k, (got, trace, _) in zip(c.cases, walks):
        what = (k.kind, k.variant, k.p, k.head)
        t = _at(trace, k.p)
        if k.kind == "commit" and k.variant.startswith("ends"):
            assert t.what == "end" and t.closed == 1 and _at(trace, k.p - 1).lineage == 1, what        # the commit at the end of input
        elif k.kind in ("commit", "alt") and k.variant != "ends":
            assert t.what == "commit" and t.closed == 1 and t.lineage == 0 and _at(trace, k.p - 1).lineage == 1, what   # left on byte p
            if k.kind == "commit":
                n = int(k.variant.rsplit("_", 1)[1])
                assert all(_at(trace, i).what == "commit" and _at(trace, i).lineage == 1 for i in range(k.p - n, k.p)), what
        elif k.kind == "alt":
            assert t.what == "end" and t.closed == 1, what
        else:                                                                                         # enter: nothing in front of p is a commit pass
            assert t.what == "commit" and t.lineage == 1 and [x.what for x in trace if x.i < k.p and x.what == "commit"] == [], what
            back = int(k.variant.split("_")[1]) if "_" in k.variant else k.p - 1
            # (field 2 begins at p - back: its first byte enters it, the others are steady, the semicolon at p - 1 is a vector step)
            assert all(_at(trace, i).what == "skip" for i in range(k.p - back + 1, k.p - 1)) and _at(trace, k.p - 1).what == "vector", what
    c, exp, it, walks, rx = _atomic("aquasi")
    assert rx.atomic_groups() == (1, 0) and it.quasi_rows
    blind = collections.Counter()
    for k, (got, trace, _) in zip(c.cases, walks):
        what = (k.variant, k.p, k.head)
        t = _at(trace, k.p)
        unknown = (k.head + k.p + 1) % 256 == 0 or k.p + 1 == len(k.line)                              # byte p + 1: next chunk, or none
        if k.variant in ("doomed", "doomed_far", "doomed_alone") and k.p >= 1:
            assert (t.what, t.quasi) == (("vector", False) if unknown else ("skip", True)), what       # skipped exactly where the row can be read
            blind[k.variant, (k.head + k.p) % 256 == 255] += 1
            assert all(x.what == "skip" and not x.quasi for x in trace if 1 <= x.i < k.p), what
        else:
            # a spawn that lives, or the last byte; or p == 0: the first byte is stepped from the start pseudo-position, which has
            # neither a steady bit nor a doomed-spawn row -- the lazy field's own position is only reached behind it
            assert t.what == "vector" and (k.p >= 1 or (it.stable[it.npos] == 0 and not int(it.quasi_idx[it.npos]))), what
        first = (k.head + k.p) % 256 == 0
        blind["first", first] += 1
    assert all(blind[v, True] == 8 and blind[v, False] > 100 for v in ("doomed", "doomed_far", "doomed_alone")) and blind["first", True] >= 40, blind


@pytest.mark.parametrize("name", sorted(ce.ATOMIC_EXITS) + sorted(ce.SIBLING.values()))
def test_each_exit_is_taken_on_byte_p(name):
    """the overflow variants leave through the family's exit ON byte p (a walk stops at its first exit: none is earlier), for every
    head; the controls leave through none and sit exactly at the cap by the step on byte p: 64 survivors appended, 64 winners of
    the vector step, 6 memberships, 64 closed segments, 10 work entries"""
    c, exp, it, walks, rx = _atomic(name)
    fam = c.family
    seen = collections.Counter()
    for k, (got, trace, _) in zip(c.cases, walks):
        what = (name, k.variant, k.p, k.head)
        t = _at(trace, k.p)
        if fam.overflows(k):
            assert got == "overflow" and exit_of(trace) == (ce.ATOMIC_EXITS[name], k.p) and t is trace[-1], (what, exit_of(trace))
            assert t.what == ("vector" if name == "avector64" else "commit"), what
        else:
            control = name if name in ce.AT_CAP else None
            assert exit_of(trace) is None and control, what
            field, cap = ce.AT_CAP[name]
            assert getattr(t, field) == cap and t.what == ("vector" if name == "avector64" else "commit"), (what, t)
            assert max(getattr(x, field) for x in trace) == cap, what                                 # ... and nowhere beyond it
        seen[fam.overflows(k), k.head] += 1
    assert all(n >= 2 * 30 for n in seen.values()) and {h for _, h in seen} == set(range(4))      # (two variants or more at 30 offsets or more, per head)
    assert {o for o, _ in seen} == ({True} if name in ce.SIBLING else {False} if name in ce.SIBLING.values() else {True, False})
    shape = {"akept64": (1, 74), "avector64": (1, 74), "alineage6": (7, 4), "alineage6c": (6, 4), "aclosed64": (66, 26), "aclosed64c": (64, 20),
             "awork10": (11, 11), "awork10c": (10, 10)}[name]
    assert (it.ninstances, it.npos) == shape and rx.atomic_groups() == (shape[0], 0)


def _mutable(it):
    """the interpreter's own copies of the steady tables, as lists the test may change"""
    it.quasi_idx = list(it.quasi_idx) if it.quasi_idx is not None else [0] * (it.npos + 1)
    it.quasi_rows = [list(r) for r in it.quasi_rows or []]
    return it


def test_the_faithful_walk_reads_the_doomed_spawn_rows_and_the_touchy_bits():
    """Mutations of the interpreter's own copy of the tables.  (?>a+?.): the row round 6's bug had -- the loop position, class of
    'a', next class of '1' -- makes the faithful walk match "aa1", which is wrong; unmutated it does not.  A cleared touchy bit on
    (?>(ab|a))(bc|d): the vector step enters the group without a membership, the first branch's exit closes nothing, the second
    branch lives and "abc" matches, which is wrong."""
    rx = B.GpuRegex(b"(?>a+?.)", engine=B.LC_ENGINE_NFA)
    it = _mutable(AtomicNfaInterp(rx))
    assert not it.quasi_rows and OracleRegex(b"(?>a+?.)").fullmatch(b"aa1") is None
    assert it.walk(b"aa1")[0] is None and not it.gate_faults(b"aa1")
    loop = [p for p in range(it.npos) if any(t == p for t, _, _ in it.follow[p])]
    assert len(loop) == 1
    ca, c1 = int(it.cmap[ord("a")]), int(it.cmap[ord("1")])
    it.quasi_rows.append([(1 << c1) if c == ca else 0 for c in range(it.ncls)])
    it.quasi_idx[loop[0]] = len(it.quasi_rows)
    got, trace = it.walk(b"aa1")
    assert got is not None and [t.what for t in trace if t.quasi] == ["skip"]                          # the row was read, and believed
    assert it.gate_faults(b"aa1")                                                                     # ... and the gate check sees it

    pat = b"(?>(ab|a))(bc|d)"
    it = AtomicNfaInterp(B.GpuRegex(pat, engine=B.LC_ENGINE_NFA))
    assert OracleRegex(pat).fullmatch(b"abc") is None and it.walk(b"abc")[0] is None
    tr = it.walk(b"abd")[1]
    assert [t.what for t in tr] == ["commit", "commit", "commit", "end_plain"]
    # the bit that sends the FIRST byte to the commit pass (nobody holds a membership yet: the gate decides alone), cleared
    ca = int(it.cmap[ord("a")])
    assert (it.touchy[it.npos] >> ca) & 1
    it.touchy[it.npos] &= ~(1 << ca)
    got, tr = it.walk(b"abc")
    assert got is not None and tr[0].what == "vector" and it.gate_faults(b"abc")                     # the bit was read, and believed


def test_255_atomic_instances_compile_and_the_last_one_commits():
    with pytest.raises(B.RegexUnsupportedError, match="more than 255 atomic group instances"):
        B.GpuRegex(ce.instance_pattern(256), engine=B.LC_ENGINE_NFA)
    rx = B.GpuRegex(ce.instance_pattern(255), engine=B.LC_ENGINE_NFA)
    it = AtomicNfaInterp(rx)
    assert rx.atomic_groups() == (255, 0) and it.ninstances == nai.MAX_INSTANCES == 255
    codes = {code for p in range(it.npos + 1) for path in it.events[p] for code, _ in path if code < nai.ASSERT_EVENT}
    assert max(codes) == 255 and min(codes) == -255                                                   # instance 254: the top of the key's 8 bits
    o, plain = OracleRegex(ce.instance_pattern(255)), OracleRegex(ce.instance_pattern(255, plain=True))
    for line, what in ce.instance_lines():
        e = o.fullmatch(line)
        e = None if e is None else [v for be in e[1:] for v in be]
        assert it.fullmatch(line, capped=False) == e, what
        for head in range(4):
            got, trace = it.walk(line, head)
            assert got == e and exit_of(trace) is None and not it.gate_faults(line, head), (what, head)
        if what == "commits":                                                                         # only the commit of instance 254 refuses it
            assert e is None and plain.fullmatch(line) is not None
            last = [t for t in trace if t.what == "commit" and t.closed][-2:]
            assert [t.i for t in last] == [len(line) - 2, len(line) - 1]
        if what == "first":
            assert e is not None and all(t.what == "commit" for t in trace[:-1]) and len(trace) == len(line) + 1


def test_the_length_bound_is_two_short_of_two_to_the_17th():
    rx = B.GpuRegex(ce.LENGTH_FAMILY.pattern, engine=B.LC_ENGINE_NFA)
    it = AtomicNfaInterp(rx)
    o = OracleRegex(ce.LENGTH_FAMILY.pattern)
    assert rx.atomic_groups() == (1, 0) and it.npos <= 5
    lines = ce.length_lines()
    assert len({len(x) % 4 for x in lines}) >= 3
    for k, line in enumerate(lines):
        got, trace = it.walk(line, k % 4)
        e = o.fullmatch(line)
        if len(line) >= ce.LENGTH_BOUND:
            assert got == "overflow" and exit_of(trace) == ("long", 0) and e is not None
        else:
            assert exit_of(trace) is None and got == (None if e is None else [v for be in e[1:] for v in be]), k
    assert sum(len(x) >= ce.LENGTH_BOUND for x in lines) == 2 and max(len(x) for x in lines if len(x) < ce.LENGTH_BOUND) == ce.LENGTH_BOUND - 1
