"""The chunk-edge corpus of tests/helpers/chunk_edges.py, without a GPU: that every case does what its label says (conditions on the
INPUTS of tests/test_gpu_chunk_edges.py, so that test cannot pass on a degenerate corpus), that every (offset, residue) pair is there
for every kind, that the instantiation table runs what the families declare, and that the product's own compiled tables -- walked by
the host interpreters (tests/helpers/table_interp.py, tests/helpers/nfa_atomic_interp.py, the backtracking program's host walk of
tests/native/bt_host_check.cpp) -- give the oracle's answer on every line.  A mismatch on the GPU is then a kernel's, not the tables'.
For run_stop the tables' own quiet / steady masks say that the run bytes are quiet and byte p is not: the kernels' run scans are on
the path."""
import collections

import numpy as np
import pytest

from loongcollector_amd import binding as B
from oracle.oracle import OracleRegex
from tests.helpers import chunk_edges as ce
from tests.helpers.nfa_atomic_interp import AtomicNfaInterp
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
    if name.startswith("over"):
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
    assert len({r.id for r in ce.ROWS}) == len(ce.ROWS) == 23
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
    assert set(ce.CHAIN) == {("chain64", "over64"), ("chain128", "over128"), ("chain-slots", "over64s"), ("nfa-wide-first", "over64"),
                             ("nfa-wide-first", "over128")} and set(ce.DECIDES) == {k for k, (has, _) in ce.CHAIN.items() if "nfa_decide_kernel" in has}
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


# (... and the overflow families': test_the_overflow_families_exceed_each_cap_by_the_step_on_byte_p, with the caps the kernels have)
@pytest.mark.parametrize("name", sorted({f for r in ce.ROWS if r.compile_engine == B.LC_ENGINE_NFA for f in r.families} - {"lazy"} - set(OVER)))
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
