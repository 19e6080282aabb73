#!/usr/bin/env python3
"""Differential fuzz of the NFA tables (packNfaBlob: steady masks, doomed-spawn rows, suffix flag) and of the atomic-elision pass: fresh
random patterns, plain and atomic / possessive, full match and search, walked by tests/helpers NfaInterp (plain programs) and by
AtomicNfaInterp.walk (atomic programs, bare and -- every other one -- behind a lazy or negated lead field and a literal: nfa_match_kernel<ATOMIC>'s byte loop restated -- steady skip, doomed-spawn rows, touchy gate, vector
step, suffix exit, every overflow exit) against the oracle; wherever that walk skips a byte or takes the vector step the full commit
pass must agree (gate_faults).  A value the faithful walk gives up ("overflow") is not dropped: the uncapped plain walk must give the
oracle's row.  Only what the oracle itself refuses (RuntimeError) is left out.
    python tools/fuzz_nfa.py FIRST_SEED LAST_SEED     (250 seeds: ~60 000 pattern x modes)"""
import os, sys, random, importlib.util, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from loongcollector_amd import binding as B
from oracle.oracle import OracleRegex
from tests.helpers.table_interp import NfaInterp
from tests.helpers.nfa_atomic_interp import AtomicNfaInterp
spec = importlib.util.spec_from_file_location("g", os.path.join(ROOT, "tests", "golden", "gen_regex_golden.py")); gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
aspec = importlib.util.spec_from_file_location("a", os.path.join(ROOT, "tests", "golden", "gen_atomic_golden.py")); agen = importlib.util.module_from_spec(aspec); aspec.loader.exec_module(agen)
t0=time.time(); checked=pats=quasi=aquasi=elided=overflows=abare=aled=0
for seed in range(int(sys.argv[1]), int(sys.argv[2])):
    rng = random.Random(9000 + seed); g = gen.Gen(rng)
    for k in range(120):
        lead = None
        if k % 3 == 2:
            p, smp = agen.gen(rng), None
            if k % 6 == 5:     # every other one behind a lazy or negated field and a literal: the shape whose programs carry doomed-spawn rows
                lead = rng.choice([(b"(.*?) SA ", b" SA "), (b"([^ ]*) ", b" "), (b"(.*?), ", b", "), (b"(.*?) S", b" S")])
                p = lead[0].decode() + p if isinstance(p, str) else lead[0] + p
        else: p, _, smp = g.alt(0)
        try: orx = OracleRegex(p)
        except ValueError: continue
        for flags, fn in ((0, orx.fullmatch), (B.LC_SYNTAX_SEARCH, orx.search)):
            try: rx = B.GpuRegex(p, syntax_flags=flags, engine=B.LC_ENGINE_NFA)
            except (B.RegexUnsupportedError, B.RegexSyntaxError): continue
            if not rx.has_nfa_program(): continue
            kept, el = rx.atomic_groups(); elided += el
            it = AtomicNfaInterp(rx) if kept else NfaInterp(rx)
            if not kept: quasi += it.quasi_rows is not None
            else: aquasi += it.quasi_rows is not None; abare += lead is None; aled += lead is not None
            pats += 1
            subs = [gen.rand_subject(rng) for _ in range(4)] + [bytes(rng.choice(b"abc1 ") for _ in range(rng.randint(0, 12))) for _ in range(4)]
            if smp is not None: subs += [gen.mutate(rng, smp()) for _ in range(4)]
            if lead is not None: subs += [bytes(rng.choice(b"xy S,") for _ in range(rng.randint(0, 6))) + lead[1] + bytes(rng.choice(b"abc1 ") for _ in range(rng.randint(0, 8))) for _ in range(6)]
            for s in subs:
                try:
                    e = fn(s)
                except RuntimeError:
                    continue
                want = None if e is None else ([v for ab in e for v in ab] if flags else [v for ab in e[1:] for v in ab])
                if kept:
                    head = (len(s) + k) % 4
                    faults = []
                    got, trace = it.walk(s, head, faults=faults)
                    assert not faults, (p, s, flags, head, faults[:2])
                    if got == "overflow":      # the kernel would send it on: the commit pass without caps decides it
                        overflows += 1
                        got = it.fullmatch(s, capped=False)
                else:
                    got = it.fullmatch(s)
                    if got == "overflow": got = it.fullmatch(s, max_threads=1 << 30)      # (more than 64 threads: nfa_wide_kernel's, or the decide kernel's)
                checked += 1
                assert got == want, (p, s, flags, type(it).__name__, got, want)
print("ok: %d patterns x modes (%d with quasi rows, %d groups elided), %d checks, %d atomic programs bare and %d behind a lead field, %d atomic programs with quasi rows, %d overflows decided by the uncapped walk, %.0f s" % (
    pats, quasi, elided, checked, abare, aled, aquasi, overflows, time.time()-t0))
