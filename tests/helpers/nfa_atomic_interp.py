"""Test-only replay of the NFA program for patterns with atomic groups / possessive quantifiers, written out in Python so that the
packed tables and the commit rules can be checked without a GPU.  Not part of the product.  Two walks:

PLAIN (`fullmatch`): the commit pass on every byte, no shortcut.  Threads carry their unsettled atomic-segment memberships ("lineage":
[g, seg, exited]); a step
  1. walks ALL epsilon paths of all threads in priority order, viable or not (tdfa.cpp commitAtomic has the rules:
     leaving a group closes its segment for everything of lower priority except continuations of the very same exit),
  2. drops memberships nobody can act on any more,
  3. drops a thread that mirrors a higher-priority one on the same position (same rule as the TDFA builder's
     pairwise `mirrors`; with empty lineages this is the ordinary "first thread on a position wins").
With capped=False it has no bound on threads or memberships: the reference the kernel's shortcuts are judged against.

FAITHFUL (`walk`): nfa_match_kernel<ATOMIC>'s byte loop and end of input restated in the kernel's order (nfa_kernel.hpp) -- the suffix
exit, the steady test (NF_OFF_STABLE, or the NF_OFF_QUASI row on (class, next class), the next class unknown across a 256-byte border of
the word-aligned view and behind the last byte), the touchy gate (NF_OFF_TOUCHY) between the ordered commit pass (nfaAtomicStep) and
the vector step, the suffix cut, NF_OFF_ATOMICPOS at the end of input -- with every overflow exit named.  It returns a trace: one Step
per byte looked at.  gate_faults() runs the plain commit wherever the faithful walk skipped a byte or took the vector step.
"""
from collections import namedtuple

import numpy as np

from loongcollector_amd import binding as B
from tests.helpers.table_interp import NfaInterp, _with_run_captures

ASSERT_EVENT = 20000
MAX_LINEAGE = 6      # nfa_kernel.hpp kNfaLineage: memberships a thread carries between steps
LINEAGE_WORK = 10    # nfa_kernel.hpp kNfaLineageWork: ... while a step is being worked out
MAX_THREADS = 64     # lanes of a wavefront: survivors of a step (nKept == 64), winners of a vector step
MAX_CLOSED = 64      # closedKey / closedBy: segments a step can close (nClosed == 64)
MAX_LENGTH = (1 << 17) - 2   # L >= this: segment ids are (offset << 6 | thread) in 23 bits
MAX_INSTANCES = 255  # a lineage key has 8 bits for the group instance
CHUNK = 256          # bytes of the word-aligned view a wavefront holds
EXITS = ("long", "vector64", "kept64", "closed64", "work10", "lineage6")

# one byte looked at.  what: "skip" (every live thread steady; quasi: some only by its doomed-spawn row), "vector", "commit", "suffix"
# (the lone suffix thread: the walk stops in front of byte i), "end" (the ordered commit at the end of input), "end_plain" (the first
# MATCH path), "long".  live: threads in front of the byte; kept: survivors appended by the commit pass (winners of a vector step);
# left: threads behind it; lineage: the largest lineage left; closed: segments the step closed; work: the largest work list;
# exit: None, or the name of the overflow exit taken on this byte.
Step = namedtuple("Step", "i what live kept left lineage closed work exit quasi", defaults=(None, False))


def exit_of(trace):
    """(name, offset) of the exit a walk left through, or None"""
    return (trace[-1].exit, trace[-1].i) if trace and trace[-1].exit else None


class AtomicNfaInterp(NfaInterp):
    def __init__(self, rx):
        super().__init__(rx)
        blob = rx.table(B.LC_TABLE_NFA_BLOB, np.uint32)
        self.atomic = int(blob[14]) != 0
        self.ninstances = int(blob[14])                                                            # NF_ATOMIC
        self.events = []          # per position: per path: [(code, visit), ...]
        if not self.atomic:
            return
        npaths = int(blob[9])
        pe = blob[int(blob[7]) // 4:int(blob[7]) // 4 + 2 * npaths].reshape(-1, 2)[:, 1]   # path word y: events
        ev = blob[int(blob[15]) // 4:]
        fs = blob[int(blob[6]) // 4:int(blob[6]) // 4 + self.npos + 2]
        for p in range(self.npos + 1):
            lst = []
            for i in range(int(fs[p]), int(fs[p + 1])):
                start, cnt = int(pe[i]) >> 8, int(pe[i]) & 0xFF
                one = []
                for w in ev[start:start + cnt]:
                    code = int(w) & 0xFFFF
                    one.append((code - 65536 if code >= 32768 else code, int(w) >> 16))
                lst.append(one)
            self.events.append(lst)
        mw = int(blob[20])
        tm = blob[int(blob[19]) // 4:int(blob[19]) // 4 + mw * (self.npos + 1)]                    # NF_OFF_TOUCHY
        self.touchy = [sum(int(tm[mw * p + k]) << (32 * k) for k in range(mw)) for p in range(self.npos + 1)]
        ap = blob[int(blob[16]) // 4:int(blob[16]) // 4 + (self.npos + 1) // 32 + 1]               # NF_OFF_ATOMICPOS
        self.atomicpos = [bool((int(ap[p >> 5]) >> (p & 31)) & 1) for p in range(self.npos + 1)]

    # ---- one priority-ordered commit pass; cands: (target, src, tags, lin, events, target_ok)
    @staticmethod
    def _commit(cands, holds, step):
        kept, closed = [], {}

        for target, src, tags, lin0, ev, target_ok in cands:
            def exit_visit_for(g, frm):
                depth = 0
                for code, visit in ev[frm:]:
                    if code >= ASSERT_EVENT:
                        if not (holds >> (code - ASSERT_EVENT)) & 1:
                            return 0
                    elif code == g + 1:
                        depth += 1
                    elif code == -(g + 1):
                        if depth == 0:
                            return visit
                        depth -= 1
                return 0

            dead = False
            for g, seg, ex in lin0:
                cl = closed.get((g, seg))
                if cl is not None and (ex or cl[0] != src or exit_visit_for(g, 0) != cl[1]):
                    dead = True
            if dead:
                continue
            lin = [list(e) for e in lin0]
            ok = True
            for i, (code, visit) in enumerate(ev):
                if code >= ASSERT_EVENT:
                    if not (holds >> (code - ASSERT_EVENT)) & 1:
                        ok = False
                        break
                elif code > 0:
                    g = code - 1
                    seg = (step + 1, src)                # one fresh segment per (step, source thread, group)
                    cl = closed.get((g, seg))
                    if cl is not None and (cl[0] != src or exit_visit_for(g, i + 1) != cl[1]):
                        dead = True
                        break
                    lin.append([g, seg, False])
                else:
                    g = -code - 1
                    for e in reversed(lin):
                        if e[0] == g and not e[2]:
                            e[2] = True
                            closed.setdefault((g, e[1]), (src, visit))
                            break
            if dead or not ok or not target_ok:
                continue
            kept.append([target, src, tags, lin])
        # memberships nobody can act on any more
        for i, k in enumerate(kept):
            k[3] = [e for e in k[3] if not e[2] or any(
                f[0] == e[0] and f[1] == e[1] and not f[2] for j in range(i) for f in kept[j][3])]

        def holds_(c, e, inside_only):
            return any(x[0] == e[0] and x[1] == e[1] and (not inside_only or not x[2]) for x in c[3])

        def mirrors(hi, lo):
            if kept[hi][0] != kept[lo][0]:
                return False
            for e in kept[hi][3]:
                if not holds_(kept[lo], e, False) and any(holds_(kept[k], e, True) for k in range(hi)):
                    return False
            for e in kept[lo][3]:
                if not e[2] and not holds_(kept[hi], e, True) and any(holds_(kept[k], e, False)
                                                                       for k in range(lo + 1, len(kept))):
                    return False
            return True

        changed = True
        while changed:
            changed = False
            for i in range(1, len(kept)):
                if any(mirrors(j, i) for j in range(i)):
                    del kept[i]
                    changed = True
                    break
        return kept

    def _stamp(self, caps, tags, at):
        caps = list(caps)
        for sl in self._slots(tags):
            caps[sl] = at
        return caps

    def plain_step(self, threads, cls, holds, pos):
        """the commit pass on one byte, no cap: threads (position, caps, lineage) -> the threads it leaves"""
        cands = []
        for t, (p, _, lin) in enumerate(threads):
            for k, (tgt, cond, tags) in enumerate(self.follow[p]):
                ok = tgt >= 0 and (self.posmask[tgt] >> cls) & 1
                cands.append((tgt, t, tags, lin, self.events[p][k], bool(ok)))
        return [(tgt, self._stamp(threads[src][1], tags, pos), lin) for tgt, src, tags, lin in self._commit(cands, holds, pos)]

    def plain_end(self, threads, holds, L):
        """the ordered commit at the end of input: the winner's row, or None"""
        cands = []
        for t, (p, _, lin) in enumerate(threads):
            for k, (tgt, cond, tags) in enumerate(self.follow[p]):
                cands.append((-1 - len(cands), t, tags, lin, self.events[p][k], tgt < 0))   # unique "positions"
        kept = self._commit(cands, holds, L)
        if not kept:
            return None
        _, src, tags, _ = kept[0]
        return self._stamp(threads[src][1], tags, L)

    @_with_run_captures
    def fullmatch(self, s, max_threads=MAX_THREADS, start=0, capped=True):
        """the PLAIN walk.  capped: give up ("overflow") beyond max_threads threads or MAX_LINEAGE memberships behind a step"""
        if not self.atomic:
            return super().fullmatch(s, max_threads=max_threads if capped else 1 << 30, start=start)
        threads = [(self.npos, [-1] * self.nslots, [])]      # (position, caps, lineage)
        prev_cls = self.ncls
        if start:
            threads = [(0, [-1] * self.nslots, [])]
            prev_cls = int(self.cmap[s[start - 1]])
        for pos in range(start, len(s)):
            cls = int(self.cmap[s[pos]])
            holds = self.behind[prev_cls] | self.ahead[cls]
            prev_cls = cls
            threads = self.plain_step(threads, cls, holds, pos)
            if capped and (len(threads) > max_threads or any(len(t[2]) > MAX_LINEAGE for t in threads)):
                return "overflow"
            if not threads:
                return None
        return self.plain_end(threads, self.behind[prev_cls] | self.ahead[self.ncls], len(s))

    # ---- the FAITHFUL walk

    def _quiet(self, p, cls, nxt):
        """nfa_kernel.hpp nfaQuiet -> (steady, by the doomed-spawn row alone)"""
        if (self.stable[p] >> cls) & 1:
            return True, False
        if nxt is None or self.quasi_idx is None or not int(self.quasi_idx[p]):
            return False, False
        return bool((self.quasi_rows[int(self.quasi_idx[p]) - 1][cls] >> nxt) & 1), True

    def _kernel_step(self, threads, cls, holds, step, final):
        """nfaAtomicStep in its own order -> (survivors [target, src, tags, lineage] or the name of an exit, stats)"""
        closed, kept, best = {}, [], set()
        st = {"closed": 0, "work": 0, "kept": 0}

        def exit_visit_for(ev, g, frm):
            depth = 0
            for code, visit in ev[frm:]:
                if code >= ASSERT_EVENT:
                    if not (holds >> (code - ASSERT_EVENT)) & 1:
                        return 0
                elif code == g + 1:
                    depth += 1
                elif code == -(g + 1):
                    if depth == 0:
                        return visit
                    depth -= 1
            return 0

        for t, (p, _, lin0) in enumerate(threads):
            for k, (tgt, cond, tags) in enumerate(self.follow[p]):
                ev = self.events[p][k]
                target_ok = tgt < 0 if final else (tgt >= 0 and bool((self.posmask[tgt] >> cls) & 1))
                dead = False
                for g, seg, ex in lin0:
                    cl = closed.get((g, seg))
                    if cl is not None and (ex or cl[0] != t or exit_visit_for(ev, g, 0) != cl[1]):
                        dead = True
                        break
                if dead:
                    continue
                work = [list(e) for e in lin0]
                st["work"] = max(st["work"], len(work))
                ok = True
                for i, (code, visit) in enumerate(ev):
                    if code >= ASSERT_EVENT:
                        if not (holds >> (code - ASSERT_EVENT)) & 1:
                            ok = False
                            break
                    elif code > 0:
                        g = code - 1
                        seg = (((step + 1) << 6) | t) & 0x7FFFFF
                        cl = closed.get((g, seg))
                        if cl is not None and (cl[0] != t or exit_visit_for(ev, g, i + 1) != cl[1]):
                            dead = True
                            break
                        if len(work) == LINEAGE_WORK:
                            return "work10", st
                        work.append([g, seg, False])
                        st["work"] = max(st["work"], len(work))
                    else:
                        g = -code - 1
                        for e in reversed(work):
                            if e[0] == g and not e[2]:
                                if (g, e[1]) not in closed:
                                    if len(closed) == MAX_CLOSED:
                                        return "closed64", st
                                    closed[(g, e[1])] = (t, visit)
                                    st["closed"] = len(closed)
                                e[2] = True
                                break
                if dead or not ok or not target_ok:
                    continue
                if not final and not work:           # among survivors without memberships the first on a position wins, right here
                    if tgt in best:
                        continue
                    best.add(tgt)
                if len(kept) == MAX_THREADS:
                    return "kept64", st
                kept.append([("final", len(kept)) if final else tgt, t, tags, work])
                st["kept"] = len(kept)
        for i, k in enumerate(kept):                 # memberships nobody can act on any more
            k[3] = [e for e in k[3] if not e[2] or any(
                f[0] == e[0] and f[1] == e[1] and not f[2] for j in range(i) for f in kept[j][3])]

        def holds_(c, e, inside_only):
            return any(x[0] == e[0] and x[1] == e[1] and (not inside_only or not x[2]) for x in c[3])

        def mirrors(hi, lo):
            for e in kept[hi][3]:
                if not holds_(kept[lo], e, False) and any(holds_(kept[k], e, True) for k in range(hi)):
                    return False
            for e in kept[lo][3]:
                if not e[2] and not holds_(kept[hi], e, True) and any(holds_(kept[k], e, False) for k in range(lo + 1, len(kept))):
                    return False
            return True

        if not final:
            dropped = object()
            changed = True
            while changed:
                changed = False
                for i in range(1, len(kept)):
                    if kept[i][0] is dropped:
                        continue
                    for j in range(i):
                        if kept[j][0] is dropped or kept[j][0] != kept[i][0] or (not kept[i][3] and not kept[j][3]):
                            continue
                        if mirrors(j, i):
                            kept[i][0], kept[i][3] = dropped, []      # parked: it holds nothing
                            changed = True
                            break
            kept = [k for k in kept if k[0] is not dropped]
        if any(len(k[3]) > MAX_LINEAGE for k in kept):
            return "lineage6", st
        return kept, st

    def _vector_step(self, threads, cls, holds, pos):
        """the vector step: per target the candidate of highest priority -> the new threads (uncut: the caller counts them)"""
        new, seen = [], set()
        for p, caps, _ in threads:
            for tgt, cond, tags in self.follow[p]:
                if tgt < 0 or (cond & ~holds) or tgt in seen or not (self.posmask[tgt] >> cls) & 1:
                    continue
                seen.add(tgt)
                new.append((tgt, self._stamp(caps, tags, pos), []))
        return new

    def _norm(self, ts, segments=False):
        """a thread list as the gate checks compare it: cut behind a suffix thread that holds no membership (nothing below it can
        win), and without the captures of a suffix thread that is not the first -- a steady position of a search pattern may re-spawn
        the wrapper's suffix thread (device_tables.h NF_OFF_STABLE), whose captures nobody reads while the thread above it lives"""
        out = []
        for p, c, l in ts:
            suf = p == self.search_suffix
            out.append((p, None if suf and out else c, [(e[0], e[1] if segments else None, e[2]) for e in l]))
            if suf and not l:
                break
        return out

    def _same(self, a, b):
        return self._norm(a) == self._norm(b) and not any(l for _, _, l in b)

    def walk(self, s, head=0, start=0, faults=None):
        """the FAITHFUL walk -> (row | None | "overflow", trace).  head: the residue mod 4 of the value's first byte in device memory
        (the chunk borders of the word-aligned view fall at line offsets 256k - head).  faults: a list that gets (offset, what, why)
        wherever the plain commit pass on the same thread list disagrees with a skip or a vector step (gate_faults)."""
        assert self.atomic and 0 <= head < 4
        L, trace = len(s), []
        if L >= MAX_LENGTH:
            return "overflow", [Step(0, "long", 1, 0, 0, 0, 0, 0, "long")]
        threads = [(self.npos, [-1] * self.nslots, [])]
        prev = self.ncls
        if start:
            start = min(start, L)
        if start:
            threads = [(0, [-1] * self.nslots, [])]
            prev = int(self.cmap[s[start - 1]])
        suffix = self.search_suffix
        i = start
        while i < L and threads:
            if suffix >= 0 and len(threads) == 1 and threads[0][0] == suffix and not threads[0][2]:
                trace.append(Step(i, "suffix", 1, 0, 1, 0, 0, 0))
                break
            idx = head + i
            cls = int(self.cmap[s[i]])
            nxt = int(self.cmap[s[i + 1]]) if i + 1 < L and (idx + 1) // CHUNK == idx // CHUNK else None
            quiet = [self._quiet(p, cls, nxt) for p, _, _ in threads]
            live = len(threads)
            lineage = max(len(t[2]) for t in threads)
            if all(q for q, _ in quiet):
                by_row = any(r for _, r in quiet)
                trace.append(Step(i, "skip", live, 0, live, lineage, 0, 0, None, by_row))
                if faults is not None:
                    self._audit_skip(s, i, threads, prev, cls, by_row, faults)
                prev = cls
                i += 1
                continue
            holds = self.behind[prev] | self.ahead[cls]
            prev = cls
            if any(t[2] or (self.touchy[t[0]] >> cls) & 1 for t in threads):
                kept, st = self._kernel_step(threads, cls, holds, i, False)
                if isinstance(kept, str):
                    trace.append(Step(i, "commit", live, st["kept"], 0, 0, st["closed"], st["work"], kept))
                    return "overflow", trace
                new = [(tgt, self._stamp(threads[src][1], tags, i), [tuple(e) for e in lin]) for tgt, src, tags, lin in kept]
                for k, t in enumerate(new):          # the suffix cut: only behind a suffix thread that holds no membership
                    if suffix >= 0 and t[0] == suffix and not t[2]:
                        new = new[:k + 1]
                        break
                trace.append(Step(i, "commit", live, st["kept"], len(new), max([len(t[2]) for t in new] or [0]), st["closed"], st["work"]))
            else:
                new = self._vector_step(threads, cls, holds, i)
                if faults is not None and not self._same(new, self.plain_step(threads, cls, holds, i)):
                    faults.append((i, "vector", "the commit pass leaves other threads"))
                if len(new) > MAX_THREADS:
                    trace.append(Step(i, "vector", live, len(new), 0, 0, 0, 0, "vector64"))
                    return "overflow", trace
                n = len(new)
                for k, t in enumerate(new):
                    if suffix >= 0 and t[0] == suffix:
                        new = new[:k + 1]
                        break
                trace.append(Step(i, "vector", live, n, len(new), 0, 0, 0))
            threads = new
            i += 1
        if not threads:
            return None, trace
        holds = self.behind[prev] | self.ahead[self.ncls]
        if any(t[2] or self.atomicpos[t[0]] for t in threads):
            kept, st = self._kernel_step(threads, 0, holds, L, True)
            if isinstance(kept, str):
                trace.append(Step(L, "end", len(threads), st["kept"], 0, 0, st["closed"], st["work"], kept))
                return "overflow", trace
            trace.append(Step(L, "end", len(threads), st["kept"], len(kept), 0, st["closed"], st["work"]))
            if not kept:
                return None, trace
            _, src, tags, _ = kept[0]
            return self._finish(s, self._stamp(threads[src][1], tags, L)), trace
        trace.append(Step(L, "end_plain", len(threads), 0, 0, 0, 0, 0))
        if faults is not None:
            want = self.plain_end(threads, holds, L)
        row = None
        for p, caps, _ in threads:
            hit = [tags for tgt, cond, tags in self.follow[p] if tgt < 0 and not (cond & ~holds)]
            if hit:
                row = self._stamp(caps, hit[0], L)
                break
        if faults is not None and row != want:
            faults.append((L, "end_plain", "the ordered commit decides otherwise"))
        return (None if row is None else self._finish(s, row)), trace

    def _finish(self, s, caps):
        """run captures "(?=(S*))", as table_interp._with_run_captures"""
        for g, members in self.runs:
            b = caps[2 * g]
            if b >= 0:
                e = b
                while e < len(s) and s[e] in members:
                    e += 1
                caps[2 * g + 1] = e
        return caps

    def _audit_skip(self, s, i, threads, prev, cls, by_row, faults):
        """a skipped byte: the commit pass leaves the same threads, each with the memberships it held (a thread inside a group may be
        steady: (?>(?:.)+?(?>b)) skips with one membership alive); a doomed spawn (skipped by its row): what the spawn leaves is gone
        behind the next byte -- commit on byte i and on byte i + 1 against the commit on byte i + 1 alone"""
        full = self.plain_step(threads, cls, self.behind[prev] | self.ahead[cls], i)
        if not by_row:
            # (memberships included: a skipped thread keeps its own.)  A steady position of a search pattern may re-spawn the wrapper's
            # suffix thread (device_tables.h NF_OFF_STABLE): the commit pass then leaves a suffix thread, and nothing behind it, that the
            # skipped list lacks -- '\w(?:(?:c)++|(?:.)+)': the '.' loop above the prefix thread.  What ranks above that thread must
            # be the same; what the skip keeps below it cannot win: the thread that re-spawns the suffix thread reaches it on whatever byte ends it
            kept, want = self._norm(threads, True), self._norm(full, True)
            spawned = len(want) >= 2 and want[-1][0] == self.search_suffix and not want[-1][2] and \
                not any(p == self.search_suffix for p, _, _ in threads[:len(want)])
            if kept != want and not (spawned and kept[:len(want) - 1] == want[:-1]):
                faults.append((i, "skip", "the commit pass changes the thread list"))
            return
        c2 = int(self.cmap[s[i + 1]])
        h2 = self.behind[cls] | self.ahead[c2]
        a, b = self.plain_step(full, c2, h2, i + 1), self.plain_step(threads, c2, h2, i + 1)
        if self._norm(a) != self._norm(b):                                           # (new segment ids name the source thread's index)
            faults.append((i, "skip", "the doomed spawn is not gone behind the next byte"))

    def gate_faults(self, s, head=0, start=0):
        """where a skip or a vector step of the faithful walk is not what the full commit pass does on the same thread list"""
        faults = []
        self.walk(s, head, start, faults)
        return faults
