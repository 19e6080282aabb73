"""Inputs for the phase-1 tests of the Grok plan (tests/test_grok_plan_model.py on the CPU, tests/test_gpu_grok_plan.py on the device):
a batch builder that controls every value's offset and the bytes around it, the synthetic literal lists, and values derived from a
screen's own DFA (strings it accepts, strings that die or reach the sink at a chosen byte, neighbours that would flip the verdict)."""
import random
from collections import deque

import numpy as np

from loongcollector_amd import binding as B

FILLER = b"."          # a byte no synthetic literal contains
SENTINEL64 = 0x5A5A5A5A5A5A5A5A
SENTINEL32 = 0x5A5A5A5A


class Batch:
    """values laid out in one buffer: add(value, before, after, align) puts `before` + value + `after` at the cursor (align: the value's
    offset modulo 16).  finish() keeps the d_data contract of lc_grok.h: the buffer ends on a 16-byte boundary behind the last value."""

    def __init__(self):
        self.buf = bytearray()
        self.off, self.len, self.values = [], [], []

    def add(self, value, before=b"", after=b"", align=None, pad=FILLER):
        if align is not None:
            while (len(self.buf) + len(before)) % 16 != align:
                self.buf += pad
        self.buf += before
        self.off.append(len(self.buf))
        self.len.append(len(value))
        self.values.append(bytes(value))
        self.buf += value
        self.buf += after
        return len(self.values) - 1

    def finish(self):
        data = bytes(self.buf) + b"\0" * (16 + (-len(self.buf)) % 16)
        assert len(data) % 16 == 0 and len(data) < 2 ** 31
        return (np.frombuffer(data, dtype=np.uint8), np.array(self.off, dtype=np.uint32), np.array(self.len, dtype=np.uint32))


# ---- the literal pass ---------------------------------------------------------------------------------------------------------------
LITERAL_LENGTHS = (1, 2, 16, 31, 32, 33, 40)
VALUE_LENGTHS = (63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 4160, 8193)
CHUNKS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65)
DELTAS = (-1, 0, 1, 30, 31, 32, 33)


def synthetic_literal(i, k):
    """literal i of k bytes: an upper-case letter and one of x / y / z that no other literal begins with, then random lower-case
    letters (never the filler); no literal contains another (a one-byte literal: lists of up to 26)"""
    r = random.Random(100 + i)
    return (chr(ord("A") + i % 26) + "xyz"[i // 26] * (k > 1) + "".join(r.choice("abcdefghijklmnopqrstuvw") for _ in range(k - 2))).encode()


def literal_list(lengths=LITERAL_LENGTHS):
    return [synthetic_literal(i, k) for i, k in enumerate(lengths)]


def literal_match(lits):
    return [l.decode() + r"(?P<x>\d+)" if l else r"(?P<x>[%s%s]\d+)" % (chr(ord("a") + i % 13), chr(ord("n") + i % 13)) for i, l in enumerate(lits)]


def placed(L, lit, end):
    """a value of L filler bytes with `lit` ending (exclusively) at byte `end`"""
    v = bytearray(FILLER * L)
    v[end - len(lit):end] = lit
    assert len(v) == L and end - len(lit) >= 0 and end <= L
    return bytes(v)


def literal_sweep(batch, lits):
    """every literal at the chunk / look-behind edges of every value length, at the value's first and last byte, and the near misses:
    the literal cut by the value's end (front), its missing byte being the neighbour's"""
    for lit in lits:
        k = len(lit)
        for L in (k,) + VALUE_LENGTHS:
            if L < k:
                continue
            ends = {k, L} | {c * 64 + d for c in CHUNKS for d in DELTAS}
            for end in sorted(e for e in ends if e - k >= 0 and e <= L):
                batch.add(placed(L, lit, end))
            if k >= 2:
                batch.add(FILLER * (L - k + 1) + lit[:-1])     # cut by the value's end: the last byte is the next value's first
                batch.add(lit[-1:] + FILLER * 3 + lit[:1])     # ... and this value's last byte is the first byte of the literal
                batch.add(lit[1:] + FILLER * (L - k + 1))      # that the next value's front cuts
    return batch


QUAD_LENGTHS = [2049, 1025, 1024, 5, 0, 1, 2048, 1023, 65]
QUAD_SIZES = (1, 2, 3, 4, 5, 6, 7, 9)


def quad_values(lits, n, seed=0):
    """n values of QUAD_LENGTHS, every one with a different set of literals: a mask written to the wrong value, or OR-ed across a lane
    group, shows"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = QUAD_LENGTHS[(i + seed) % len(QUAD_LENGTHS)]
        v = bytearray(FILLER * L)
        want = (i * 37 + seed * 11 + 1) % (1 << len(lits))      # the set, as a mask (what fits is placed)
        at = L
        for p, lit in enumerate(lits):
            if (want >> p) & 1 and at - len(lit) >= 0:
                v[at - len(lit):at] = lit
                at -= len(lit) + rng.choice((0, 1, 30, 63))
        out.append(bytes(v))
    return out


# ---- values derived from a screen's DFA (tests.helpers.grok_plan_model.Screen) --------------------------------------------------------
def class_bytes(sc):
    """per byte class the bytes of it, printable ones first"""
    if getattr(sc, "_per", None) is None:
        sc._per = [[] for _ in range(sc.ncls)]
        for b in list(range(32, 127)) + list(range(0, 32)) + list(range(127, 256)):
            sc._per[sc.cmap[b]].append(b)
    return sc._per


def path_to(sc, state, goal, avoid=lambda s: False, max_len=400):
    """shortest byte string from `state` to a state with goal(s); never through the dead state or avoid(s).  None: there is none"""
    per = class_bytes(sc)
    if goal(state):
        return b""
    seen = {state: None}
    q = deque([state])
    while q:
        s = q.popleft()
        for c in range(sc.ncls):
            if not per[c]:
                continue
            t = sc.table[s * sc.ncls + c]
            if t in seen or (t == 0 and not goal(0)) or (avoid(t) and not goal(t)):
                continue
            seen[t] = (s, per[c][0])
            if goal(t):
                out = bytearray()
                while seen[t] is not None:
                    t, b = seen[t]
                    out.append(b)
                return bytes(reversed(out)) if len(out) <= max_len else None
            q.append(t)
    return None


def accepted(sc):
    """a shortest string the screen passes"""
    return path_to(sc, sc.start, lambda s: s == sc.sink or (s != 0 and sc.accept[s]))


def alive_walk(sc, rng, L, state=None):
    """L bytes that keep the automaton away from the dead state and the sink for as long as it can be -> (bytes, end state)"""
    per = class_bytes(sc)
    state = sc.start if state is None else state
    out = bytearray()
    while len(out) < L:
        nxt = [(sc.table[state * sc.ncls + c], c) for c in range(sc.ncls) if per[c]]
        good = [(t, c) for t, c in nxt if t != 0 and t != sc.sink] or [(t, c) for t, c in nxt if t != 0] or nxt
        t, c = rng.choice(good)
        out.append(rng.choice(per[c][:4]))
        state = t
        if t == 0 or t == sc.sink:
            out += bytes(rng.choice(per[rng.randrange(sc.ncls)] or [46]) for _ in range(L - len(out)))
    return bytes(out), sc.walk(bytes(out))


def flipping_tail(sc, state):
    """bytes behind a value that ended in `state` which would change the verdict if the walk ran on: towards acceptance for a value
    that does not pass, towards the dead state (or any non-accepting state) for one that does"""
    passing = state == sc.sink or (state != 0 and sc.accept[state])
    if state == 0 or state == sc.sink:
        return (accepted(sc) or b"")[:16]
    if passing:
        t = path_to(sc, state, lambda s: s == 0 or not sc.accept[s], max_len=16)
    else:
        t = path_to(sc, state, lambda s: s == sc.sink or (s != 0 and sc.accept[s]), max_len=64)
    return (t or b"")[:16]


def ends_at(sc, rng, goal, at):
    """a string whose byte number `at` (and no earlier one) takes the walk to the dead state (goal = 0) or to the sink; None if the
    search does not find one"""
    d = 1
    for _ in range(60):
        if at + 1 - d < 0:
            d = 1
        head, s = alive_walk(sc, rng, at + 1 - d)
        if s in (0, sc.sink):
            continue
        tail = path_to(sc, s, lambda t: t == goal, avoid=lambda t: t == sc.sink, max_len=at + 1)
        if tail is None:
            continue
        if len(tail) == d:
            w = head + tail
            assert sc.walk(w) == goal and sc.walk(w[:-1]) not in (0, sc.sink) and len(w) == at + 1
            return w
        d = len(tail)
    return None


def unit_end_values(batch, sc, lit, rng):
    """The walks test for the sink and the dead state once per aligned 16-byte unit.  For every offset of the value modulo 16 and every
    byte j of a unit: a value whose walk dies exactly at that byte of a unit and one whose walk reaches the sink there, with a
    string behind -- inside the value -- that a restarted walk would accept.  -> the set of (j, dead or sink) produced: every j, for each end the automaton has."""
    acc = accepted(sc) or b""
    made = set()
    # (a search automaton restarts instead of dying: the screens of unanchored formats have no reachable dead state)
    kinds = [(sc.sink, "sink")] + ([(0, "dead")] if path_to(sc, sc.start, lambda t: t == 0) is not None else [])
    for align in range(16):
        for j in range(16):
            at = (j - align) % 16 + 32 + 16 * ((align + j) % 2)      # byte number inside the value; (align + at) % 16 == j
            for goal, kind in kinds:
                w, al = ends_at(sc, rng, goal, at), align
                if w is None:          # (the shortest walk from the start state, at the offset that puts its last byte on j)
                    w = path_to(sc, sc.start, lambda t: t == goal, avoid=lambda t: t == sc.sink)
                    al = (j - (len(w) - 1)) % 16
                batch.add(w + acc + (lit or b"") + FILLER * (j % 5), before=FILLER, after=acc[:8] or FILLER, align=al)
                assert (batch.off[-1] + len(w) - 1) % 16 == j and sc.walk(w) == goal and sc.walk(w[:-1]) not in (0, sc.sink)
                made.add(((batch.off[-1] + len(w) - 1) % 16, kind))     # (where the walk's last byte really lies)
    assert made == {(j, kind) for j in range(16) for _, kind in kinds}
    return made


def screen_edge_values(batch, sc, lit, rng, lengths=(0, 1, 15, 16, 17, 31, 32, 33, 48, 4096), splice=0.5):
    """For one screen, at every offset modulo 16: values of every length that stay alive as long as they can, with the bytes in front
    and behind chosen to flip the verdict; values that die / reach the sink at byte j with an accepted string behind; an accepted
    string cut by either end of the value.  `lit`: the entry's literal, spliced in where it fits (the screen is consulted only for
    values that carry it)."""
    acc = accepted(sc) or b""
    to_sink = path_to(sc, sc.start, lambda s: s == sc.sink) if sc.sink != 0xFFFFFFFF else None
    for align in range(16):
        for L in lengths:
            v, end = alive_walk(sc, rng, L)
            if lit and L >= len(lit) + 2 and rng.random() < splice:
                at = rng.randrange(0, L - len(lit))
                v = v[:at] + lit + v[at + len(lit):]
                end = sc.walk(v)
            batch.add(v, before=acc[:1] or FILLER, after=flipping_tail(sc, end) or FILLER, align=align)
        # an accepted string whose first / last byte is the neighbour's, and the whole of it with one more byte of it behind
        if len(acc) >= 2:
            batch.add(acc[1:], before=acc[:1], after=FILLER, align=align)
            batch.add(acc[:-1], before=FILLER, after=acc[-1:], align=align)
            batch.add(acc, before=acc[-1:], after=flipping_tail(sc, sc.walk(acc)) or FILLER, align=align)
    return batch


# ---- the 50-entry list of configs[2] --------------------------------------------------------------------------------------------------
GROK_SYNTAX = (B.LC_SYNTAX_SEARCH | B.LC_SYNTAX_NAMED_ONLY | B.LC_SYNTAX_NO_DOTALL | B.LC_SYNTAX_NO_MULTILINE
               | B.LC_SYNTAX_REGEXP2)
EDGE_SCREENS = (0, 5, 6, 9, 20)      # entries of configs[2] without a literal or with a one-byte one: their screens see most values


def required_literals(g):
    return [B.GpuRegex(g.expanded(i).encode("utf-8"), syntax_flags=GROK_SYNTAX).required_literal() for i in range(g.n_match)]


def config3_edge_values(screens, lits, seed=11, lengths=(0, 1, 15, 16, 17, 31, 32, 33, 48, 4096)):
    """the edge values of the screen tests (section 3 of the phase-1 tests), as a Batch"""
    rng = random.Random(seed)
    batch = Batch()
    for p in EDGE_SCREENS:
        screen_edge_values(batch, screens[p], lits[p], rng, lengths=lengths)
    for p in (0, 9):                  # (no literal: every value is looked at; "[": ten states)
        unit_end_values(batch, screens[p], lits[p], rng)
    # ... and whole log lines, which the screens of their formats PASS after a walk to the last byte, at every offset modulo 16, their
    # neighbours one byte away
    from loongcollector_amd.grok_corpus import grok_lines
    for i, line in enumerate(grok_lines(480, seed=77)):
        batch.add(line, before=b"]", after=b"[", align=i % 16)
    return batch
