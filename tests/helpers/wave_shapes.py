"""Test-only corpus for the TDFA stream kernels (csrc/tdfa_stream_kernel.hpp, csrc/tdfa_kernel.hpp tdfaWriteResults): batches in
which a WAVE -- 64 consecutive lines -- has a shape chosen on purpose.  The kernels map slot = block * BLOCK + tid, so lines
64k .. 64k+63 are one wavefront for every workgroup size, and much of their control flow is decided per wavefront: the copy of
the chunk loop from the wave's shortest span (allNextInside: minSpan >= s0 + 64 + 8; nextInsideButLast: >= s0 + 64; waveFull per
chunk; the unchecked copy of the other kernels only when every lane's next chunk is full), the epilogue's path from __all(live),
one accepting state per wave, the number of output slots and the alignment of the capture table.

Wave kinds (the label of a wave is (kind, L)):
  uniform     all 64 lines have length L, for every L of UNIFORM_L: every chunk (8), pair (2), 16-byte segment and 64-byte stage
              boundary of the first four stages with +-9 around them, and 511..513
  one_short   63 lines of length L and one of length 0, 1, L-1, L-8 or L-9 in lane 0, 31, 32 or 63 (rotating), L of EDGE_L
              (Family.edge_len: WORDS(k) moves a length it cannot match up by whole stages)
  one_long    63 lines of 10 bytes and one of length L: the wave's stage count comes from one lane, the others walk the identity column
  all_dead    every line fails, in the byte the label names as L (byte 0, a byte of chunk 7 of stage 0, the first byte of stage 1)
  half_dead   even lanes fail in their first bytes, odd lanes match at length L
  two_formats the lines match through different alternatives and end in different accepting states, L of TWO_FORMAT_L
  tail        the last wave has 31 lines only; Corpus.cut_counts() gives n = 64k + r for r of TAIL_R

Content of the uniform waves.  Lane j places its field separators where j says; lanes are chosen one after the other, each from a
handful of candidates, to cover what the wave and the batch still lack: every offset of the wave's last 18 (two chunks and a pair)
as a capture begin and as a capture end inside the wave, every offset 0..L as a begin and as an end over the batch.  A few lanes
carry the lines a family names itself (specials): empty fields at offset 0, at L and at the first byte of a stage, a field that
ends on the last byte of a stage.  One-byte fields (the DOUBLE entries of the pair tables) begin at even and at odd offsets.
Two lanes of a uniform wave are NEEDY where the pattern can be: a line that fails for want of one more byte, with that very byte
behind it in the packed data.  Every pattern here ends in (.*), so on a line that matches a walk that takes one byte too many
changes nothing -- status and captures stay what they were; on a needy line it turns a failure into a match (SWEEP, which no line
fails: it moves the end of a capture).
What a pattern cannot do is said by its family: SWEEP accepts every byte string (every part of it is optional and the dot matches
a newline), so it has no failing line and no all_dead / half_dead wave; FIELDS, ALT and WORDS cannot begin an empty field at
offset 0, and WORDS(k) has no match shorter than 2k - 3 bytes.  tests/test_tdfa_wave_shapes.py asserts all of this against the
oracle, so that the GPU test cannot pass on a degenerate corpus.

Python's own `re` is used here to choose among candidate lines only (same Perl semantics for these patterns); what a line is
expected to give always comes from the oracle.  Not part of the product, never imported by loongcollector_amd/.
"""
import functools
import re
from collections import namedtuple

import numpy as np

SWEEP = rb"(\w*) ?(\d?)(\d*)([^|]*)\|?(.?)(.*)"
FIELDS = rb"(\w)(\w)(\w?)(\w*),(\d?)(\d*);(.)(.)(.*)"           # (tests/test_gpu_deferred_stamps.py FIELDS)
ALT = rb"(a|ab)(c|bcd)(d*)(.*)"


def WORDS(k):
    return b" ".join([rb"(\w+)"] * (k - 1)) + rb" ?(.*)"


UNIFORM_L = (list(range(0, 19)) + list(range(55, 75)) + list(range(119, 139)) + list(range(183, 203)) +
             [247, 248, 255, 256, 257, 264, 511, 512, 513])
assert len(UNIFORM_L) == 88
EDGE_L = (64, 65, 72, 73, 128, 136, 137, 200)
SHORT_LANES = (0, 31, 32, 63)
TWO_FORMAT_L = (72, 130)
DEAD_AT = (0, 60, 64)            # byte 0, a byte of chunk 7 of stage 0, the first byte of stage 1
TAIL_R = (1, 31, 63)
TAIL_L = 136
NEEDY_LANES = 2                  # lines of a uniform wave that fail for want of one more byte
WINDOW = 18                      # offsets L-17 .. L: the last two chunks and a pair
COVER_MAX = 264                  # the offset-coverage rules hold for every uniform L up to here
STAGE = 64


def short_lengths(L):
    return (0, 1, L - 1, L - 8, L - 9)


Wave = namedtuple("Wave", "kind L first count detail")


def _clamp(v, lo, hi):
    return max(lo, min(int(v), hi))


def _pick(rng, alphabet, n):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), size=n).astype(np.uint8)) if n > 0 else b""


class Family:
    """A pattern and how to write lines for it.  make(L, aim, rng): a line of exactly L bytes that matches whenever L >= min_len,
    with one of its free separators at (or just below) offset `aim`; specials(L): lines a uniform wave of length L must carry;
    dead(L, at): a line of L bytes that reaches the dead state in byte `at` (None: the pattern cannot); formats(L): lines of L bytes
    that match through different alternatives."""
    name = pattern = None
    min_len = 0           # no shorter line matches
    free_len = 0          # from this length on a line has room to put a separator anywhere in its last WINDOW offsets
    first_begin = 0       # every offset from here on can be a capture begin / end (smaller ones are pinned by the pattern)
    first_end = 0
    can_fail = True
    empty_at_0 = False    # an empty capture at offset 0 exists
    empty_in_stage = False  # an empty capture at the first byte of a stage INSIDE the line exists (not only at its end)
    dead_at = DEAD_AT

    def edge_len(self, L):
        """a length of EDGE_L / TAIL_L as this family's waves carry it: moved up by whole stages until a line of that length can match
        with room to spare (the same place in its chunk, pair and stage; WORDS(k) only)"""
        while L < self.min_len + 9:
            L += STAGE
        return L

    def specials(self, L):
        return []

    needy_matches = False  # SWEEP, which no line fails: its needy lines match, and one more byte moves a capture

    def needy(self, L, rng):
        """-> (a line of L bytes that fails for want of ONE more byte, that byte) or None: what a walk that takes a byte too many
        turns into a match.  (Every pattern here ends in (.*): on most lines that match, a byte too many changes nothing.)"""
        return None

    def dead(self, L, at):
        return None

    def early_dead(self, L, j):
        return self.dead(L, self.dead_at[0])


class SweepFamily(Family):
    name, pattern = "sweep", SWEEP
    can_fail = False
    empty_at_0 = empty_in_stage = True
    dead_at = ()

    @staticmethod
    def _line(L, c1, c2, c3, rng):
        """word bytes [0, c1), a space and digits [c1, c2), filler [c2, c3), a bar at c3 (if c3 < L) and anything behind it"""
        s = _pick(rng, b"aZ_9q", c1)
        if c2 > c1:
            s += b" " + _pick(rng, b"0123456789", c2 - c1 - 1)
        s += _pick(rng, b"-.#-", c3 - c2)
        if c3 < L:
            s += b"|" + _pick(rng, b"xy |7,", L - c3 - 1)
        assert len(s) == L
        return s

    def make(self, L, aim, rng):
        c3 = _clamp(aim - int(rng.integers(0, 3)), 0, L)
        c2 = int(rng.integers(0, c3 + 1))
        c1 = int(rng.integers(0, c2 + 1))
        shape = int(rng.integers(0, 4))
        if shape == 1:
            c2 = c1                               # no digits: the second and third field empty
        elif shape == 2:
            c2 = c3                               # the bar right behind the digits: the fourth field empty
        elif shape == 3:
            c1 = c2 = c3 = _clamp(aim, 0, L)      # words up to the bar
        return self._line(L, c1, c2, c3, rng)

    needy_matches = True

    def needy(self, L, rng):
        """words and a space: the digit fields are empty at L -- and the first of them is [L, L + 1) for a walk that takes the digit behind"""
        return (self._line(L, L - 1, L, L, rng), b"7") if L >= 1 else None

    def specials(self, L):
        rng = np.random.default_rng(L)
        out = [self._line(L, 0, 0, 0, rng), self._line(L, L, L, L, rng)]           # fields 1-4 empty at 0; fields 2-6 empty at L
        for s0 in range(STAGE, min(L, 4 * STAGE) + 1, STAGE):
            out.append(self._line(L, s0, s0, s0, rng))                             # field 1 ends on the stage's last byte, 2-4 empty behind it
        if L >= 4:
            out.append(self._line(L, 0, 2, 2, rng))                                # " d|...": a one-byte field at an odd offset
            out.append(self._line(L, 1, 3, 3, rng))                                # and at an even one
        return out

    def formats(self, L):
        rng = np.random.default_rng(L)
        return [self._line(L, L, L, L, rng), self._line(L, 5, 9, L, rng), self._line(L, 5, 9, 20, rng), self._line(L, 0, 0, L - 1, rng),
                self._line(L, 3, 3, L - 2, rng), self._line(L, 4, L, L, rng)]


class FieldsFamily(Family):
    name, pattern = "fields", FIELDS
    min_len, free_len, first_begin, first_end = 6, 30, 3, 1
    empty_in_stage = True

    @staticmethod
    def _line(L, a, c2, rng):
        """word bytes [0, a), a comma at a, digits, a semicolon at c2, two bytes, anything"""
        s = _pick(rng, b"ab1_9", a) + b"," + _pick(rng, b"0123456789", c2 - a - 1) + b";" + _pick(rng, b"pq ,;", 2) + _pick(rng, b"ab1 ,;_9", L - c2 - 3)
        assert len(s) == L and 2 <= a < c2 <= L - 3
        return s

    def make(self, L, aim, rng):
        if L < self.min_len:
            return b"ab,1;p"[:L]
        if rng.integers(0, 2):
            c2 = _clamp(aim - int(rng.integers(0, 4)), 3, L - 3)
            a = c2 - 1 if rng.integers(0, 3) == 0 else int(rng.integers(2, c2))
        else:
            a = _clamp(aim - int(rng.integers(0, 3)), 2, L - 4)
            c2 = a + 1 if rng.integers(0, 3) == 0 else int(rng.integers(a + 1, L - 2))
        return self._line(L, a, c2, rng)

    def specials(self, L):
        if L < self.min_len:
            return []
        rng = np.random.default_rng(L)
        out = [self._line(L, 2, L - 3, rng), self._line(L, L - 4, L - 3, rng)]     # the last field empty at L
        for s0 in range(STAGE, 4 * STAGE + 1, STAGE):
            if s0 + 3 <= L:
                out.append(self._line(L, s0 - 1, s0, rng))                         # the digit fields empty at the stage's first byte
                out.append(self._line(L, 2, s0 - 3, rng))                          # the second one-byte field ends on the stage's last byte
        return out

    def needy(self, L, rng):
        if L < 5:
            return None
        a = int(rng.integers(2, L - 2))
        return self._line(L + 1, a, L - 2, rng)[:L], b"q"             # one byte behind the semicolon: the second one is missing

    def dead(self, L, at):
        s = (b"," if at == 0 else b"ab" + b"c" * (at - 2) + b";") + b"x,1;pq" * (L // 6 + 1)
        return s[:L] if at == 0 or at >= 2 else None

    def early_dead(self, L, j):
        return self.dead(L, (0, 2, 3)[j // 2 % 3])

    def formats(self, L):
        rng = np.random.default_rng(L)
        return [self._line(L, 2, L - 3, rng), self._line(L, 5, 9, rng), self._line(L, 3, 4, rng), self._line(L, L - 4, L - 3, rng)]


class AltFamily(Family):
    name, pattern = "alt", ALT
    min_len, free_len, first_begin, first_end = 2, 30, 0, 1
    dead_at = (0, 1, 2)
    PREFIX = (b"ac", b"abc", b"abcd", b"abbcd")

    @staticmethod
    def _line(L, prefix, c, rng):
        """an alternative of each of the first two groups, d's up to c, then something that is no d"""
        s = prefix + b"d" * (c - len(prefix))
        if c < L:
            s += b"x" + _pick(rng, b"dxa c", L - c - 1)
        assert len(s) == L
        return s

    def make(self, L, aim, rng):
        if L < self.min_len:
            return b"a"[:L]
        fits = [p for p in self.PREFIX if len(p) <= L]
        prefix = fits[int(rng.integers(0, len(fits)))]
        return self._line(L, prefix, _clamp(aim, len(prefix), L), rng)

    def specials(self, L):
        rng = np.random.default_rng(L)
        return [self._line(L, p, L, rng) for p in self.PREFIX[:2] if len(p) <= L]   # the last field empty at L

    def needy(self, L, rng):
        return {1: (b"a", b"c"), 2: (b"ab", b"c"), 4: (b"abbc", b"d")}.get(L)

    def dead(self, L, at):
        return ((b"x", b"ax", b"abx")[at] + b"acdx" * (L // 4 + 1))[:L] if at <= 2 and L > at else None

    def early_dead(self, L, j):
        return self.dead(L, j // 2 % 3)

    def formats(self, L):
        rng = np.random.default_rng(L)
        return ([self._line(L, p, L, rng) for p in self.PREFIX] + [self._line(L, p, len(p), rng) for p in self.PREFIX] +
                [self._line(L, p, 40, rng) for p in self.PREFIX])


class WordsFamily(Family):
    def __init__(self, k):
        self.k, self.nw = k, k - 1
        self.name, self.pattern = "words%d" % k, WORDS(k)
        self.min_len = 2 * self.nw - 1
        self.free_len = self.min_len + 40
        self.first_begin, self.first_end = 2, 1

    @staticmethod
    def _compose(total, parts, rng):
        """`parts` positive lengths that add up to `total`"""
        cuts = np.sort(rng.integers(0, total - parts + 1, size=parts - 1))
        edges = np.concatenate(([0], cuts, [total - parts]))
        return [int(x) + 1 for x in np.diff(edges)]

    def _line(self, L, lens, tail_mode, rng):
        """the words, then (tail_mode) 0: nothing, 1: a space and the rest, 2: the rest behind a byte that is no word byte"""
        arr = rng.choice(np.frombuffer(b"wQ_7", np.uint8), size=sum(lens) + len(lens) - 1).astype(np.uint8)
        arr[np.cumsum(np.asarray(lens) + 1)[:-1] - 1] = 32
        s = bytes(arr)
        if tail_mode == 1 and len(s) < L:
            s += b" " + _pick(rng, b"t -7", L - len(s) - 1)
        elif len(s) < L:
            s += b"-" + _pick(rng, b"t -7", L - len(s) - 1)
        assert len(s) == L, (L, len(s), tail_mode)
        return s

    def make(self, L, aim, rng):
        nw = self.nw
        if L < self.min_len:
            return (b"w " * (L // 2 + 1))[:L]
        aim = _clamp(aim, 0, L)
        # word i begins at aim: i spaces and i words in front of it, 2 * (nw - i) - 1 bytes at least from it on
        lo, hi = max(1, nw - (L - aim + 1) // 2), min(nw - 1, aim // 2)
        if lo <= hi and rng.integers(0, 3):
            i = int(rng.integers(lo, hi + 1))
            rest = int(rng.integers(2 * (nw - i) - 1, L - aim + 1))               # bytes of words i .. nw-1 and the spaces between them
            lens = self._compose(aim - i, i, rng) + self._compose(rest - (nw - i - 1), nw - i, rng)
            return self._line(L, lens, int(rng.integers(1, 3)), rng)
        # the last field begins at aim (behind a space, or at a byte that is no word byte), or the words run to the end
        mode = int(rng.integers(1, 3))
        area = aim - 1 if mode == 1 else aim
        if aim >= L and rng.integers(0, 2):
            area, mode = L, 0
        if area < self.min_len:
            area = int(rng.integers(self.min_len, L + 1))
        return self._line(L, self._compose(area - (nw - 1), nw, rng), mode if area < L else 0, rng)

    def specials(self, L):
        if L < self.min_len:
            return []
        rng = np.random.default_rng(L)
        out = [self._line(L, self._compose(L - (self.nw - 1), self.nw, rng), 0, rng)]             # the last field empty at L, no space
        if L > self.min_len:
            out.append(self._line(L, self._compose(L - 1 - (self.nw - 1), self.nw, rng), 1, rng))   # ... behind a space
        return out

    def needy(self, L, rng):
        if L < 2 * (self.nw - 1):
            return None
        lens = self._compose(L - 1 - (self.nw - 2), self.nw - 1, rng)
        return self._line(L - 1, lens, 0, rng) + b" ", b"w"            # the space in front of the last word, and no last word

    def dead(self, L, at):
        """one-byte words, then a second space where word at/2 should begin"""
        if at % 2 or at // 2 >= self.nw or L <= at:
            return None
        return ((b"w " * (at // 2)) + b" " + b"w " * L)[:L]

    def early_dead(self, L, j):
        return self.dead(L, (0, 2, 4)[j // 2 % 3])

    def formats(self, L):
        rng = np.random.default_rng(L)
        nw, m = self.nw, self.min_len
        if L < m + 3:
            return []
        return [self._line(L, self._compose(L - (nw - 1), nw, rng), 0, rng), self._line(L, [1] * nw, 1, rng), self._line(L, [1] * nw, 2, rng),
                self._line(L, self._compose(L - 1 - (nw - 1), nw, rng), 1, rng)]


FAMILIES = {f.name: f for f in (SweepFamily(), FieldsFamily(), AltFamily(), WordsFamily(40), WordsFamily(70))}


class Corpus:
    def __init__(self, family, lines, waves, meant, after):
        """meant[i]: line i is written to match; after[i]: the byte behind line i in the packed data (never part of the line)"""
        self.family, self.lines, self.waves, self.meant, self.after = family, lines, waves, np.array(meant, bool), after
        self.wave_of = np.repeat(np.arange(len(waves)), [w.count for w in waves])

    def label(self, i):
        """which wave and lane line i is: for failure messages"""
        w = self.waves[int(self.wave_of[i])]
        return "%s: wave %d (%s, L=%d%s), lane %d, line %d of %d bytes" % (
            self.family.name, int(self.wave_of[i]), w.kind, w.L, ", " + w.detail if w.detail else "", i - w.first, i, len(self.lines[i]))

    def pack(self, n=None):
        """-> (data, off[n+1], len[n]): the first n lines, each followed by one separator byte (a newline, or what a needy line lacks)"""
        lines = self.lines if n is None else self.lines[:n]
        length = np.array([len(s) for s in lines], np.uint32)
        off = np.zeros(len(lines) + 1, np.uint32)
        off[1:] = np.cumsum(length + np.uint32(1))
        data = np.frombuffer(b"".join(s + a for s, a in zip(lines, self.after)), np.uint8)
        return data, off, length

    def cut_counts(self):
        """n = 64k + r for r of TAIL_R: the last wave has lanes without a line (the cut falls into waves of different kinds)"""
        nw = len(self.waves)
        return [64 * k + r for k, r in zip((nw - 2, nw // 2, 3), TAIL_R)]

    def waves_of(self, kind):
        return [w for w in self.waves if w.kind == kind]


def _uniform_wave(fam, rx, L, rng, need_b, need_e):
    """64 lines of length L; need_b / need_e: the offsets the batch still lacks as a capture begin / end (updated)"""
    G = rx.groups
    win_b = set(range(max(0, L - WINDOW + 1), L + 1))
    win_e = set(win_b)

    def spans(s):
        m = rx.fullmatch(s)
        return [] if m is None else [m.span(g) for g in range(1, G + 1)]

    def take(s):
        for b, e in spans(s):
            for pool in (win_b, need_b):
                pool.discard(b)
            for pool in (win_e, need_e):
                pool.discard(e)

    lanes, after = [None] * 64, {}
    for k, s in enumerate(fam.specials(L)[:12]):
        lanes[(L + 5 + 9 * k) % 64] = s
        take(s)
    for k in range(NEEDY_LANES):                     # lines that fail for want of one byte, in lanes that move with L
        nd = fam.needy(L, rng)
        if nd is not None:
            j = next(j % 64 for j in range(7 * L + 29 * k, 7 * L + 29 * k + 64) if lanes[j % 64] is None)
            lanes[j], after[j] = nd
    for j in range(64):
        if lanes[j] is not None:
            continue
        aims = [(j * (L + 1)) // 64]
        for pool in (win_b, win_e):
            if pool:
                aims.append(max(pool))
        for pool in (need_b, need_e):
            below = [o for o in pool if o <= L]
            if below:
                aims += [min(below), max(below)]
        if len(aims) > 1:
            aims.append(int(rng.integers(0, L + 1)))
        best, best_score = None, -1
        for aim in aims:
            for _ in range(2 if len(aims) > 1 else 1):
                s = fam.make(L, aim, rng)
                sp = spans(s)
                score = (100 * (len(win_b & {b for b, _ in sp}) + len(win_e & {e for _, e in sp})) +
                         len(need_b & {b for b, _ in sp}) + len(need_e & {e for _, e in sp}))
                if score > best_score:
                    best, best_score = s, score
        lanes[j] = best
        take(best)
    return lanes, after


@functools.lru_cache(maxsize=None)
def generate(family, seed=1):
    """-> Corpus for FAMILIES[family] (computed once per process: callers leave it unchanged)"""
    fam = FAMILIES[family]
    rng = np.random.default_rng(seed)
    rx = re.compile(fam.pattern, re.S)
    lines, waves, meant, after = [], [], [], []

    def add(kind, L, wave_lines, detail="", fails=(), behind=None):
        """fails: the lanes written to fail; behind: lane -> the byte behind its line"""
        waves.append(Wave(kind, L, len(lines), len(wave_lines), detail))
        lines.extend(wave_lines)
        meant.extend(len(s) >= fam.min_len and j not in fails for j, s in enumerate(wave_lines))
        after.extend((behind or {}).get(j, b"\n") for j in range(len(wave_lines)))

    def some(L):
        return fam.make(L, int(rng.integers(0, L + 1)), rng)

    need_b, need_e = set(range(COVER_MAX + 1)), set(range(COVER_MAX + 1))
    for L in UNIFORM_L:
        wave_lines, behind = _uniform_wave(fam, rx, L, rng, need_b, need_e)
        add("uniform", L, wave_lines, fails=() if fam.needy_matches else set(behind), behind=behind)
    turn = 0
    for L in map(fam.edge_len, EDGE_L):
        for short in short_lengths(L):
            lane = SHORT_LANES[turn % 4]
            turn += 1
            w = [some(L) for _ in range(64)]
            w[lane] = some(short)
            add("one_short", L, w, "%d bytes in lane %d" % (short, lane))
    for L in map(fam.edge_len, EDGE_L):
        lane = SHORT_LANES[turn % 4]
        turn += 1
        w = [some(10) for _ in range(64)]
        w[lane] = some(L)
        add("one_long", L, w, "lane %d" % lane)
    if fam.can_fail:
        for at in fam.dead_at:
            add("all_dead", at, [fam.dead(at + 8 + j, at) for j in range(64)], "fails in byte %d" % at, fails=range(64))
        for L in map(fam.edge_len, EDGE_L):
            add("half_dead", L, [some(L) if j % 2 else fam.early_dead(8 + j, j) for j in range(64)], fails=range(0, 64, 2))
    for L in map(fam.edge_len, TWO_FORMAT_L):
        fmts = fam.formats(L)
        add("two_formats", L, [fmts[(j + j // len(fmts)) % len(fmts)] for j in range(64)])
    add("tail", fam.edge_len(TAIL_L), [some(fam.edge_len(TAIL_L)) for _ in range(TAIL_R[1])])
    assert all(s is not None for s in lines)
    return Corpus(fam, lines, waves, meant, after)


# ---- the instantiations of tdfa_stream_kernel the GPU test runs the corpus through: the environment a pattern is compiled and launched
# under, the kernel name lc_launched_kernels must report, and the table format that goes with it (read from the blob header: TD_BLOCK,
# TD_OFF_PAIR / TP_FORMAT, TD_NREGS bit 31).  compact: the launch walks the compact tables (LC_TABLE_TDFA_WIDE_BLOB, 16-bit registers);
# pair: None = no byte-pair table, 0 = two stamps per pair entry, 1 = one stamp.
ENV_KEYS = ("LC_TDFA_PAIR", "LC_TDFA_COMPACT", "LC_TDFA_DEFER_STAMPS")
Inst = namedtuple("Inst", "id env family kernel block compact pair nogen")
_P2C = {"LC_TDFA_PAIR": "2", "LC_TDFA_COMPACT": "512"}
INSTANTIATIONS = [
    Inst("pair1-256-sweep", {"LC_TDFA_PAIR": "2"}, "sweep", "tdfa_stream_kernel<nogeneral,pair1>", 256, False, 1, True),
    Inst("pair1-128-words40", {}, "words40", "tdfa_stream_kernel<nogeneral,pair1>", 128, False, 1, True),
    Inst("nogeneral-256-fields", {}, "fields", "tdfa_stream_kernel<nogeneral>", 256, False, None, True),
    Inst("nogeneral-64-words70", {}, "words70", "tdfa_stream_kernel<nogeneral>", 64, False, None, True),
    Inst("general-256-alt", {}, "alt", "tdfa_stream_kernel", 256, False, None, False),
    Inst("pair-256-fields", {"LC_TDFA_PAIR": "1"}, "fields", "tdfa_stream_kernel<pair>", 256, False, 0, True),
    Inst("pair-256-alt", {"LC_TDFA_PAIR": "1"}, "alt", "tdfa_stream_kernel<pair>", 256, False, 0, False),
    Inst("compact-256-fields", {"LC_TDFA_PAIR": "0", "LC_TDFA_COMPACT": "256"}, "fields", "tdfa_stream_kernel<compact,nogeneral,dma>", 256, True, None, True),
    Inst("compact-512-fields", {"LC_TDFA_PAIR": "0", "LC_TDFA_COMPACT": "512"}, "fields", "tdfa_stream_kernel<compact,nogeneral,dma>", 512, True, None, True),
    Inst("compact-256-alt", {"LC_TDFA_PAIR": "0", "LC_TDFA_COMPACT": "256"}, "alt", "tdfa_stream_kernel<compact,dma>", 256, True, None, False),
    Inst("compact-512-alt", {"LC_TDFA_PAIR": "0", "LC_TDFA_COMPACT": "512"}, "alt", "tdfa_stream_kernel<compact,dma>", 512, True, None, False),
    Inst("compact-pair-256-fields", {"LC_TDFA_PAIR": "1", "LC_TDFA_COMPACT": "256"}, "fields", "tdfa_stream_kernel<compact,pair>", 256, True, 0, True),
    Inst("compact-pair-256-alt", {"LC_TDFA_PAIR": "1", "LC_TDFA_COMPACT": "256"}, "alt", "tdfa_stream_kernel<compact,pair>", 256, True, 0, False),
    Inst("compact-pair1-512-sweep", dict(_P2C, LC_TDFA_DEFER_STAMPS="0"), "sweep", "tdfa_stream_kernel<compact,nogeneral,pair1,dma>", 512, True, 1, True),
    Inst("compact-pair1-512-fields", dict(_P2C, LC_TDFA_DEFER_STAMPS="0"), "fields", "tdfa_stream_kernel<compact,nogeneral,pair1,dma>", 512, True, 1, True),
    Inst("compact-pair1-512-defer-sweep", dict(_P2C, LC_TDFA_DEFER_STAMPS="1"), "sweep", "tdfa_stream_kernel<compact,nogeneral,pair1,dma,defer>", 512, True, 1, True),
    Inst("compact-pair1-512-defer-fields", dict(_P2C, LC_TDFA_DEFER_STAMPS="1"), "fields", "tdfa_stream_kernel<compact,nogeneral,pair1,dma,defer>", 512, True, 1, True),
]


def table_format(blob):
    """-> (TD_BLOCK, pair format or None, no-general bit) of a packed TDFA blob (csrc/device_tables.h)"""
    po = int(blob[7])                                             # TD_OFF_PAIR
    return int(blob[15]), (int(blob[po // 4 + 4]) if po else None), bool(int(blob[3]) >> 31)


def set_env(monkeypatch, inst):
    """the environment of an instantiation: set before the pattern is compiled, kept for the launch"""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in inst.env.items():
        monkeypatch.setenv(k, v)
