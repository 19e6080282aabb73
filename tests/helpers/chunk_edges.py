"""Test-only corpus for the engines that walk ONE VALUE PER WAVEFRONT (csrc/nfa_kernel.hpp nfa_match_kernel, csrc/nfa_wide_kernel.hpp,
csrc/tdfa_l2_kernel.hpp tdfaWaveBody) and for their lane-per-value neighbours (tdfa_l2_kernel, nfa_decide_kernel, nfa_dfs_kernel,
bt_match_kernel): values in which ONE decision of the walk falls on a chosen byte, for every alignment of the value's first byte.

The wave walks hold a 256-byte chunk of the value as one dword per lane.  The view is word-aligned (head = address & 3), so a chunk
border falls at line offset 256k - head.  tdfa_l2_kernel reads 16-byte pieces (head = address & 15).  Every shortcut inside a chunk --
the steady / quiet run scan, the search skip, the doomed-spawn look-ahead, the chunk reload, the resume chunk, the suffix-thread exit,
the stop on the absorbing state -- is a comparison against a chunk border, the end of the value or the start offset.

A case is (family, kind, variant, p, head, line, after, frm): `p` is the line offset of the event the kind names, `head` the residue
the line's first byte must have in device memory, `after` the byte right behind the line in the packed data (never part of the line),
`frm` the offset a search resumes at (resume cases only).  Kinds:
  run_stop      a quiet / steady run ends at p: byte p is the first that is not quiet (the run starts at 0, p-1, p-2, p-5, p-40)
  run_to_end    the value ends at L = p inside a run; NEEDY variants have the byte behind them in memory that would change the result
  stamp         a capture begins or ends at p; a one-byte field [p, p+1); an empty field at p
  dead          the value fails in byte p; the bytes behind it would match if walked
  absorb        the automaton reaches its final (.*) at p, with 300+ bytes behind
  search_start  (search patterns) the first byte a match can start with is at p: (a) a match follows, (b) a doomed start -- the second
                byte refuses it --, (c) a start byte that is the last byte of the value, (d) a start the look-behind refuses
  resume        (search patterns) the search resumes at frm = p-1, p, p+1; the next match begins at frm, frm+1 or in the next chunk
  threads       (NFA only) 8, exactly 6 (kNfaSteadyScanThreads) or 1 live steady threads in a run that ends at p
  miss          (lazy automata) byte p is the first on which the partial automaton has no transition: the kernel hands the value back
                and the thread-list kernels take it from its first byte; it matches, matches with 300 bytes behind p, does not match, or
                fails for want of the byte behind it
  overflow      (thread-list programs with a counted tail) the step on byte p leaves one thread more than a kernel of the chain holds
                (65: nfa_match_kernel hands the value to nfa_wide_kernel; 129: that one hands it to nfa_decide_kernel): the value
                matches, matches 300+ bytes behind p, ends with byte p, has one byte too many -- and `at_cap`, the control: one
                'a' fewer, the peak is EXACTLY the cap at p and nothing overflows
  absent        (run captures) the optional branch that holds the run group is not taken at p: the group reads (-1, -1)
Kinds of the atomic instantiation, nfa_match_kernel<ATOMIC> (its ordered commit pass nfaAtomicStep, lane 0; tests/test_chunk_edges.py
proves each event on byte p from the trace of tests/helpers/nfa_atomic_interp.py's faithful walk, for every head):
  alog          the log family's kinds under (?>([^,]*)),(?>([0-9]*));(?>([^ ]*)) (.*): the commit pass on every byte of fields 1 to 3,
                memberships alive across both chunk borders, the vector step and the skip from the last separator on
  commit        (acommit) an atomic group is left on byte p behind a run of 1, 2, 5, 40, 300 bytes: the value matches; fails only
                because the group gives no byte back; ends at p inside the group (the commit at the end of input decides, and the byte
                behind the value would change the result)
  enter         (acommit) the first byte that needs the commit pass is at p, behind a steady run from 0, p-1, p-2, p-5, p-40
  alt           (acommit) (?>(ab|a)) is left on byte p through its first branch; the second, closed by then, would have matched
  doomed        (aquasi: a kept atomic group AND doomed-spawn rows) a doomed spawn on byte p: skipped by its row, or -- p the last byte
                of a chunk or of the value -- stepped in full
  overflow      (akept64, avector64, alineage6, aclosed64, awork10) the step on byte p leaves through one named exit of the commit
                pass, or through the vector step's 65th thread inside the ATOMIC instantiation, and nfa_decide_kernel takes the value;
                the controls sit exactly at the cap on byte p: `at_cap` variants, or -- where the cap is the pattern's -- a sibling
                family (alineage6c, aclosed64c, awork10c) launched beside it
The `runcap` family gives run_stop and run_to_end to run_capture_kernel (gpu_runtime.hip): the run of a group written (?=(S*)) ends
on byte p / with the value at p, for every residue mod 16 of the value's first byte and runs of 0 to 40 bytes in front of p.
What a pattern cannot do is said by its family (Family.kinds: kind -> the smallest p it exists for).  tests/test_chunk_edges.py
asserts all of this against the oracle and against the compiled tables, so that the GPU test cannot pass on a degenerate corpus.
The atomic families rest on tests/helpers/nfa_atomic_interp.py: its faithful walk's trace says which step of the kernel falls on byte p.

pack(form, modulus): "len" = (off, len) with filler bytes between the lines that give every line its head (the filler would change
the answer if it were read); "sep" = off[n + 1] and one separator byte, where alignment follows from the lengths (the residues that
came out are returned, the tests assert that all occur).  Not part of the product, never imported by loongcollector_amd/."""
import functools
from collections import namedtuple

import numpy as np

from loongcollector_amd import binding as B

W256_P = tuple(range(0, 6)) + tuple(range(246, 263)) + tuple(range(502, 519))   # 6 below .. 6 behind the first two borders, any head
W16_P = tuple(range(0, 34))
W16R_P = W16_P + tuple(range(42, 58))                                           # ... and 16 offsets a run of 40 bytes fits in front of
WALKS = {"w256": (W256_P, 4), "w16": (W16_P, 16), "w16r": (W16R_P, 16)}         # walk -> (offsets, modulus of head)
RUN_BACK = (1, 2, 5, 40)                                                        # a run that ends at p starts at p - k (or at 0)
GUARD_BYTES = 64                                                                # zero bytes behind the packed data

Case = namedtuple("Case", "family kind variant p head line after frm")


def _cyc(alphabet, n, phase=0):
    return bytes(alphabet[(phase + i) % len(alphabet)] for i in range(n)) if n > 0 else b""


class Family:
    """A pattern and the lines that put each of its kinds on offset p.  cases(kind, p) -> [(variant, line, after, frm)];
    kinds: kind -> smallest p;  needy_min: smallest p at which run_to_end has a variant whose result the byte behind changes."""
    name = pattern = None
    flags = 0
    search = False
    kinds = {}
    needy_min = None
    filler = b"\n"            # between the lines of the (off, len) form: bytes that would change the answer if read
    after = b"\n"             # behind a line that names no byte of its own

    def cases(self, kind, p):
        return getattr(self, "k_" + kind)(p)


class LogFamily(Family):
    """a full-match log format that ends in (.*): [^x]* fields give quiet runs, the last separator the absorbing state"""
    name, pattern = "log", rb"([^,]*),(\d*);([^ ]*) (.*)"
    kinds = {"run_stop": 0, "run_to_end": 0, "stamp": 0, "dead": 1, "absorb": 3}
    needy_min = 2
    filler, after = b",7; ", b"7"
    TAIL = b" ok,1;z "

    def _line(self, c, s, t, L):
        """[^,]* bytes [0, c), a comma at c, digits, a semicolon at s, [^ ]* bytes, a space at t, anything up to L"""
        assert 0 <= c < s < t < L, (c, s, t, L)
        return _cyc(b"xyz-", c, c) + b"," + _cyc(b"0123456789", s - c - 1, s) + b";" + _cyc(b"uvw;", t - s - 1, t) + b" " + _cyc(self.TAIL, L - t - 1)

    def k_run_stop(self, p):
        out = [("f1_from0", self._line(p, p + 2, p + 4, p + 8), None, None)]
        for k in RUN_BACK:
            if p - k - 1 >= 0:
                out.append(("digits_%d" % k, self._line(p - k - 1, p, p + 3, p + 8), None, None))     # comma at p-k-1, digits [p-k, p), ';' at p
            if p - k - 2 >= 0:
                out.append(("f3_%d" % k, self._line(0, p - k - 1, p, p + 8), None, None))             # ';' at p-k-1, [^ ]* [p-k, p), ' ' at p
        return out

    def k_run_to_end(self, p):
        out = [("f1", _cyc(b"xyz-", p), b";", None)]                                                  # fails: no comma
        if p >= 1:
            out.append(("digits", b"," + _cyc(b"0123456789", p - 1), b";", None))
            out.append(("digits_f1", _cyc(b"xy", (p - 1) // 2) + b"," + _cyc(b"0123456789", p - 1 - (p - 1) // 2), b";", None))
        if p >= 2:
            out.append(("f3_needy", b",;" + _cyc(b"uvw", p - 2), b" ", None))                          # fails for want of the space behind it
        if p >= 4:
            out.append(("f3_needy_f1", _cyc(b"xy", (p - 2) // 2) + b",;" + _cyc(b"uvw;", p - 2 - (p - 2) // 2), b" ", None))
        return out

    def k_stamp(self, p):
        out = []
        if p >= 1:
            out += [("digits_begin", self._line(p - 1, p + 3, p + 5, p + 9), None, None),
                    ("digits_end", self._line(max(0, p - 3), p, p + 2, p + 6), None, None),
                    ("one_byte", self._line(p - 1, p + 1, p + 3, p + 7), None, None),
                    ("empty", self._line(p - 1, p, p + 2, p + 6), None, None)]
        else:
            out += [("one_byte", b"x,1;u t", None, None), ("empty", b",1;u t", None, None)]
        if p >= 2:
            out.append(("f3_end", self._line(0, max(1, p - 3), p, p + 5), None, None))
        if p >= 3:
            out.append(("rest_begin", self._line(0, 1, p - 1, p + 5), None, None))
            out.append(("rest_empty", self._line(0, 1, p - 1, p), None, None))                         # (.*) empty at p = L
        return out

    def k_dead(self, p):
        c = p - 1 if p < 4 else p - 3
        return [("digits", _cyc(b"xyz-", c, c) + b"," + _cyc(b"0123456789", p - c - 1) + b"Z" + b"7;u " + _cyc(self.TAIL, 5), None, None)]

    def k_absorb(self, p):
        c = max(0, p - 6)
        return [("space", self._line(c, c + 1 if p < 5 else p - 3, p - 1, p + 300 + p % 7), None, None)]


class BigFamily(LogFamily):
    """a tagged DFA of 8 000+ states: its tables stay in global memory, so tdfa_l2_kernel / tdfa_wave_kernel run by necessity"""
    name, pattern = "big", rb"([^,]*),(\d*);(?:a|b)*a(?:a|b){12}(c+)(d*) (.*)"
    filler, after = b",7;c ", b"c"
    AB = 13                                                                        # bytes of "a" + 12 of [ab]: the first c is AB + 2 behind a stretch that starts at 2
    kinds = {"run_stop": 0, "run_to_end": 0, "stamp": 0, "dead": 1, "absorb": AB + 4}
    needy_min = AB + 3

    def _big(self, c, s, m, k, j, L):
        """as _line up to the semicolon at s, then m bytes of [ab], "a" and AB - 1 of [ab], c's [u, u + k), d's, a space, anything up to L"""
        u = s + 1 + m + self.AB
        assert 0 <= c < s and k >= 1 and u + k + j < L, (c, s, m, k, j, L)
        return (_cyc(b"xyz-", c, c) + b"," + _cyc(b"0123456789", s - c - 1, s) + b";" + self._free(m) + self._tail(s) +
                b"c" * k + b"d" * j + b" " + _cyc(self.TAIL, L - u - k - j - 1))

    def _free(self, m):
        return _cyc(b"ab", m, m)

    def _tail(self, s):
        return b"a" + _cyc(b"bab", self.AB - 1, s)

    def k_run_stop(self, p):
        out = [("f1_from0", self._big(p, p + 2, 1, 2, 1, p + 30), None, None)]
        for k in RUN_BACK:
            if p - k - 1 >= 0:
                out.append(("digits_%d" % k, self._big(p - k - 1, p, 2, 1, 0, p + 26), None, None))
            if p - k - self.AB - 2 >= 0:
                out.append(("c_%d" % k, self._big(0, 1, p - k - self.AB - 2, k, 2, p + 9), None, None))   # c's [p-k, p), a 'd' at p
        return out

    def k_run_to_end(self, p):
        out = [("f1", _cyc(b"xyz-", p), b";", None)]
        if p >= 1:
            out.append(("digits", b"," + _cyc(b"0123456789", p - 1), b";", None))
        if p >= self.AB + 3:
            out.append(("c_needy", self._big(0, 1, 0, p - self.AB - 2, 0, p + 1)[:p], b" ", None))   # fails for want of the space behind it
        if p >= self.AB + 4:
            out.append(("d_needy", self._big(0, 1, 0, 1, p - self.AB - 3, p + 1)[:p], b" ", None))
        return out

    def k_stamp(self, p):
        out = []
        if p >= 1:
            out += [("digits_begin", self._big(p - 1, p + 3, 0, 1, 1, p + 24), None, None),
                    ("digits_end", self._big(max(0, p - 3), p, 1, 2, 0, p + 24), None, None),
                    ("one_byte", self._big(p - 1, p + 1, 0, 1, 0, p + 22), None, None),
                    ("empty", self._big(p - 1, p, 0, 1, 0, p + 22), None, None)]
        else:
            out += [("one_byte", self._big(1, 3, 0, 1, 0, 24), None, None), ("empty", self._big(0, 2, 0, 1, 0, 24), None, None)]
        if p >= self.AB + 2:
            out.append(("c_begin", self._big(0, 1, p - self.AB - 2, 3, 2, p + 9), None, None))
        if p >= self.AB + 3:
            out.append(("c_one_byte_d_empty", self._big(0, 1, p - self.AB - 3, 1, 0, p + 5), None, None))   # c+ = [p-1, p), d* empty at p
        if p >= self.AB + 5:
            out.append(("rest_empty", self._big(0, 1, p - self.AB - 5, 2, 0, p), None, None))   # the space is the value's last byte, behind a run
        return out

    def k_dead(self, p):
        c = p - 1 if p < 4 else p - 3
        out = [("digits", _cyc(b"xyz-", c, c) + b"," + _cyc(b"0123456789", p - c - 1) + b"Z7" + self._big(0, 1, 0, 1, 0, 22)[1:], None, None)]
        if p >= 3:
            out.append(("ab", b",;" + _cyc(b"ab", p - 2) + b"Z" + self._big(0, 1, 0, 1, 0, 22)[2:], None, None))
        return out

    def k_absorb(self, p):
        return [("space", self._big(0, 1, p - self.AB - 4, 1, 0, p + 300 + p % 7), None, None)]   # c at p-2, the space at p-1


class LazyFamily(BigFamily):
    """the big family with 14 in the place of 12: it does not determinise, so the handle is a thread-list program, and lazy_train
    builds a partial automaton along TRAINING lines (kept apart from the cases).  Behind an a/b stretch the automaton's state is the
    stretch's last AB bytes.  Every decided line's stretch is one fixed shape -- "abab..." from its first byte, then "aa" and a fixed
    rest --, so the windows the training lines walk are the alternating ones and those that hold the "aa".  A `miss` case alternates
    up to p - 2, where a 'b' stands, and has a second 'b' at p - 1: a window no training line has, on a value that may match all the
    same.  Byte p is the first the automaton has no transition for."""
    name, pattern = "lazy", rb"([^,]*),(\d*);(?:a|b)*a(?:a|b){14}(c+)(d*) (.*)"
    AB = 15
    kinds = {"run_stop": 0, "run_to_end": 0, "stamp": 0, "dead": 1, "absorb": AB + 4, "miss": AB + 2}
    needy_min = AB + 3
    REST = b"bbabbabbabbab"
    TRAIN_M = tuple(range(0, 2 * AB + 4)) + (600, 601)       # stretch lengths: every short one, and both parities of the long ones

    def _free(self, m):
        return _cyc(b"ab", m)

    def _tail(self, s):
        return b"aa" + self.REST

    def _alt_bb(self, p):
        """",;" and an alternating stretch [2, p - 1) whose last byte, at p - 2, is 'b'; then the second 'b' at p - 1.  The automaton
        has the state behind it (every state a training line enters gets all its transitions) but none of the transitions out of it:
        the walk leaves on byte p"""
        return b",;" + _cyc(b"ab", p - 3, (p - 1) % 2) + b"b"

    def k_miss(self, p):
        head = self._alt_bb(p)
        assert len(head) == p and head[p - 2:] == b"bb" and head[p - self.AB:p - self.AB + 1] == b"a"
        return [("last", head + b"cd " + _cyc(self.TAIL, 6), None, None),                             # byte p - 1 is the last of the stretch
                ("far", head + _cyc(b"ab", 300 + p % 5) + self._tail(0) + b"c " + _cyc(self.TAIL, 6), None, None),
                ("no_match", head + b"Z" + self._tail(0) + b"c t", None, None),
                ("needy", head + b"cc", b" ", None)]                                                  # fails for want of the space behind it

    def training(self):
        """the lines lazy_train gets: every shape a decided case has, at stretch lengths that span the offsets (a state behind AB or
        more stretch bytes depends on their parity alone), none of them a case"""
        out = []
        for m in self.TRAIN_M:
            for k, j in ((1, 0), (2, 1), (3, 2)):
                full = self._big(1, 3 + j, m, k, j, 3 + j + m + self.AB + k + j + 2 + 5 * k)
                out += [full, full[:full.index(b" ") + 1], full[:full.index(b" ")], full[:full.index(b" ") - j]]
            out.append(b"t,4;" + self._free(m) + b"Z" + self._tail(0) + b"c t")
            out.append(b",;" + self._free(m) + self._tail(0)[:m % self.AB] + b"Zc t")
            out.append(b"t,4;b" + self._free(m) + self._tail(0) + b"cd t")                             # (a stretch may begin with the 'b')
        out += [b"t,4Z;" + self._tail(0) + b"c t", b"xyz-xyz;", b"xy,0123;;"]
        return list(dict.fromkeys(out))


class SearchFamily(Family):
    """search patterns: junk the pattern cannot start in, then what the kind asks for at p"""
    search, flags = True, B.LC_SYNTAX_SEARCH
    kinds = {"search_start": 0, "resume": 0}
    JUNK = b"xyz -"
    HIT = DOOMED = START = None      # a match; a start byte and a byte that refuses it; the start byte alone
    BEHIND = None                    # (look-behind patterns) a byte in front of HIT that refuses the start
    filler = after = None            # set per family: the beginning of HIT / what completes a match

    def k_search_start(self, p):
        j = _cyc(self.JUNK, p, p)
        out = [("a_match", j + self.HIT + b" t", None, None), ("a_match_at_end", j + self.HIT, None, None),
               ("b_doomed", j + self.DOOMED + _cyc(self.JUNK, 2) + self.HIT + b" t", None, None),
               ("b_doomed_far", j + self.DOOMED + _cyc(self.JUNK, 300, p) + self.HIT, None, None),
               ("b_doomed_alone", j + self.DOOMED + _cyc(self.JUNK, 3), None, None),
               ("c_last_byte", j + self.START, None, None)]
        if self.BEHIND is not None and p >= 1:
            out.append(("d_behind", j[:-1] + self.BEHIND + self.HIT + b" " + self.HIT + b" t", None, None))
        return out

    def k_resume(self, p):
        out = []
        for frm in (p - 1, p, p + 1):
            if frm < 0:
                continue
            for name, gap in (("at_from", 0), ("at_from1", 1), ("next_chunk", 300)):
                line = self.HIT + b" " + _cyc(self.JUNK, max(0, frm + gap - len(self.HIT) - 1), frm)
                line = line[:frm + gap] + self.HIT + b" t" if len(line) >= frm + gap else None
                if line is not None:
                    out.append(("from%+d_%s" % (frm - p, name), line, None, frm))
        return out


class QuasiFamily(SearchFamily):
    """QUASI_PATTERNS[2] of tests/test_host_compilers.py: a doomed-spawn shape (a start byte most occurrences of which lead nowhere)"""
    name, pattern = "quasi", rb"Group = (.*), IP = (\d+), NAT"
    HIT, DOOMED, START = b"Group = ab, IP = 9, NAT", b"Gx", b"G"
    JUNK = b"xyz -,"
    filler, after = b"Group = ", b"T"

    def k_search_start(self, p):
        out = super().k_search_start(p)
        out.append(("needy", _cyc(self.JUNK, p, p) + self.HIT[:-1], b"T", None))                       # fails for want of the 'T' behind it
        return out


class LookFamily(SearchFamily):
    """a look-behind in front of the first byte: the class of byte p - 1 decides whether a match may begin at p"""
    name, pattern = "look", rb"(?<![0-9.])(\d+)\.(\d+)\.(\d+)\.(\d+)(?![0-9])"
    HIT, DOOMED, START, BEHIND = b"10.2.3.4", b"1x", b"1", b"."
    filler, after = b"9.", b"5"                                                                        # (a digit behind a line: the look-ahead would refuse)


class AtomicFamily(SearchFamily):
    """an atomic group: nfa_match_kernel<atomic>"""
    name, pattern = "atomic", rb"(?>[a-z]+)(\d\d)"
    JUNK = b"-_ ."
    HIT, DOOMED, START = b"ab12", b"a-", b"a"
    filler, after = b"q", b"3"

    def k_search_start(self, p):
        out = super().k_search_start(p)
        out.append(("needy", _cyc(self.JUNK, p, p) + b"ab1", b"2", None))                              # fails for want of the digit behind it
        return out


class ThreadsFamily(Family):
    """eight alternatives, each a self loop on the run's bytes: a digit k in front of the run kills alternative k, what is left are
    that many live threads, all steady, until the comma at p (NFA only: a DFA has one state whatever the count)"""
    name = "threads"
    pattern = b"(?:" + b"|".join(b"([^,%d]*)" % k for k in range(1, 9)) + b"),(.*)"
    kinds = {"threads": 0}
    filler, after = b",", b","
    LIVE = {8: b"", 7: b"1", 6: b"12", 5: b"123", 1: b"1234567"}

    def k_threads(self, p):
        out = []
        for live, kill in self.LIVE.items():
            if len(kill) <= p:
                out.append(("live%d" % live, kill + _cyc(b"xyz-", p - len(kill), p) + b"," + b"tail, 1", None, None))
                out.append(("live%d_to_end" % live, kill + _cyc(b"xyz-", p - len(kill), p), b",", None))   # L = p: fails, the comma is behind it
        return out


class BackrefFamily(Family):
    """a back-reference: only the backtracking engine runs it (bt_match_kernel reads bytes directly: no chunk, the same offsets)"""
    name, pattern = "backref", rb"(\w+),(\d*);\1 ?(.*)"
    kinds = {"stamp": 1, "dead": 2, "run_to_end": 3}
    needy_min = 3
    filler, after = b"a,;a", b"a"

    @staticmethod
    def _line(c, s, L):
        """a word of c bytes, a comma, digits, a semicolon at s, the word again, a space, anything up to L"""
        w = _cyc(b"abc_9", c, c)
        assert 1 <= c < s and s + 1 + c < L, (c, s, L)
        return w + b"," + _cyc(b"0123456789", s - c - 1) + b";" + w + b" " + _cyc(b"t ,;a", L - s - c - 2)

    def k_stamp(self, p):
        out = [("word_end", self._line(p, p + 2, 2 * p + 7), None, None)]
        if p >= 2:
            out += [("digits_end", self._line(max(1, p - 3), p, p + max(1, p - 3) + 6), None, None),
                    ("empty", self._line(p - 1, p, 2 * p + 4), None, None)]
        if p >= 5:
            c = (p - 3) // 2
            out.append(("rest_begin", self._line(c, p - c - 2, p + 4), None, None))                   # the space at p - 1
        return out

    def k_dead(self, p):
        c = max(1, p - 3)
        if c >= p:
            return []
        return [("digits", _cyc(b"abc_9", c, c) + b"," + _cyc(b"0123456789", p - c - 1) + b"Z" + b"7;" + _cyc(b"abc_9", c, c) + b" t", None, None)]

    def k_run_to_end(self, p):
        """the value ends one byte short of the word's second copy: that byte is behind it"""
        c = (p - 1) // 2
        d = p - 2 * c - 1                                   # digits: 0 or 1
        w = _cyc(b"abc_9", c, c)
        if c < 1:
            return []
        return [("needy", w + b"," + b"7" * d + b";" + w[:-1], w[-1:], None)]


def nested(body, depth):
    """`body` as a capture group nested `depth` deep: depth groups with one span"""
    return b"(" * depth + body + b")" * depth


class NestedLogFamily(LogFamily):
    """the log family with each of its four groups nested `depth` deep: the same lines, kinds and events, 4 * depth groups and
    8 * depth capture slots on the same 7 positions -- the thread-list kernels' NS = 64 / 128 / 320 instantiations at their exact fit"""

    def __init__(self, depth):
        self.depth, self.name = depth, "log%d" % (8 * depth)
        self.pattern = nested(rb"[^,]*", depth) + b"," + nested(rb"\d*", depth) + b";" + nested(rb"[^ ]*", depth) + b" " + nested(rb".*", depth)


class OverflowFamily(Family):
    """([^;]*);(.*)a(.{T}): behind the semicolon every 'a' leaves one more live thread -- the (.*) loop and one thread per 'a' in the
    counted tail -- so on "x..x;bbb" + m 'a's the step on the m-th 'a' leaves m + 1 threads.  m = cap: thread cap + 1 appears by the
    step on byte p (the run's last 'a'); m = cap - 1: the peak is exactly cap at p.  T > cap, so no thread has left the tail by then."""
    kinds = {}
    filler, after = b";ab", b"b"                                                  # (a 'b' behind a matching value: read, it would not match)
    HEAD = b";bbb"

    def __init__(self, name, tail, cap, depth=1, pattern=None):
        assert tail > cap
        self.name, self.tail, self.cap = name, tail, cap
        self.pattern = pattern or nested(rb"[^;]*", depth) + b";" + nested(rb".*", depth) + b"a" + nested(b".{%d}" % tail, depth)
        self.kinds = {"overflow": len(self.HEAD) + cap - 1}                       # the smallest p that leaves room for the run

    def _run(self, p, m):
        """"x..x;bbb" and m 'a's, the last of them at p"""
        x = p + 1 - m - len(self.HEAD)
        assert x >= 0, (p, m)
        return _cyc(b"xyz-", x, p) + self.HEAD + b"a" * m

    def k_overflow(self, p):
        out = []
        for tag, m in (("", self.cap), ("at_cap", self.cap - 1)):
            run, T = self._run(p, m), self.tail
            name = lambda v: (tag + "_" + v) if tag else v
            out += [(name("match"), run + _cyc(b"bc", T, p), None, None),
                    (name("far"), run + _cyc(b"bc", 300 + p % 7, p) + b"a" + _cyc(b"cb", T, p), None, None)]
            if not tag:
                out += [("ends", run, None, None), ("one_more", run + _cyc(b"bc", T + 1, p), None, None)]
        return out

    def overflows(self, case):
        return case.kind == "overflow" and not case.variant.startswith("at_cap")


class RunCaptureFamily(Family):
    """a run capture "(?=(S*))" inside an optional branch: the automata stamp where group 2 begins, run_capture_kernel walks the
    run -- bytes up to a 16-byte address, 16-byte loads, a tail -- and writes its end.  The set [^|] runs across the space that
    ends the next field, so the run ends on the first '|' or with the value, wherever the match's own events are."""
    name, pattern = "runcap", rb"([^,]*),(?:!(?=([^|]*)))?([^ ]*) (.*)"
    kinds = {"run_stop": 2, "run_to_end": 3, "absent": 1}
    needy_min = 3
    filler, after = b"u, ", b"u"                                                  # (behind a value: a byte of the run's set)
    BACK = (0, 1, 15, 16, 17, 40)

    def k_run_stop(self, p):
        """the first '|' at p, the run begins k bytes in front of it (the comma at p - k - 2, the '!' behind it)"""
        out = []
        for k in self.BACK:
            c = p - k - 2
            if c < 0:
                continue
            run = bytearray(_cyc(b"uvw_", k, p))
            if k >= 2:
                run[k // 2] = ord(" ")                                          # the field's end lies inside the run
            out.append(("back_%d" % k, _cyc(b"xyz-", c, c) + b",!" + bytes(run) + b"|" + (b"r|t" if k >= 2 else b"q r|t"), None, None))
        return out

    def k_run_to_end(self, p):
        """the value ends at p inside the run: the byte behind it belongs to the set"""
        out = [("needy_from2", b",!" + _cyc(b"uvw_", (p - 3) // 2, p) + b" " + _cyc(b"tuv ", p - 3 - (p - 3) // 2, p), b"u", None)]
        if p >= 4:
            out.append(("needy_short", _cyc(b"xyz-", p - 3, p) + b",! ", b"u", None))
        return out

    def k_absent(self, p):
        """no '!' at p, right behind the comma: the branch is not taken"""
        f1 = _cyc(b"xyz-", p - 1, p)
        out = [("plain", f1 + b",uv|w t|u", None, None), ("bang_later", f1 + b",u!v|w t|u", None, None)]
        if p >= 2:
            out.append(("bang_in_front", f1[:-1] + b"!,|uv t", None, None))                           # (a '!' in the first field)
        return out


# ---- nfa_match_kernel<ATOMIC>: the ordered commit pass (nfaAtomicStep) on chosen bytes, and each of its overflow exits

class AtomicLogFamily(LogFamily):
    """the log family's lines and kinds with its first three fields in atomic groups: 3 kept groups on the same 7 positions and
    8 slots, the same rows -- and the commit pass on every byte of fields 1 to 3, memberships alive across the chunk borders"""
    name, pattern = "alog", rb"(?>([^,]*)),(?>(\d*));(?>([^ ]*)) (.*)"


def _pre(n):
    """n >= 1 bytes of the two prefix fields of the acommit family: one comma, no semicolon"""
    assert n >= 1
    c = (n - 1) // 2
    return _cyc(b"xyz_", c, n) + b"," + _cyc(b"uvw ", n - 1 - c, n)


class AtomicCommitFamily(Family):
    """two prefix fields, one atomic group whose run [a-z]* crosses the borders, a byte of the group's own set (or '-'), an atomic
    alternation, a tail; everything behind the group is optional, so a value that ends inside the group matches by the commit at the
    end of input.  commit: the group is LEFT on byte p ('-', the first byte outside its set) behind a run of 1, 2, 5, 40, 300 bytes;
    `noback`: the run ends in "zad" / "zabd", which the plain form of the pattern would give back to match; `ends`: the value ends
    at p inside the group (the byte behind it, read, would refuse it).  enter: the group is ENTERED on byte p, behind a steady run
    of the second prefix field.  alt: (?>(ab|a)) is left on byte p through its first branch; `second_would`: only the second branch,
    which the commit closed, would have matched."""
    name, pattern = "acommit", rb"([^,]*),([^;]*);(?>([a-z]*))(?:(?:z|-)(?>(ab|a))(bc|d)(.*))?"
    PLAIN = rb"([^,]*),([^;]*);(?:([a-z]*))(?:(?:z|-)(?:(ab|a))(bc|d)(.*))?"
    kinds = {"commit": 3, "enter": 2, "alt": 6}
    filler, after = b",;a", b"-"
    RUNS = (1, 2, 5, 40, 300)

    def k_commit(self, p):
        out = []
        for k in self.RUNS:
            n = p - k - 1                                                       # prefix bytes in front of the semicolon
            if n < 1:
                continue
            head = _pre(n) + b";"
            out.append(("match_%d" % k, head + _cyc(b"abcdy", k, p) + b"-abd t", None, None))
            out.append(("ends_%d" % k, head + _cyc(b"abcdy", k, p), b"-", None))
            if k >= 5:          # (what the plain form gives back is "zabd" or "zad": no run of 1 or 2 bytes holds it)
                out.append(("noback_%d" % k, head + _cyc(b"abcdy", k - 4, p) + b"zabd" + b"- t", None, None))
        return out

    def k_enter(self, p):
        out = []
        for k in (0, 1, 4, 39):                                                 # the steady run of field 2: [p - 1 - k, p - 1)
            c = p - 2 - k
            if c >= 0:
                out.append(("from_%d" % (k + 1), _cyc(b"xyz_", c, p) + b"," + _cyc(b"uvw ", k, p) + b";" + b"abc-ad t", None, None))
        if p >= 3:
            out.append(("from0", b"," + _cyc(b"uvw ", p - 2, p) + b";" + b"abc-abd", None, None))
        return out

    def k_alt(self, p):
        head = _pre(p - 5) + b";" + b"q-"                                       # "ab" at [p - 2, p)
        return [("first", head + b"abd t", None, None), ("second_would", head + b"abc t", None, None),
                ("second", _pre(p - 4) + b";" + b"q-" + b"ad t", None, None), ("ends", head + b"ab", b"d", None)]


class AtomicQuasiFamily(Family):
    """a full-match pattern with a kept atomic group AND doomed-spawn rows: the lazy field's thread spawns on a space and the spawn
    is gone again unless an 'S' follows.  doomed: a space at p with no 'S' behind it -- skipped by the row, except where byte p + 1
    lies in the next chunk or behind the value, where the step is taken in full"""
    name, pattern = "aquasi", rb"(.*?) SA (?>([a-z]+)=)(\d+)"
    kinds = {"doomed": 0}
    filler, after = b" SA a=", b"7"
    JUNK, HIT = b"xyz-_,", b" SA ab=12"

    def k_doomed(self, p):
        j = _cyc(self.JUNK, p, p)
        return [("hit", j + self.HIT, None, None),                                                    # (not doomed: the 'S' follows)
                ("doomed", j + b" x" + _cyc(self.JUNK, 2) + self.HIT, None, None),
                ("doomed_S", j + b" Sx" + self.HIT, None, None),                                      # (the spawn lives one byte longer)
                ("doomed_far", j + b" x" + _cyc(self.JUNK, 300, p) + self.HIT, None, None),
                ("doomed_alone", j + b" x" + _cyc(self.JUNK, 3), None, None),
                ("last_byte", j + b" ", b"S", None)]


class LineageFamily(Family):
    """([^;]*); and (a+) inside d atomic groups, then (z+): the step on the first 'a', byte p, enters all d groups.  d = 7: one
    membership more than a thread carries (kNfaLineage); d = 6, the sibling: exactly 6 through the whole run of 'a's"""
    kinds = {"overflow": 1}
    filler, after = b";a", b"z"

    def __init__(self, name, depth, over):
        self.name, self.depth, self.over = name, depth, over
        self.pattern = rb"([^;]*);" + b"(?>" * depth + b"(a+)" + b")" * depth + b"(z+)"

    def _variants(self, head, p):
        tag = "" if self.over else "at_cap_"
        return [(tag + "match", head + b"az", None, None), (tag + "far", head + b"a" * (300 + p % 7) + b"z", None, None),
                (tag + "ends", head, None, None), (tag + "one_more", head + b"azq", None, None)]

    def k_overflow(self, p):
        return self._variants(_cyc(b"xyz-", p - 1, p) + b";a", p)

    def overflows(self, case):
        return self.over


class WorkFamily(LineageFamily):
    """five atomic groups around a+ and n nested optional ones behind it: the step on 'h', byte p, carries 5 memberships and enters
    and leaves n empty groups -- n = 6: the 11th work entry (kNfaLineageWork); n = 5, the sibling: exactly 10"""
    kinds = {"overflow": 2}
    filler, after = b";ah", b"z"

    def __init__(self, name, n, over):
        self.name, self.n, self.over = name, n, over
        opt = b"(?>" * n + b")".join(b"%c?" % c for c in b"bcdefg"[:n]) + b")"
        self.pattern = rb"([^;]*);(?>(?>(?>(?>(?>(a+" + opt + b"h))))))(z+)"

    def k_overflow(self, p):
        head = _cyc(b"xyz-", p - 2, p) + b";ah"
        tag = "" if self.over else "at_cap_"
        return [(tag + "match", head + b"z", None, None), (tag + "far", head + b"z" * (300 + p % 7), None, None),
                (tag + "ends", head, None, None), (tag + "one_more", head + b"zq", None, None)]


class ClosedFamily(LineageFamily):
    """n alternatives, each ([^,K]*) inside d atomic groups, then a comma: the step on the comma, byte p, closes n * d segments --
    22 x 3 = 66: the 65th closed segment of a step; 16 x 4, the sibling: exactly 64"""
    kinds = {"overflow": 1}
    filler, after = b";x,", b"t"

    def __init__(self, name, n, depth, over):
        self.name, self.n, self.depth, self.over = name, n, depth, over
        alts = b"|".join(b"(?>" * depth + b"([^,\\x%02x]*)" % (k + 1) + b")" * depth for k in range(n))
        self.pattern = rb"([^;]*);(?:" + alts + b"),(.*)"

    def k_overflow(self, p):
        """the semicolon at p - 1: byte p is the first behind it, and its step walks every alternative's way out, viable or not"""
        return self._variants(_cyc(b"uvw ", p - 1, p) + b";", p)

    def _variants(self, head, p):
        tag = "" if self.over else "at_cap_"
        return [(tag + "match", head + b",tail", None, None), (tag + "far", head + b"," + _cyc(b"tail ,;", 300 + p % 7), None, None),
                (tag + "ends", head + b",", None, None), (tag + "one_more", head + b"xy,t", None, None)]


_AKEPT = rb"([^;]*);(.*)a(?>(.{70}))"          # tail threads hold one membership each: every step a commit pass, the 65th survivor appended
_AVECTOR = rb"(?>([^;]*));(.*)a(.{70})"        # no membership left behind the semicolon: the vector step's 65th thread, in the ATOMIC instantiation
ATOMIC_EXITS = {"akept64": "kept64", "avector64": "vector64", "alineage6": "lineage6", "aclosed64": "closed64", "awork10": "work10"}
# the families whose cap belongs to the pattern, not the value: family -> its control, a sibling family launched beside it
SIBLING = {"alineage6": "alineage6c", "aclosed64": "aclosed64c", "awork10": "awork10c"}
AT_CAP = {"akept64": ("kept", 64), "avector64": ("kept", 64), "alineage6c": ("lineage", 6), "aclosed64c": ("closed", 64), "awork10c": ("work", 10)}


class BoundFamily(Family):
    """a pattern and a handful of explicit values (the two bound tests of the atomic instantiation): no kinds, no offsets"""
    kinds = {}

    def __init__(self, name, pattern, filler, after):
        self.name, self.pattern, self.filler, self.after = name, pattern, filler, after


def explicit_corpus(fam, lines):
    """the given lines as a Corpus of the 256-byte walk: line k at head k % 4"""
    return Corpus(fam, "w256", [Case(fam.name, "bound", "line%d" % k, 0, k % 4, line, None, None) for k, line in enumerate(lines)])


# nfa_match_kernel<ATOMIC> gives a value of L >= 2^17 - 2 bytes up before it looks at it (segment ids are (offset << 6 | thread) in 23 bits)
LENGTH_BOUND = (1 << 17) - 2
LENGTH_FAMILY = BoundFamily("alength", rb"([^;]*);(?>(\d+))(.*)", b";1", b"7")
LENGTH_TAIL = b";12 x"


def length_lines():
    """values of 2^17 - 3, 2^17 - 2 and 2^17 bytes -- a [^;] run and a short tail -- among short ones"""
    long = [_cyc(b"xyz-", L - len(LENGTH_TAIL), L) + LENGTH_TAIL for L in (LENGTH_BOUND - 1, LENGTH_BOUND, LENGTH_BOUND + 2)]
    short = [b"ab;7 t", b"nothing here", b";42", b"x;12", b"uvw;x1", b"", b"q;007 rest;1", b"x" * 300 + b";5 y"]
    return short[:3] + long[:1] + short[3:5] + long[1:2] + short[5:6] + long[2:] + short[6:]


# a lineage key has 8 bits for the group instance: 255 instances compile, the last one (index 254) is the top of them
INSTANCE_UNIT, INSTANCE_LAST = rb"(?>a+)a?,", rb"(?>(ab|a))(bc|;)"


def instance_pattern(n, plain=False):
    """n atomic group instances none of which the elision pass can drop, the last one an alternation that commits; plain: the same
    pattern with ordinary groups"""
    p = INSTANCE_UNIT * (n - 1) + INSTANCE_LAST
    return p.replace(b"(?>", b"(?:") if plain else p


INSTANCE_FAMILY = BoundFamily("ainstances", instance_pattern(255), b"a,", b"c")


def instance_lines():
    """(line, what): `commits` fails only because instance 254 gives nothing back"""
    head = b"aa," * 200 + b"a," * 54
    return [(head + b"ab;", "first"), (head + b"abc", "commits"), (head + b"abbc", "first_bc"), (head + b"a;", "second"),
            (head + b"ab", "short"), (head[3:] + b"ab;", "a unit short"), (b"a,ab;", "tiny")]


FAMILIES = {f.name: f for f in (LogFamily(), BigFamily(), LazyFamily(), QuasiFamily(), LookFamily(), AtomicFamily(), ThreadsFamily(), BackrefFamily(),
                                NestedLogFamily(8), NestedLogFamily(16), NestedLogFamily(40),
                                OverflowFamily("over64", 70, 64), OverflowFamily("over128", 140, 128), OverflowFamily("over64s", 70, 64, depth=11),
                                RunCaptureFamily(), AtomicLogFamily(), AtomicCommitFamily(), AtomicQuasiFamily(),
                                OverflowFamily("akept64", 70, 64, pattern=_AKEPT), OverflowFamily("avector64", 70, 64, pattern=_AVECTOR),
                                LineageFamily("alineage6", 7, True), LineageFamily("alineage6c", 6, False),
                                ClosedFamily("aclosed64", 22, 3, True), ClosedFamily("aclosed64c", 16, 4, False),
                                WorkFamily("awork10", 6, True), WorkFamily("awork10c", 5, False))}


class Corpus:
    def __init__(self, family, walk, cases):
        self.family, self.walk, self.cases = family, walk, cases
        self.lines = [c.line for c in cases]
        self.offsets, self.modulus = WALKS[walk]

    def label(self, i):
        c = self.cases[i]
        return "(%s, %s/%s, p=%d, head=%d%s), line %d of %d bytes" % (c.family, c.kind, c.variant, c.p, c.head,
                                                                      "" if c.frm is None else ", from=%d" % c.frm, i, len(c.line))

    def kinds_of(self, bad):
        """{kind: count} of the listed case indices: for failure messages"""
        out = {}
        for i in bad:
            out[self.cases[int(i)].kind] = out.get(self.cases[int(i)].kind, 0) + 1
        return out

    def frm(self):
        return np.array([c.frm or 0 for c in self.cases], np.uint32)

    def pack(self, form):
        """-> (data, off, len, residues).  "len": off[n], every line at an address = its head (mod the walk's modulus) when `data`
        itself is aligned, the line's `after` byte and filler between the lines; "sep": off[n + 1], one byte (`after`) behind each line.
        GUARD_BYTES zero bytes end the data, so that a walk that runs a piece too far still reads inside the allocation."""
        fam, M = self.family, self.modulus
        buf, off = bytearray(), []
        for k, c in enumerate(self.cases):
            if form == "len":
                buf += _cyc(fam.filler, (c.head - len(buf)) % M, k)
            off.append(len(buf))
            buf += c.line + (c.after or fam.after)
        length = np.array([len(c.line) for c in self.cases], np.uint32)
        off = np.array(off + ([len(buf)] if form == "sep" else []), np.uint32)
        data = np.frombuffer(bytes(buf) + b"\0" * GUARD_BYTES, np.uint8)
        return data, off, length, (off[:len(self.cases)] % M).astype(np.int64)


@functools.lru_cache(maxsize=None)
def generate(family, walk="w256"):
    """-> Corpus of FAMILIES[family] for the offsets and residues of `walk` (computed once per process: callers leave it unchanged).
    The order is shuffled (seeded), so that in the separator form the residues follow no pattern of the generator's loops."""
    fam = FAMILIES[family]
    offsets, M = WALKS[walk]
    cases = []
    for kind, min_p in fam.kinds.items():
        for p in offsets:
            if p < min_p:
                continue
            made = [m for m in fam.cases(kind, p) if m is not None]
            assert made, (family, kind, p)
            for head in range(M):
                for variant, line, after, frm in made:
                    cases.append(Case(family, kind, variant, p, head, line, after, frm))
    order = np.random.default_rng(20261018).permutation(len(cases))
    return Corpus(fam, walk, [cases[int(i)] for i in order])


# ---- dfa_screen_kernel (csrc/screen_kernel.hpp): one value per lane, 16-byte pieces from `address & ~15`, a yes/no walk that leaves on the
# sink ("a match is certain whatever follows"), and a list of the accepted values.  Every family but the back-reference gets a relaxed
# screen; the corpus is the w16 one.  A screen is a search, so it has no dead state: its walk ends on the sink or with the value.
SCREEN_FAMILIES = ("log", "big", "quasi", "look", "atomic", "threads")
SCREEN_BORDERS = (16, 32)                  # the first two piece borders of the aligned view


def compile_screen(family):
    fam = FAMILIES[family]
    scr = B.GpuRegex.compile_screen(fam.pattern, syntax_flags=fam.flags, relaxed=True, max_states=20000, max_table_bytes=2 << 20)
    assert scr is not None, family
    return scr


@functools.lru_cache(maxsize=None)
def screen_corpus(family):
    """the w16 corpus, and for the search families -- whose corpus the pattern finds something in nearly everywhere -- each value
    that ends with its match once more, cut one and two bytes short: kind `cut`, rejected, and the one-byte cut has the missing byte
    right behind it in memory"""
    base = generate(family, "w16")
    cuts = []
    for k in base.cases:
        if k.variant == "a_match_at_end":
            cuts.append(k._replace(kind="cut", variant="needy_1", line=k.line[:-1], after=k.line[-1:]))
            cuts.append(k._replace(kind="cut", variant="short_2", line=k.line[:-2], after=None))
    return Corpus(base.family, "w16", base.cases + cuts)


class ScreenWalk:
    """the screen's logical tables (tests/helpers/table_interp.py TdfaInterp reads the same) walked as dfa_screen_kernel walks its blob:
    the sink is the first accepting state every byte class keeps (regex_handle.cpp packScreenBlob)"""

    def __init__(self, it):
        self.cmap, self.start = it.cmap, it.start
        self.next = (it.trans & 0xFFFF).reshape(it.nstates, it.ncls)
        self.accept = it.final_id != 0xFFFF
        keeps = [st for st in range(1, it.nstates) if self.accept[st] and (self.next[st] == st).all()]
        self.sink = keeps[0] if keeps else None
        self.dead_transitions = int((self.next[1:] == 0).sum())

    def walk(self, line):
        """-> (accepted, "absorb" | "dead" | "end", the offset behind the last byte the walk looked at)"""
        state = self.start
        for i, b in enumerate(line):
            state = int(self.next[state, self.cmap[b]])
            if state == 0:
                return False, "dead", i + 1
            if state == self.sink:
                return True, "absorb", i + 1
        return bool(self.accept[state]), "end", len(line)


# ---- the instantiations the GPU test runs the corpus through: how the handle is compiled and launched, the families (with the walk
# whose offsets they take), and the kernel name lc_launched_kernels must report.  compile_engine / launch_engine: the engine= arguments;
# env: set before the pattern is compiled, kept for the launch; wave: the handle asks for the wave walk (prefer_wave_tdfa); dfs:
# lc_nfa_set_dfs(1) around the launch (restored to -1); min_n: the corpus is repeated until the batch has at least that many values.
# train: the handle is a thread-list program that gets a lazy automaton right after it is compiled (training_lines): "family" = the
# family's own training lines, so that its `miss` cases miss and are handed to the thread-list kernels; "corpus" = the first
# TRAIN_CORPUS lines of the corpus itself, which decide everything else (the decided path alone).
# A (row, kind) pair outside this table is not run: every row runs every kind its families declare.
Row = namedtuple("Row", "id kernel families walk compile_engine launch_engine env wave dfs min_n train", defaults=(None,))
_NFA, _TDFA = B.LC_ENGINE_NFA, B.LC_ENGINE_TDFA
_NOLAZY = {"LC_LAZY_TDFA": "0"}
ENV_KEYS = ("LC_LAZY_TDFA", "LC_NFA_WIDE_FIRST", "LC_TDFA_WAVE_MAX", "LC_BT_LANES")
UNSTAGED_ABOVE = 32768                     # gpu_runtime.hip launchTdfaL2Family: the register programs ride in LDS up to this many values
ROWS = [
    Row("nfa", "nfa_match_kernel", ("log", "quasi", "look", "threads"), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("nfa-atomic", "nfa_match_kernel<atomic>", ("atomic",), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("nfa-atomic-edges", "nfa_match_kernel<atomic>", ("alog", "acommit", "aquasi"), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("nfa-wide-first", "nfa_wide_kernel:first", ("log", "quasi", "look", "threads", "over64", "over128", "log64"), "w256", _NFA, _NFA,
        dict(_NOLAZY, LC_NFA_WIDE_FIRST="1"), False, False, 0),
    Row("wave-small-staged", "tdfa_l2_kernel:wave", ("log", "quasi", "look", "atomic"), "w256", B.LC_ENGINE_AUTO, _TDFA, {}, True, False, 0),
    Row("wave-large-staged", "tdfa_l2_kernel:wave", ("big",), "w256", B.LC_ENGINE_AUTO, _TDFA, {}, False, False, 0),
    # (a handle that ASKED for the wave walk gets it up to 16 384 values only: the unstaged launch needs the large automaton)
    Row("wave-unstaged", "tdfa_l2_kernel:wave", ("big",), "w256", B.LC_ENGINE_AUTO, _TDFA, {}, False, False, UNSTAGED_ABOVE + 1),
    Row("l2-lane", "tdfa_l2_kernel", ("big",), "w16", B.LC_ENGINE_AUTO, _TDFA, {"LC_TDFA_WAVE_MAX": "0"}, False, False, 0),
    Row("decide", "nfa_decide_kernel", ("log", "look"), "w256", _NFA, B.LC_ENGINE_DECIDE, _NOLAZY, False, False, 0),
    Row("dfs", "nfa_dfs_kernel", ("log", "quasi"), "w256", _NFA, _NFA, _NOLAZY, False, True, 0),
    Row("bt", "bt_match_kernel", ("backref",), "w256", B.LC_ENGINE_BT, B.LC_ENGINE_BT, {"LC_BT_LANES": "64"}, False, False, 0),
    Row("lazy-wave", "tdfa_l2_kernel:wave:lazy", ("lazy",), "w256", _NFA, _NFA, {}, False, False, 0, "family"),
    Row("lazy-lane", "tdfa_l2_kernel:lazy", ("lazy",), "w16", _NFA, _NFA, {"LC_TDFA_WAVE_MAX": "0"}, False, False, 0, "family"),
    Row("lazy-wave-decided", "tdfa_l2_kernel:wave:lazy", ("log", "threads"), "w256", _NFA, _NFA, {}, False, False, 0, "corpus"),
    Row("lazy-lane-decided", "tdfa_l2_kernel:lazy", ("log", "threads"), "w16", _NFA, _NFA, {"LC_TDFA_WAVE_MAX": "0"}, False, False, 0, "corpus"),
    # the hand-offs of the chain (CHAIN says which kernels a launch of these rows must and must not report)
    Row("chain64", "nfa_wide_kernel", ("over64",), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("chain128", "nfa_decide_kernel", ("over128",), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("chain-slots", "nfa_decide_kernel", ("over64s",), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    # the overflow exits of the atomic instantiation, one row each: nfa_decide_kernel takes what it gives up (no wide kernel runs
    # atomic programs); a family and its sibling control (SIBLING) share a row
    Row("achain-kept64", "nfa_match_kernel<atomic>", ("akept64",), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("achain-vector64", "nfa_match_kernel<atomic>", ("avector64",), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("achain-lineage6", "nfa_match_kernel<atomic>", ("alineage6", "alineage6c"), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("achain-closed64", "nfa_match_kernel<atomic>", ("aclosed64", "aclosed64c"), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("achain-work10", "nfa_match_kernel<atomic>", ("awork10", "awork10c"), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    # nfa_match_kernel<NS = 64 / 128 / 320> at their exact fit
    Row("nfa-ns64", "nfa_match_kernel", ("log64",), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("nfa-ns128", "nfa_match_kernel", ("log128",), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("nfa-ns320", "nfa_match_kernel", ("log320",), "w256", _NFA, _NFA, _NOLAZY, False, False, 0),
    # run_capture_kernel behind a thread-list program, the wave walk and the LDS tagged-DFA kernel (a name that ends in "*" is a prefix:
    # which tdfa_stream_kernel instantiation serves the automaton is the launch layer's business)
    Row("runcap-nfa", "nfa_match_kernel", ("runcap",), "w16r", _NFA, _NFA, _NOLAZY, False, False, 0),
    Row("runcap-wave", "tdfa_l2_kernel:wave", ("runcap",), "w16r", B.LC_ENGINE_AUTO, _TDFA, {}, True, False, 0),
    Row("runcap-lds", "tdfa_stream_kernel*", ("runcap",), "w16r", B.LC_ENGINE_AUTO, _TDFA, {}, False, False, 0),
]
# row id (, family) -> (names a launch must report, names it must not): the chain's hand-offs seen from outside.  chain64: 74 positions
# fit nfa_wide_kernel's 128 threads, so nothing can be left for the decide kernels and none is queued; chain-slots: 66 capture slots,
# nfa_wide_kernel<NS <= 64> does not apply and nfa_decide_kernel takes what nfa_match_kernel gives up
CHAIN = {
    ("chain64", "over64"): (("nfa_match_kernel", "nfa_wide_kernel"), ("nfa_wide_kernel:first", "nfa_decide_kernel")),
    ("chain128", "over128"): (("nfa_match_kernel", "nfa_wide_kernel", "nfa_decide_kernel"), ("nfa_wide_kernel:first",)),
    ("chain-slots", "over64s"): (("nfa_match_kernel", "nfa_decide_kernel"), ("nfa_wide_kernel", "nfa_wide_kernel:first")),
    ("nfa-wide-first", "over64"): (("nfa_wide_kernel:first",), ("nfa_match_kernel", "nfa_wide_kernel", "nfa_decide_kernel")),
    ("nfa-wide-first", "over128"): (("nfa_wide_kernel:first", "nfa_decide_kernel"), ("nfa_match_kernel", "nfa_wide_kernel")),
}
ACHAIN = [(r.id, f) for r in ROWS if r.id.startswith("achain-") for f in r.families]
CHAIN.update({k: (("nfa_match_kernel<atomic>", "nfa_decide_kernel"), ("nfa_wide_kernel", "nfa_wide_kernel:first", "nfa_match_kernel")) for k in ACHAIN})
# (row, family) whose launches leave values to nfa_decide_kernel: lc_decide_stats must count exactly the overflow variants of the launch
DECIDES = (("chain128", "over128"), ("chain-slots", "over64s"), ("nfa-wide-first", "over128")) + tuple(ACHAIN)
NS_ROWS = {"nfa-ns64": 64, "nfa-ns128": 128, "nfa-ns320": 320}                     # row -> the program's capture slots
TRAIN_CORPUS = 200
SEARCH_ROWS = [r for r in ROWS if any(FAMILIES[f].search for f in r.families)]
# test_result_edges: one family per kernel
EDGE_FAMILY = {"nfa": "log", "nfa-atomic": "atomic", "nfa-atomic-edges": "alog", "achain-kept64": "akept64", "achain-vector64": "avector64",
               "achain-lineage6": "alineage6", "achain-closed64": "aclosed64", "achain-work10": "awork10", "nfa-wide-first": "log", "wave-small-staged": "log", "wave-large-staged": "big",
               "wave-unstaged": "big", "l2-lane": "big", "decide": "log", "dfs": "log", "bt": "backref",
               "lazy-wave": "lazy", "lazy-lane": "lazy", "lazy-wave-decided": "log", "lazy-lane-decided": "threads",
               "chain64": "over64", "chain128": "over128", "chain-slots": "over64s", "nfa-ns64": "log64", "nfa-ns128": "log128",
               "nfa-ns320": "log320", "runcap-nfa": "runcap", "runcap-wave": "runcap", "runcap-lds": "runcap"}


def ran(row, names):
    """the instantiation the row names is among the kernels a launch reported"""
    if row.kernel.endswith("*"):
        return any(n.startswith(row.kernel[:-1]) for n in names)
    return row.kernel in names


def set_env(monkeypatch, row):
    """the environment of a row: set before the pattern is compiled, kept for the launch"""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)


def training_lines(row, family):
    """what a row with a lazy automaton hands to lazy_train, once"""
    return FAMILIES[family].training() if row.train == "family" else generate(family, row.walk).lines[:TRAIN_CORPUS]


def miss_lines(walk):
    """the lazy family's `miss` lines: handed to lazy_train a second time they REBUILD the handle's automaton between two launches"""
    return list(dict.fromkeys(k.line for k in generate("lazy", walk).cases if k.kind == "miss"))


def compile_row(row, family):
    """the handle of a (row, family) as the row says, under the environment set_env has set"""
    fam = FAMILIES[family]
    rx = B.GpuRegex(fam.pattern, syntax_flags=fam.flags, engine=row.compile_engine)
    if row.wave:
        assert rx.prefer_wave_tdfa(), (row.id, family)
    if row.train:
        assert rx.lazy_train(training_lines(row, family))["in_use"] == 1, (row.id, family)
    return rx
