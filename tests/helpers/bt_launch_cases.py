"""Test-only: the cases of tests/test_bt_launch_model.py and tests/test_gpu_bt_launch.py -- a family of patterns and values whose need of
backtracking STACK is a closed form, so that a value can be put on either side of every threshold of the backtracking engine's launch layer
(gpu_runtime.hip launchBt, bt_kernel.hpp bt_match_kernel): the 2048-word slice of pass 1, the 16384-word slice of pass 2, the rule that
hands every lane the large slice, the refusal, the 48 KiB stage.  Not part of the product.

The family.  P(m) = (?:(a)|b)*\\1(?:z + (?:x*)* x m + )?     V(k) = "ab" x k + "a" (matches, group 1 = [2k-2, 2k-1])
                                                             N(k) = "ab" x k + "c" (does not match)
The m loops sit behind a `z` no value holds: each costs one loop register and 80 bytes of program, none runs.  The walk keeps an
alternative and an undo record per byte, so (measured with the host build of btRun, tests/test_bt_launch_model.py asserts it)

    min_words(V(k)) = max(10 k + 16, 32) + BT_NCAPS + BT_NLOOP          min_words(N(k)) = max(10 k + 8, 32) + BT_NCAPS + BT_NLOOP

(the floor of 32: btRun refuses a slice with fewer than 32 words of stack, bt_vm.hpp:92).  R(q) is the same pattern with (?:)* for the
loop: four instructions per loop register instead of five, so that 16 316 registers fit the 65 536 instructions of a program
(bt_program.cpp:15) -- the only way to the refusal's threshold.

The REFERENCE of every decided value is OracleRegex cross-checked against CPython's re on the same bytes (reference()).  Whether a value
IS decided is a condition, not a reference: min_words / min_budget bisect on the host build of the routine the kernel runs per lane.
"""
import ctypes
import os
import re
import subprocess

import numpy as np

from loongcollector_amd import binding as B
from oracle.oracle import OracleRegex

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# ---- the launch constants, restated (a change of the product's shows as a failing test, not as a test that follows it)
SLICE_WORDS = 2048           # bt_kernel.hpp:22  kBtSliceWords: a lane's scratch in pass 1
RETRY_SLICE_WORDS = 16384    # bt_kernel.hpp:23  kBtRetrySliceWords: in pass 2, and in pass 1 under the large-slice rule
BLOCK_LANES = 64             # bt_kernel.hpp:16  kBtBlock
STAGE_BYTES = 48 * 1024      # bt_kernel.hpp:26  kBtStageMaxBytes: larger programs are walked from global memory
DEFAULT_BUDGET = 1 << 22     # bt_kernel.hpp:30  kBtDefaultBudget
POOL_ABOVE_BYTES = 64 << 20  # gpu_runtime.hip:1124  kBtCachedWordsMax (64 MB): larger scratch comes from the stream-ordered pool
MAX_INSTRUCTIONS = 65536     # bt_program.cpp:15  kBtMaxInstructions
MIN_STACK_WORDS = 32         # bt_vm.hpp:92


def need(ncaps, nloop):
    """gpu_runtime.hip:1148"""
    return ncaps + nloop + 64


def takes_large_slice(ncaps, nloop):
    """gpu_runtime.hip:1150: every lane gets the large slice from the start (and there is no second pass)"""
    return need(ncaps, nloop) + 128 > SLICE_WORDS


def refused(ncaps, nloop):
    """gpu_runtime.hip:1152"""
    return need(ncaps, nloop) > RETRY_SLICE_WORDS


def blocks(n, lanes=131072):
    """-> (blocks of pass 1, blocks of pass 2)   gpu_runtime.hip:1143-1145"""
    first = min((n + BLOCK_LANES - 1) // BLOCK_LANES, lanes // BLOCK_LANES)
    return first, max(1, min(first // 8, 8192 // BLOCK_LANES))


def scratch_bytes(n, lanes=131072):
    """the scratch of a two-pass launch of n values   gpu_runtime.hip:1179"""
    first, retry = blocks(n, lanes)
    return 4 * (64 + max(first * BLOCK_LANES * SLICE_WORDS, retry * BLOCK_LANES * RETRY_SLICE_WORDS))


# ---- the family
LOOP_X, LOOP_EMPTY = b"(?:x*)*", b"(?:)*"
LOOP_BYTES = {LOOP_X: 80, LOOP_EMPTY: 64}     # program bytes per loop: five / four instructions of 16 bytes
HEAD = b"(?:(a)|b)*\\1"
NCAPS, NCAPS_SEARCH = 4, 6                    # 2 x (groups + 1); a search's group 1 is the whole match


def P(m, loop=LOOP_X):
    return HEAD + b"(?:z" + loop * m + b")?"


def R(q):
    return P(q, LOOP_EMPTY)


def V(k):
    return b"ab" * k + b"a"


def N(k):
    return b"ab" * k + b"c"


def program_bytes(m, loop=LOOP_X):
    """the size of P(m)'s program: a header of 32 bytes, three byte classes of 32 (a, b, z; x is the fourth), 14 instructions of 16 and
    five (x*: REPSET inside the loop) or four per loop (asserted by tests/test_bt_launch_model.py for every m in use)"""
    if m == 0:
        return 352
    return (464 if loop == LOOP_X else 416) + (m - 1) * LOOP_BYTES[loop]


def closed_form(value, ncaps, nloop):
    """min_words of V(k) / N(k)"""
    k, last = (len(value) - 1) // 2, value[-1:]
    assert value == b"ab" * k + last and last in (b"a", b"c")
    return max(10 * k + (16 if last == b"a" else 8), MIN_STACK_WORDS) + ncaps + nloop


_compiled = {}


def compiled(pattern, flags=0):
    """-> (GpuRegex, its backtracking program): one handle per (pattern, flags), shared by every test"""
    key = (pattern, flags)
    if key not in _compiled:
        rx = B.GpuRegex(pattern, syntax_flags=flags)
        assert rx.info()["engine"] == B.LC_ENGINE_BT
        _compiled[key] = (rx, rx.table(B.LC_TABLE_BT_BLOB, np.uint32))
    return _compiled[key]


# ---- the host build of btRun (the library of tests/test_backref.py's host_vm fixture)
_host = None


def host_lib():
    global _host
    if _host is None:
        out_dir = os.path.join(ROOT, "tests", "_build")
        os.makedirs(out_dir, exist_ok=True)
        src = os.path.join(ROOT, "tests", "native", "bt_host_check.cpp")
        hdr = os.path.join(ROOT, "loongcollector_amd", "csrc", "bt_vm.hpp")
        lib = os.path.join(out_dir, "libbt_host_check.so")
        if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, src])
        L = ctypes.CDLL(lib)
        L.bt_host_run.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                  ctypes.c_uint32, ctypes.c_uint32]
        L.bt_host_run.restype = ctypes.c_int
        _host = L
    return _host


def host_walk(blob, s, words, budget=DEFAULT_BUDGET, frm=0):
    """btRun on the host -> 1 match, 0 no match, -1 out of steps, -2 out of stack"""
    caps = np.full(int(blob[2]), -9, np.int32)
    return host_lib().bt_host_run(blob.ctypes.data, s, len(s), frm, caps.ctypes.data, len(caps), words, budget)


_min_words, _min_budget = {}, {}


def min_words(pattern, s, flags=0, frm=0):
    """the smallest slice with which the walk decides s (every smaller one ends out of stack)"""
    key = (pattern, flags, s, frm)
    if key not in _min_words:
        blob = compiled(pattern, flags)[1]
        lo, hi = 0, 1 << 21
        assert host_walk(blob, s, hi, frm=frm) in (0, 1)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if host_walk(blob, s, mid, frm=frm) in (0, 1):
                hi = mid
            else:
                lo = mid
        _min_words[key] = hi
    return _min_words[key]


def min_budget(pattern, s, words, flags=0, frm=0):
    """the smallest budget with which the walk of s, on a slice of `words` that decides it, does not run out of steps"""
    key = (pattern, flags, s, frm, words)
    if key not in _min_budget:
        blob = compiled(pattern, flags)[1]
        lo, hi = 0, DEFAULT_BUDGET
        assert host_walk(blob, s, words, hi, frm) in (0, 1)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if host_walk(blob, s, words, mid, frm) == -1:
                lo = mid
            else:
                hi = mid
        _min_budget[key] = hi
    return _min_budget[key]


# ---- the reference
_reference = {}


def reference(pattern, s, search=False, frm=0):
    """-> the capture row a match launch writes for s (a full match: groups 1..; a search: the whole match, then groups 1..), or None:
    OracleRegex and CPython's re on the same bytes, which must agree"""
    key = (pattern, s, search, frm)
    if key not in _reference:
        if pattern not in _reference:
            _reference[pattern] = (OracleRegex(pattern), re.compile(pattern))
        o, py = _reference[pattern]
        got = o.search(s, frm) if search else o.fullmatch(s)
        m = py.search(s, frm) if search else py.fullmatch(s)
        want = None if m is None else [m.span(g) for g in range(py.groups + 1)]
        assert got == want, ("the oracle and re differ", pattern[:40], len(pattern), s[:20], len(s), got, want)
        _reference[key] = None if got is None else [v for be in (got if search else got[1:]) for v in be]
    return _reference[key]


def expected(pattern, values, slice_words=RETRY_SLICE_WORDS, budget=DEFAULT_BUDGET, flags=0, frm=None):
    """-> (caps[n, 2G], status[n]) of a match launch over `values` whose undecided values end on a slice of `slice_words` (the large
    one: pass 2, or pass 1 under the large-slice rule).  A value is decided iff min_words <= that slice and min_budget <= budget; a
    decided value has the reference's status and captures; any other is LC_GAVE_UP with every capture -1.  Plain rules: nothing of
    the launch is modelled but its FINAL slice and its budget (which is fresh in each pass)."""
    search = bool(flags & B.LC_SYNTAX_SEARCH)
    G = compiled(pattern, flags)[0].groups
    caps = np.full((len(values), 2 * G), -1, np.int32)
    status = np.zeros(len(values), np.uint8)
    for i, s in enumerate(values):
        f = 0 if frm is None else min(int(frm[i]), len(s))
        if min_words(pattern, s, flags, f) > slice_words or min_budget(pattern, s, slice_words, flags, f) > budget:
            status[i] = B.LC_GAVE_UP
            continue
        row = reference(pattern, s, search, f)
        if row is not None:
            caps[i] = row
            status[i] = B.LC_MATCH
    return caps, status


def pack(values, form):
    """-> (data u8[], off u32[], len u32[] or None, sep): "len": offsets + lengths, the values back to back; "sep": n + 1 offsets and a
    one-byte separator behind every value"""
    sep = 0 if form == "len" else 1
    length = np.array([len(v) for v in values], np.uint32)
    off = np.zeros(len(values) + 1, np.uint32)
    off[1:] = np.cumsum(length + sep)
    data = np.frombuffer((b"\n" if sep else b"").join(list(values) + [b""]) + b"\0" * 16, np.uint8)
    return data, (off[:-1] if form == "len" else off), (length if form == "len" else None), sep


def largest_staged_m():
    """the largest m whose program is walked from LDS (<= 48 KiB), by search over the compiled programs"""
    lo, hi = 0, 4096       # (P(0) fits, P(4096) does not)
    assert 4 * len(compiled(P(lo))[1]) <= STAGE_BYTES < 4 * len(compiled(P(hi))[1])
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if 4 * len(compiled(P(mid))[1]) <= STAGE_BYTES:
            lo = mid
        else:
            hi = mid
    return lo


# ---- the (pattern, k) pairs of the GPU tests: tests/test_bt_launch_model.py checks the conditions they rest on for exactly these
def edge_ks(nregs):
    """k around both slice caps for a pattern with nregs = BT_NCAPS + BT_NLOOP: the last V(k) a 2048-word slice decides with its
    neighbours, the same for 16384 words, and k = 1 (for nregs = 4: 1, 201..204, 1635..1638)"""
    ks = {1}
    for words in (SLICE_WORDS, RETRY_SLICE_WORDS):
        last = (words - 16 - nregs) // 10
        ks.update(k for k in (last - 1, last, last + 1, last + 2) if k >= 1)
    return sorted(ks)


def values_of(ks):
    return [f(k) for k in ks for f in (V, N)]


M_SMALL_SLICE_LAST = 1852    # BT_NCAPS + BT_NLOOP = 1856: need + 128 = 2048, the last program on the small slice (96 stack entries)
M_LARGE_SLICE = 1900
Q_ACCEPTED_LAST = 16316      # BT_NCAPS + BT_NLOOP = 16320: need = 16384, the last program a launch accepts (32 stack entries)
SHORT_KS = (1, 2, 3)
PENDING_K, GAVE_UP_K = 203, 1637   # with P(0): the first value left to pass 2, the first neither pass decides
BUDGET_KS = (50, 203)


def gpu_cases():
    """-> [(pattern, flags, BT_NLOOP, [k, ...])]: every program and every k the GPU tests launch"""
    staged = largest_staged_m()
    out = [(P(0), 0, 0, sorted(set(edge_ks(NCAPS)) | set(SHORT_KS) | set(BUDGET_KS) | {5, PENDING_K, GAVE_UP_K}))]
    for m in (staged, staged + 1, 700, M_SMALL_SLICE_LAST, M_SMALL_SLICE_LAST + 1, M_LARGE_SLICE):
        out.append((P(m), 0, m, edge_ks(NCAPS + m)))
    out.append((R(Q_ACCEPTED_LAST), 0, Q_ACCEPTED_LAST, [1, 2, 3, 4, 5, 6]))
    return out
