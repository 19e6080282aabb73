"""Test-only: the cases of tests/test_decide_launch_model.py and tests/test_gpu_decide_launch.py -- the LAUNCH around the depth-first
decide walk (gpu_runtime.hip launchDecide; nfa_decide_kernel.hpp nfa_decide_plan_kernel and the worker loop of nfa_decide_kernel): which
workers get the memo, which walk without it under LC_DECIDE_BUDGET, which values find no room, which do not even fit the list.  Not part
of the product.

Two families of values whose walks have a closed form.

W = (.*)a(.{140})   142 positions, no atomic group: a frame is 20 bytes, the memo 71 bytes per frame.  The memo never shortens a walk of
                    this family (every (position, offset) pair is reached once), so the step count of a value is the same with and
                    without it -- what the memo costs here is room.  b x L takes 2L + 2 steps, every `a` with at least 141 bytes behind it
                    141 more, an `a` with 139 bytes behind it 140 more; an `a` with exactly 140 bytes behind it matches.
E = (a|aa)*b        4 positions: on a x n the walk takes 7n steps with the memo and Fibonacci-many without it (839 at n = 10, 15 123 at
                    n = 16, 103 678 at n = 20).

The planner's arithmetic is RESTATED here from the header's formulas (plan()); tests/test_decide_launch_model.py pins what it gives for
every launch below at 8 MiB and at 256 MiB, and the step counts written down below against the model of the walk
(tests/helpers/nfa_dfs_interp.py).  The status and capture rows of every DECIDED value come from OracleRegex, never from the model;
whether a value is decided follows from plan() and, for a walk without the memo, from its step count against the budget.
"""
from collections import namedtuple

import numpy as np

from loongcollector_amd import binding as B
from oracle.oracle import OracleRegex

# ---- the launch constants, restated (a change of the product's shows as a failing test, not as a test that follows it)
WORKERS = 128                 # nfa_decide_kernel.hpp kDecideWorkers
HEADER_BYTES = 256            # kDecideHeaderBytes
FRAME_WORDS = 5               # kDecideFrameWords
NODE_WORDS = 3                # kDecideNodeWords
BUDGET_NO_MEMO = 1 << 22      # kDecideBudgetNoMemo: what LC_DECIDE_BUDGET replaces
BUDGET_MEMO = 1 << 28         # kDecideBudgetMemo: no knob
POOL_DEFAULT = 256 << 20      # gpu_runtime.hip decidePoolBytes: LC_DECIDE_POOL_MB unset
POOL_SMALL = 8 << 20          # ... and its minimum, the child's LC_DECIDE_POOL_MB=8

W, E = rb"(.*)a(.{140})", rb"(a|aa)*b"
NPOS = {(W, 0): 142, (E, 0): 4, (W, B.LC_SYNTAX_SEARCH): 144}      # positions of the compiled programs (the search wrapper adds two)


def fixed_bytes(n_frames, closed_cap=0, max_enter=0):
    """decideFixedBytes: the frames and the node arena of a walk over n_frames offsets"""
    frame_words = FRAME_WORDS + closed_cap
    node_words = NODE_WORDS * max_enter
    return (n_frames * (frame_words + node_words) + node_words) * 4 + 64


def memo_bytes(n_frames, n_pos):
    """decideMemoBytes: a nibble per (position, offset)"""
    return ((n_frames * n_pos + 1) // 2 + 15) & ~15


def list_cap(pool, n_lines):
    """the list may take a quarter of the pool behind the header, four bytes a value"""
    return min((pool - HEADER_BYTES) // 4 // 4, n_lines)


Plan = namedtuple("Plan", "branch count dropped workers slice walks")


def plan(pool, frames, n_pos, closed_cap=0, max_enter=0):
    """nfa_decide_plan_kernel and the worker loop's own tests, for a launch that lists values of `frames` = L - from + 1 offsets each.
    -> Plan: branch = which of the planner's outcomes ("memo for all", "fewer workers", "no memo", "one worker"), with " + list full"
    behind it when values were dropped; count = listed values; dropped = values the list had no room for (LC_GAVE_UP, which ones is a
    race); workers, slice; walks = per value "memo" / "plain" / "no room" (LC_GAVE_UP) -- for the values in their order when none was
    dropped, else for a value of the largest and every other size only by size (walk_of)."""
    cap = list_cap(pool, len(frames))
    count = min(len(frames), cap)
    dropped = len(frames) - count
    if count == 0:
        return Plan("nothing listed", 0, dropped, 0, 0, [])
    slices_at = HEADER_BYTES + ((count * 4 + 255) & ~255)
    avail = pool - slices_at
    longest = max(frames)
    fixed = fixed_bytes(longest, closed_cap, max_enter)
    with_memo = fixed + memo_bytes(longest, n_pos)
    workers = min(count, WORKERS)
    branch = "memo for all"
    if with_memo * workers > avail:
        fit = avail // with_memo
        if fit >= 1:
            workers, branch = min(fit, workers), "fewer workers"
        elif avail // fixed >= 1:
            workers, branch = min(avail // fixed, workers), "no memo"
        else:
            workers, branch = 1, "one worker"          # (never 0 workers: that gave up every value of the launch)
    slice_bytes = (avail // workers) & ~255
    assert slices_at + workers * slice_bytes <= pool
    walks = [walk_of(slice_bytes, f, n_pos, closed_cap, max_enter) for f in frames]
    return Plan(branch + (" + list full" if dropped else ""), count, dropped, workers, slice_bytes, walks)


def walk_of(slice_bytes, n_frames, n_pos, closed_cap=0, max_enter=0):
    """the worker loop's per-value tests"""
    fixed = fixed_bytes(n_frames, closed_cap, max_enter)
    if fixed > slice_bytes:
        return "no room"
    return "memo" if fixed + memo_bytes(n_frames, n_pos) <= slice_bytes else "plain"


# ---- the values
def w_fail(L, a_at=None):
    """b x L, with an `a` at offset a_at"""
    s = bytearray(b"b" * L)
    if a_at is not None:
        s[a_at] = ord("a")
    return bytes(s)


def w_match(L, fill=b"c"):
    """an `a` with exactly 140 bytes behind it: group 1 = [0, L - 141], group 2 = [L - 140, L]"""
    return b"b" * (L - 141) + b"a" + fill * 140


def w_over(L, n_a=130, match=False):
    """n_a >= 128 `a` in front: more live threads than nfa_wide_kernel holds -- the thread-list chain leaves the value LC_OVERFLOW"""
    tail = L - n_a
    return b"a" * n_a + (b"b" * (tail - 141) + b"a" + b"c" * 140 if match else b"b" * tail)


LONG = 100000
W_S = w_fail(LONG, LONG - 140)          # the `a` 139 bytes before the end: 2L + 142 steps
W_S1 = w_fail(LONG, LONG - 142)         # ... 141 bytes before the end: 2L + 143
W_LONG_MATCH = w_match(LONG)
S = 2 * LONG + 142
SHORT_W = [w_match(341), w_fail(300), w_fail(500, 17), w_match(141), b"", w_fail(1, 0)]
SHORT_E_UNDER_W = [b"a" * n for n in (12, 14, 16, 18, 20)]
HUGE = 450000                           # 450 001 frames of 20 bytes: 9 MB, more than the whole small pool

# plain (memo-less) step counts of the values that walk without the memo somewhere below: (pattern, flags, value, from) -> steps, each
# asserted against the model by tests/test_decide_launch_model.py
G_LONG = [w_over(LONG - 1, match=True), w_over(LONG, match=True), w_over(LONG + 1, match=True), w_over(40000)]
SEARCH_VALUE = w_fail(LONG, LONG - 200)
PLAIN_STEPS = [
    (W, 0, W_S, 0, S),
    (W, 0, W_S1, 0, S + 1),
    (W, 0, W_LONG_MATCH, 0, LONG + 284),
    (W, B.LC_SYNTAX_SEARCH, SEARCH_VALUE, 0, 100403),
    (W, 0, G_LONG[0], 0, LONG + 283),
    (W, 0, G_LONG[1], 0, LONG + 284),
    (W, 0, G_LONG[2], 0, LONG + 285),
    (W, 0, G_LONG[3], 0, 2 * 40000 + 2 + 130 * 141),
]
# (The real bound is not among the launches: b x 100 027 behind 28 328 `a` takes 2L + 2 + 141 k = 2^22 steps, and such a walk was measured
# at 5.4 s on the device -- too long for a suite that every change runs.  Run once: decided at 2^22 steps, LC_GAVE_UP at 2^22 + 1.)
G_BUDGET = LONG + 283                   # G_LONG[0] is decided with its last step; G_LONG[1] and [2] give up; G_LONG[3] takes 98 332


def plain_steps(pattern, flags, value, frm):
    for p, f, v, fr, steps in PLAIN_STEPS:
        if (p, f, fr) == (pattern, flags, frm) and v == value:
            return steps
    raise KeyError("no step count written down for a value of %d bytes that walks without the memo" % len(value))


Launch = namedtuple("Launch", "name pattern flags values frm budget")


def e_values(n):
    vals = (b"a", b"b")
    return [vals[(i * 7 // 3) % 2] for i in range(n)]


LIST_CAP_SMALL = 524272                 # (8 * 2^20 - 256) / 16


def launches():
    """-> {name: Launch}: the launches of the child (8 MiB pool); the parent reruns a, b and c-long with the budget unset"""
    mixed_4k = [(w_match(4096), w_fail(4096), w_fail(4096, 4096 - 140), w_fail(4096, 4096 - 142), w_match(4096, b"a"))[i % 5] for i in range(128)]
    c_values = [W_S, SHORT_W[0], W_S1, SHORT_W[1], W_LONG_MATCH, SHORT_W[2]]
    out = [
        Launch("a", E, 0, [b"a" * (12 + i % 9) for i in range(200)], None, 1000),
        Launch("b", W, 0, mixed_4k, None, 1000),
        Launch("c, budget S", W, 0, c_values, None, S),
        Launch("c, budget S + 1", W, 0, c_values, None, S + 1),
        Launch("c, budget unset", W, 0, c_values, None, None),
        Launch("d, from L - 60", W, B.LC_SYNTAX_SEARCH, [SEARCH_VALUE], [LONG - 60], 1000),
        Launch("d, from 0", W, B.LC_SYNTAX_SEARCH, [SEARCH_VALUE], [0], 1000),
        Launch("e", W, 0, SHORT_W[:3] + [w_fail(HUGE)] + SHORT_W[3:5] + SHORT_E_UNDER_W, None, 1000),
        Launch("f, list + 5", E, 0, e_values(LIST_CAP_SMALL + 5), None, 1000),
        Launch("f, list", E, 0, e_values(LIST_CAP_SMALL), None, 1000),
        Launch("c-long", W, 0, [W_S, W_S1, W_LONG_MATCH], None, None),
    ]
    return {x.name: x for x in out}


def frames_of(launch):
    frm = launch.frm or [0] * len(launch.values)
    return [len(v) - min(f, len(v)) + 1 for v, f in zip(launch.values, frm)]


def plan_of(launch, pool):
    return plan(pool, frames_of(launch), NPOS[(launch.pattern, launch.flags)])


_oracles = {}


def oracle_rows(pattern, flags, values, frm=None):
    """-> (caps[n, 2G], status[n]) as a match launch writes them for decided values: the oracle's, once per distinct (value, from)"""
    if pattern not in _oracles:
        _oracles[pattern] = OracleRegex(pattern)
    o = _oracles[pattern]
    search = bool(flags & B.LC_SYNTAX_SEARCH)
    G = o.groups + (1 if search else 0)
    caps = np.full((len(values), 2 * G), -1, np.int32)
    status = np.zeros(len(values), np.uint8)
    seen = {}
    for i, s in enumerate(values):
        f = 0 if frm is None else int(frm[i])
        if (s, f) not in seen:
            r = o.search(s, f) if search else o.fullmatch(s)
            seen[(s, f)] = None if r is None else [v for be in (r if search else r[1:]) for v in be]
        if seen[(s, f)] is not None:
            caps[i] = seen[(s, f)]
            status[i] = B.LC_MATCH
    return caps, status


def expected(launch, pool, budget="its own"):
    """-> (caps, status, (listed, given up), Plan): the oracle's rows, with LC_GAVE_UP and a row of -1 for every value that finds no
    room, or walks without the memo and takes more steps than the budget.  Values the LIST has no room for are not marked (which ones
    is a race): stats counts them, and the caller allows exactly Plan.dropped rows to read LC_GAVE_UP instead."""
    budget = launch.budget if budget == "its own" else budget
    budget = BUDGET_NO_MEMO if budget is None else budget
    pl = plan_of(launch, pool)
    caps, status = oracle_rows(launch.pattern, launch.flags, launch.values, launch.frm)
    gave_up = 0
    for i, walk in enumerate(pl.walks):
        f = launch.frm[i] if launch.frm else 0
        if walk == "no room" or (walk == "plain" and plain_steps(launch.pattern, launch.flags, launch.values[i], f) > budget):
            caps[i], status[i] = -1, B.LC_GAVE_UP
            gave_up += 1
    if pl.dropped:
        assert gave_up == 0       # (with a full list the workers take the first `count` of a race: only by-size statements hold)
    return caps, status, (pl.count, gave_up + pl.dropped), pl


def pack(values):
    """-> (data u8[] with 16 bytes of padding, off u32[n], len u32[n])"""
    length = np.array([len(v) for v in values], np.uint32)
    off = np.zeros(len(values), np.uint32)
    off[1:] = np.cumsum(length[:-1])
    return np.frombuffer(b"".join(values) + b"\0" * 16, np.uint8), off, length
