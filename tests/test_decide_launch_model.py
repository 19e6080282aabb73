"""The conditions tests/test_gpu_decide_launch.py rests on, checked without a GPU (tests/helpers/decide_launch_cases.py): the step
counts of the two families from the model of the walk (tests/helpers/nfa_dfs_interp.py counts self.steps where decideLine counts
`steps`), the planner's arithmetic restated from the header's formulas, and the branch it takes for every launch at 8 MiB and at
256 MiB.  A compiler change that moves a position count or a step count fails here, not on the device."""
import numpy as np
import pytest

from loongcollector_amd import binding as B
from tests.helpers import decide_launch_cases as dl
from tests.helpers.nfa_dfs_interp import DfsNfaInterp


@pytest.fixture(scope="module")
def interp():
    made = {}

    def get(pattern, flags=0):
        if (pattern, flags) not in made:
            rx = B.GpuRegex(pattern, syntax_flags=flags, engine=B.LC_ENGINE_NFA)
            made[(pattern, flags)] = (rx, DfsNfaInterp(rx))
        return made[(pattern, flags)]
    return get


def steps(it, s, memo, frm=0, budget=None):
    r = it.fullmatch(s, frm, memo=memo, budget=budget)
    return it.steps, r


def test_the_programs_have_the_positions_the_helper_states(interp):
    for (pattern, flags), npos in dl.NPOS.items():
        rx, _ = interp(pattern, flags)
        assert rx.info()["positions"] == npos and rx.atomic_groups()[0] == 0, (pattern, flags, rx.info())
    assert interp(dl.W)[0].groups == 2 and interp(dl.E)[0].groups == 1 and interp(dl.W, B.LC_SYNTAX_SEARCH)[0].groups == 3


def test_family_w_step_counts(interp):
    """2L + 2 on b x L; + 141 per `a` with at least 141 bytes behind it; + 140 for one with 139; the same with and without the memo"""
    _, it = interp(dl.W)
    for L in (300, 4096):
        for memo in (True, False):
            assert steps(it, dl.w_fail(L), memo) == (2 * L + 2, None)
            assert steps(it, dl.w_fail(L, L - 140), memo) == (2 * L + 142, None)
            assert steps(it, dl.w_fail(L, L - 142), memo) == (2 * L + 143, None)
            assert steps(it, dl.w_fail(L, 3), memo) == (2 * L + 143, None)
            assert steps(it, dl.w_over(L), memo) == (2 * L + 2 + 130 * 141, None)
            assert steps(it, dl.w_match(L), memo) == (L + 284, [0, L - 141, L - 140, L])
    assert dl.S == 200142


def test_family_e_step_counts(interp):
    _, it = interp(dl.E)
    for n, plain in ((10, 839), (16, 15123), (20, 103678)):
        assert steps(it, b"a" * n, True) == (7 * n, None) and steps(it, b"a" * n, False) == (plain, None)
    # launch a: under budget 1000 a walk without the memo gives up from n = 11 on, one with the memo never
    assert steps(it, b"a" * 16, False, budget=1000)[1] == "gave_up" and steps(it, b"a" * 12, False, budget=1000)[1] == "gave_up"
    assert all(steps(it, v, True, budget=1000)[1] is None for v in set(dl.launches()["a"].values))
    assert steps(it, b"b", True) == (4, [-1, -1]) and steps(it, b"a", True) == (7, None)       # launch f's values


def test_the_step_counts_written_down_for_the_walks_without_the_memo(interp):
    for pattern, flags, value, frm, want in dl.PLAIN_STEPS:
        _, it = interp(pattern, flags)
        got, r = steps(it, value, False, frm)
        assert got == want, (len(value), flags, frm, got, want)
        assert steps(it, value, False, frm, budget=want)[1] == r and steps(it, value, False, frm, budget=want - 1)[1] == "gave_up"
    assert dl.plain_steps(dl.W, 0, dl.W_S, 0) + 1 == dl.plain_steps(dl.W, 0, dl.W_S1, 0) == dl.S + 1
    # launch d: from L - 60 the walk fits budget 1000 only WITH the memo
    _, it = interp(dl.W, B.LC_SYNTAX_SEARCH)
    assert steps(it, dl.SEARCH_VALUE, True, dl.LONG - 60) == (303, None) and steps(it, dl.SEARCH_VALUE, False, dl.LONG - 60) == (3843, None)
    # launch g: the budget lies on the last step of the first long value
    g = [dl.plain_steps(dl.W, 0, v, 0) for v in dl.G_LONG]
    assert [x > dl.G_BUDGET for x in g] == [False, True, True, False] and g[0] == dl.G_BUDGET


def test_the_restated_sizes():
    assert dl.fixed_bytes(4097) == 4097 * 20 + 64 and dl.fixed_bytes(1) == 84
    assert dl.fixed_bytes(10, closed_cap=4, max_enter=2) == (10 * (9 + 6) + 6) * 4 + 64
    assert dl.memo_bytes(4097, 142) == 290896 and dl.memo_bytes(2, 4) == 16 and dl.memo_bytes(1, 1) == 16 and dl.memo_bytes(8, 4) == 16
    assert dl.memo_bytes(8, 4) + 16 == dl.memo_bytes(8, 4 + 1)        # 16.5 nibble-bytes round to 32
    assert dl.list_cap(dl.POOL_SMALL, 10 ** 9) == dl.LIST_CAP_SMALL == 524272 and dl.list_cap(dl.POOL_SMALL, 7) == 7
    assert dl.list_cap(dl.POOL_DEFAULT, 10 ** 9) == (256 * 2 ** 20 - 256) // 16
    assert dl.fixed_bytes(dl.HUGE + 1) == 9000084 > dl.POOL_SMALL


BRANCHES = {
    # launch: (branch, workers at 8 MiB), (branch, workers at 256 MiB)
    "a": (("memo for all", 128), ("memo for all", 128)),
    "b": (("fewer workers", 22), ("memo for all", 128)),
    "c, budget S": (("no memo", 4), ("memo for all", 6)),
    "c, budget S + 1": (("no memo", 4), ("memo for all", 6)),
    "c, budget unset": (("no memo", 4), ("memo for all", 6)),
    "d, from L - 60": (("memo for all", 1), ("memo for all", 1)),
    "d, from 0": (("no memo", 1), ("memo for all", 1)),
    "e": (("one worker", 1), ("fewer workers", 6)),       # (256 MiB / (9.0 + 31.95 MB) = 6.55)
    "f, list + 5": (("memo for all + list full", 128), ("memo for all", 128)),
    "f, list": (("memo for all", 128), ("memo for all", 128)),
    "c-long": (("no memo", 3), ("memo for all", 3)),
}


def test_the_branch_every_launch_takes_at_8_and_at_256_mib():
    L = dl.launches()
    assert set(L) == set(BRANCHES)
    for name, want in BRANCHES.items():
        got = tuple((p.branch, p.workers) for p in (dl.plan_of(L[name], pool) for pool in (dl.POOL_SMALL, dl.POOL_DEFAULT)))
        assert got == want, (name, got)


def test_what_the_walks_of_each_launch_are_at_8_mib():
    L = dl.launches()
    small = lambda name: dl.plan_of(L[name], dl.POOL_SMALL)
    assert set(small("a").walks) == {"memo"} and small("a").count == 200 > dl.WORKERS
    b = small("b")         # 128 workers with the memo do not fit, 22 do, 23 do not
    need = dl.fixed_bytes(4097) + dl.memo_bytes(4097, 142)
    avail = dl.POOL_SMALL - dl.HEADER_BYTES - 512
    assert need == 372900 and 128 * need > avail and 22 * need <= avail < 23 * need and set(b.walks) == {"memo"}
    assert b.slice == (avail // 22) & ~255 and 1000 < 2 * 4096
    assert small("c, budget S").walks == ["plain", "memo", "plain", "memo", "plain", "memo"]
    assert small("d, from L - 60").walks == ["memo"] and small("d, from 0").walks == ["plain"]
    e = small("e")
    assert e.walks == ["memo"] * 3 + ["no room"] + ["memo"] * 7 and e.slice == dl.POOL_SMALL - 512 and e.count == 11
    f = small("f, list + 5")
    assert (f.count, f.dropped) == (dl.LIST_CAP_SMALL, 5) and set(f.walks) == {"memo"}
    assert (small("f, list").count, small("f, list").dropped) == (dl.LIST_CAP_SMALL, 0)
    # the processor's launch (six values that overflow the thread-list kernels): the long ones walk without the memo
    g = dl.plan(dl.POOL_SMALL, [len(v) + 1 for v in dl.G_LONG] + [342, 331], 142)
    assert (g.branch, g.workers, g.walks) == ("no memo", 4, ["plain"] * 4 + ["memo"] * 2)
    # at 256 MiB every value of the parent's launches has the memo
    for name in ("a", "b", "c-long"):
        assert set(dl.plan_of(L[name], dl.POOL_DEFAULT).walks) == {"memo"}


def test_expected_rows_and_stats():
    L = dl.launches()
    G = B.LC_GAVE_UP
    caps, status, stats, _ = dl.expected(L["a"], dl.POOL_SMALL)
    assert stats == (200, 0) and not status.any() and (caps == -1).all()
    caps, status, stats, _ = dl.expected(L["b"], dl.POOL_SMALL)
    assert stats == (128, 0) and status.tolist() == [1, 0, 0, 0, 1] * 25 + [1, 0, 0] and caps[0].tolist() == [0, 3955, 3956, 4096]
    caps, status, stats, _ = dl.expected(L["c, budget S"], dl.POOL_SMALL)
    assert stats == (6, 1) and status.tolist() == [0, 1, G, 0, 1, 0] and caps[4].tolist() == [0, 99859, 99860, 100000] and (caps[2] == -1).all()
    for name in ("c, budget S + 1", "c, budget unset"):
        _, status, stats, _ = dl.expected(L[name], dl.POOL_SMALL)
        assert stats == (6, 0) and status.tolist() == [0, 1, 0, 0, 1, 0]
    _, status, stats, _ = dl.expected(L["d, from L - 60"], dl.POOL_SMALL)
    assert stats == (1, 0) and status.tolist() == [0]
    caps, status, stats, _ = dl.expected(L["d, from 0"], dl.POOL_SMALL)          # 100 403 steps without the memo: given up at 1000
    assert stats == (1, 1) and status.tolist() == [G] and (caps == -1).all()
    caps, status, stats, _ = dl.expected(L["d, from 0"], dl.POOL_DEFAULT)
    assert stats == (1, 0) and caps.tolist() == [[0, 99941, 0, 99800, 99801, 99941]]
    caps, status, stats, _ = dl.expected(L["e"], dl.POOL_SMALL)
    assert stats == (11, 1) and status.tolist() == [1, 0, 0, G, 1, 0, 0, 0, 0, 0, 0]
    caps, status, stats, pl = dl.expected(L["f, list + 5"], dl.POOL_SMALL)
    assert stats == (524272, 5) and pl.dropped == 5 and 200000 < int(status.sum()) < 320000 and G not in status
    assert dl.expected(L["f, list"], dl.POOL_SMALL)[2] == (524272, 0)
    assert dl.expected(L["c-long"], dl.POOL_DEFAULT)[2] == (3, 0)
