"""The conditions tests/test_gpu_bt_launch.py rests on, checked without a GPU: the closed form of the stack-depth family
(tests/helpers/bt_launch_cases.py) against the host build of btRun for every program and value the GPU tests launch, the sizes of the
programs, the step counts, and the two references against each other.

The host walk IS the routine the kernel runs per lane (bt_vm.hpp btRun through tests/native/bt_host_check.cpp): what is asserted here
is where the thresholds lie, not that the walk is right -- that is pinned by tests/test_backref.py against the oracle."""
import numpy as np
import pytest

from loongcollector_amd import binding as B
from tests.helpers import bt_launch_cases as bl


@pytest.fixture(scope="module")
def cases():
    return bl.gpu_cases()


def test_the_programs_have_the_registers_and_sizes_the_helper_states(cases):
    for pattern, flags, nloop, _ in cases:
        rx, blob = bl.compiled(pattern, flags)
        loop = bl.LOOP_EMPTY if bl.LOOP_EMPTY in pattern else bl.LOOP_X
        assert rx.groups == 1 and int(blob[2]) == bl.NCAPS and int(blob[3]) == nloop, (len(pattern), list(blob[:8]))
        assert 4 * len(blob) == bl.program_bytes(nloop, loop), (nloop, 4 * len(blob))
        assert int(blob[0]) <= bl.MAX_INSTRUCTIONS
    rs, sblob = bl.compiled(bl.P(0), B.LC_SYNTAX_SEARCH)
    assert rs.groups == 2 and int(sblob[2]) == bl.NCAPS_SEARCH and int(sblob[3]) == 0


def test_the_stage_threshold_lies_between_two_members_of_the_family():
    m = bl.largest_staged_m()
    assert m == 609       # 464 + 608 x 80 = 49 104 bytes; no member of the family has exactly 49 152
    assert bl.program_bytes(m) <= bl.STAGE_BYTES < bl.program_bytes(m + 1)
    assert 4 * len(bl.compiled(bl.P(m))[1]) == bl.program_bytes(m) and 4 * len(bl.compiled(bl.P(m + 1))[1]) == bl.program_bytes(m + 1)
    assert not any(bl.program_bytes(x) == bl.STAGE_BYTES for x in range(m - 2, m + 3))


def test_the_launch_rules_put_the_programs_where_the_gpu_tests_expect_them():
    nc = bl.NCAPS
    assert not bl.takes_large_slice(nc, bl.M_SMALL_SLICE_LAST) and bl.takes_large_slice(nc, bl.M_SMALL_SLICE_LAST + 1)
    assert nc + bl.M_SMALL_SLICE_LAST == 1856 and (bl.SLICE_WORDS - 1856) // 2 == 96
    assert bl.takes_large_slice(nc, bl.M_LARGE_SLICE) and not bl.takes_large_slice(nc, 700)
    assert nc + bl.Q_ACCEPTED_LAST == 16320 and (bl.RETRY_SLICE_WORDS - 16320) // 2 == 32
    assert not bl.refused(nc, bl.Q_ACCEPTED_LAST) and bl.refused(nc, bl.Q_ACCEPTED_LAST + 1)
    # the batches of the slot test: blocks of pass 1 / pass 2, and the one whose scratch comes from the pool
    assert bl.blocks(65, 64) == (1, 1) and bl.blocks(200, 64) == (1, 1)
    assert bl.blocks(1088) == (17, 2) and bl.blocks(8256) == (129, 16) and bl.blocks(64) == (1, 1)
    assert bl.scratch_bytes(1088) <= bl.POOL_ABOVE_BYTES < bl.scratch_bytes(8256)
    assert bl.edge_ks(nc) == [1, 201, 202, 203, 204, 1635, 1636, 1637, 1638]
    assert bl.edge_ks(nc + 700)[1:] == [131, 132, 133, 134, 1565, 1566, 1567, 1568]


def test_the_closed_form_holds_for_every_value_the_gpu_tests_use(cases):
    """min_words, bisected on the host walk, against max(10 k + 16 | 8, 32) + BT_NCAPS + BT_NLOOP; every value far inside the default
    budget (< 2^20 steps with the large slice, whether it decides the value or runs out of stack)."""
    checked = 0
    for pattern, flags, nloop, ks in cases:
        blob = bl.compiled(pattern, flags)[1]
        for s in bl.values_of(ks):
            checked += 1
            assert bl.min_words(pattern, s, flags) == bl.closed_form(s, bl.NCAPS, nloop), (nloop, len(s), s[-1:])
            assert bl.host_walk(blob, s, bl.RETRY_SLICE_WORDS, 1 << 20) != -1, (nloop, len(s))
            if bl.min_words(pattern, s, flags) <= bl.RETRY_SLICE_WORDS:
                assert bl.min_budget(pattern, s, bl.RETRY_SLICE_WORDS, flags) < 1 << 20
    assert checked > 120
    assert bl.min_budget(bl.P(0), bl.V(1637), 1 << 20) == 21301 and bl.min_budget(bl.P(0), bl.N(1637), bl.RETRY_SLICE_WORDS) == 32743


def test_the_thresholds_of_the_issue(cases):
    p0 = bl.P(0)
    mw = lambda p, s: bl.min_words(p, s)
    assert mw(p0, bl.V(202)) <= bl.SLICE_WORDS < mw(p0, bl.V(203)) and mw(p0, bl.V(1636)) <= bl.RETRY_SLICE_WORDS < mw(p0, bl.V(1637))
    assert mw(p0, bl.N(1637)) == 16382 and mw(p0, bl.N(1638)) > bl.RETRY_SLICE_WORDS
    p700 = bl.P(700)
    assert mw(p700, bl.V(132)) <= bl.SLICE_WORDS < mw(p700, bl.V(133)) and mw(p700, bl.V(1566)) <= bl.RETRY_SLICE_WORDS < mw(p700, bl.V(1567))
    ps = bl.P(bl.M_SMALL_SLICE_LAST)
    assert mw(ps, bl.V(17)) <= bl.SLICE_WORDS < mw(ps, bl.V(18))
    pl = bl.P(bl.M_LARGE_SLICE)
    assert mw(pl, bl.V(1446)) <= bl.RETRY_SLICE_WORDS < mw(pl, bl.V(1447)) and mw(pl, bl.N(1447)) <= bl.RETRY_SLICE_WORDS < mw(pl, bl.N(1448))
    r = bl.R(bl.Q_ACCEPTED_LAST)
    assert mw(r, bl.V(4)) <= bl.RETRY_SLICE_WORDS < mw(r, bl.V(5))


def test_the_oracle_and_re_agree_on_every_value(cases):
    """reference() asserts the agreement; V(k) matches with group 1 = [2k - 2, 2k - 1], N(k) does not"""
    for pattern, flags, nloop, ks in cases:
        for k in ks:
            assert bl.reference(pattern, bl.V(k)) == [2 * k - 2, 2 * k - 1] and bl.reference(pattern, bl.N(k)) is None, (nloop, k)
    for s in (bl.V(bl.PENDING_K), b"cc" + bl.V(bl.PENDING_K), bl.N(3)):
        for frm in (0, 1, 3):
            row = bl.reference(bl.P(0), s, True, frm)      # (N(3) from 3, "babc": no match -- a group that took no part)
            assert (row is None) == (s == bl.N(3) and frm == 3) and (row is None or row[0] >= frm)


def test_expected_applies_the_final_slice_and_the_budget():
    p0 = bl.P(0)
    vals = [bl.V(202), bl.V(203), bl.V(1636), bl.V(1637), bl.N(1637), bl.N(1638)]
    caps, status = bl.expected(p0, vals)
    assert status.tolist() == [1, 1, 1, 3, 0, 3] and caps.tolist() == [[402, 403], [404, 405], [3270, 3271], [-1, -1], [-1, -1], [-1, -1]]
    assert bl.expected(p0, vals, slice_words=bl.SLICE_WORDS)[1].tolist() == [1, 3, 3, 3, 3, 3]
    b = bl.min_budget(p0, bl.V(50), bl.RETRY_SLICE_WORDS)
    assert bl.expected(p0, [bl.V(50)], budget=b)[1].tolist() == [1] and bl.expected(p0, [bl.V(50)], budget=b - 1)[1].tolist() == [3]
    assert np.array_equal(bl.expected(p0, [bl.V(50)], budget=b - 1)[0], [[-1, -1]])
