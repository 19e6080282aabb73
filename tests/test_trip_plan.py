"""The planning arithmetic of the packed-lines trip (csrc/trip_buffers.hpp) on the CPU: which lines a chunk takes (tripCarve), where the
offsets and the result arrays lie (tripInLayout, tripLayout), the packed staging (tripPackLines, tripPackPairs) and which shadow ranges
come down in one copy (tripCoalesce).  tests/native/trip_plan_check.cpp is built with AddressSanitizer and UBSan and run as a child
process, with small limits: they are parameters.  The closed forms are written out here."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trip_plan") / "trip_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "loongcollector_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "trip_plan_check.cpp")])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-2000:]
        return r.stdout.decode().split("\n")[:-1]
    return run


def up(v, a=64):
    return (v + a - 1) // a * a


# ---------------------------------------------------------------------------------------------- carve
def carve(plan, lens, max_lines=8, max_bytes=100, line_result=0, max_result=0, cnt=0, size=0, start=0):
    ok, cnt, size = (int(x) for x in plan("carve", max_lines, max_bytes, line_result, max_result, cnt, size, start, *lens)[0].split())
    return bool(ok), cnt, size


def test_carve_takes_the_first_line_even_alone_over_every_cap(plan):
    assert carve(plan, [500, 1], max_bytes=100, line_result=50, max_result=10) == (True, 1, 500)
    assert carve(plan, [7, 500, 1], start=1, max_bytes=100) == (True, 1, 500)


def test_carve_stops_at_max_lines_exactly(plan):
    assert carve(plan, [1] * 9, max_lines=8) == (True, 8, 8)
    assert carve(plan, [1] * 8, max_lines=8) == (True, 8, 8)
    assert carve(plan, [1] * 7, max_lines=8) == (True, 7, 7)      # n reached before any cap


def test_carve_stops_at_max_bytes_exactly_and_one_byte_over(plan):
    assert carve(plan, [40, 60, 1], max_bytes=100) == (True, 2, 100)
    assert carve(plan, [40, 61, 1], max_bytes=100) == (True, 1, 40)
    assert carve(plan, [40, 0, 60, 0, 1], max_bytes=100) == (True, 4, 100)    # (empty lines ride along)


def test_carve_stops_at_the_result_cap_exactly_and_one_line_over(plan):
    assert carve(plan, [1] * 8, line_result=25, max_result=100) == (True, 4, 4)
    assert carve(plan, [1] * 8, line_result=25, max_result=99) == (True, 3, 3)
    assert carve(plan, [1] * 4, line_result=25, max_result=100) == (True, 4, 4)


def test_carve_with_no_result_bytes_per_line_has_no_result_cap(plan):
    assert carve(plan, [1] * 8, line_result=0, max_result=0) == (True, 8, 8)


def test_carve_counts_a_lead_in_line_that_is_already_there(plan):
    # the line before `start` was counted by the caller: it takes one of max_lines and its bytes count, but a first line still goes
    assert carve(plan, [30, 1, 1, 1, 1], start=1, max_lines=3, cnt=1, size=30) == (True, 3, 32)
    assert carve(plan, [30, 71, 1], start=1, max_bytes=100, cnt=1, size=30) == (True, 2, 101)
    assert carve(plan, [30, 70, 1], start=1, max_bytes=100, cnt=1, size=30) == (True, 2, 100)
    assert carve(plan, [30, 1, 1], start=1, max_lines=1, cnt=1, size=30) == (True, 1, 30)     # (no room: the caller's limit is above 1)


def test_carve_refuses_two_gib_of_payload_and_takes_one_byte_less(plan):
    assert carve(plan, [(1 << 31) - 1], max_bytes=32 << 20) == (True, 1, (1 << 31) - 1)
    assert carve(plan, [1 << 31], max_bytes=32 << 20) == (False, 1, 1 << 31)
    assert carve(plan, [1, (1 << 31) - 1], max_bytes=32 << 20) == (True, 1, 1)
    assert carve(plan, [1, (1 << 31) - 1], max_bytes=1 << 32) == (False, 2, 1 << 31)


# ---------------------------------------------------------------------------------------------- layout
RESULT_SETS = {    # bytes per line of each array, in the owner's order (W = 5)
    "delimiter": (5 * 8, 4, 1),                    # spans, ncols, status
    "json": (5 * 24, 4, 4, 1),                     # records, counts, error offsets, status
    "apsara": (5 * 12, 32, 8, 4, 4, 1),            # pairs, base, secs, nanos, npairs, status
    "container log": (24, 4, 1, 1),                # spans, rewrite_begin, status, flags
    "timestamp": (8, 4, 4, 4, 1, 1),               # secs, nanos, matched, frac_len, status, same_as_prev
}


@pytest.mark.parametrize("cnt", [1, 63, 64, 65])
def test_layout_starts_are_aligned_ascending_and_apart(plan, cnt):
    for name, each in RESULT_SETS.items():
        got = [int(x) for x in plan("layout", cnt, *each)[0].split()]
        size, at = got[0], got[1:]
        assert len(at) == len(each) and at[0] == 0 and all(a % 64 == 0 for a in at), name
        for k in range(len(each)):
            end = at[k + 1] if k + 1 < len(each) else size
            assert at[k] + cnt * each[k] <= end, name


@pytest.mark.parametrize("cnt", [1, 63, 64, 65])
def test_layout_equals_the_closed_forms_of_the_five_result_sets(plan, cnt):
    W = 5

    def got(name):
        return [int(x) for x in plan("layout", cnt, *RESULT_SETS[name])[0].split()]
    ncols = up(cnt * W * 8)
    status = ncols + up(cnt * 4)
    assert got("delimiter") == [status + up(cnt), 0, ncols, status]
    count = up(cnt * W * 24)
    err = count + up(cnt * 4)
    status = err + up(cnt * 4)
    assert got("json") == [status + up(cnt), 0, count, err, status]
    base = up(cnt * W * 12)
    secs = base + up(cnt * 32)
    nanos = secs + up(cnt * 8)
    npairs = nanos + up(cnt * 4)
    status = npairs + up(cnt * 4)
    assert got("apsara") == [status + up(cnt), 0, base, secs, nanos, npairs, status]
    rewrite = up(cnt * 24)
    status = rewrite + up(cnt * 4)
    flags = status + up(cnt)
    assert got("container log") == [flags + up(cnt), 0, rewrite, status, flags]
    nanos = up(cnt * 8)
    matched = nanos + up(cnt * 4)
    frac = matched + up(cnt * 4)
    status = frac + up(cnt * 4)
    same = status + up(cnt)
    assert got("timestamp") == [same + up(cnt), 0, nanos, matched, frac, status, same]


def test_layout_with_no_columns_gives_the_first_array_no_room(plan):
    assert [int(x) for x in plan("layout", 65, 0, 4, 1)[0].split()] == [up(65 * 4) + up(65), 0, 0, up(65 * 4)]


@pytest.mark.parametrize("payload, cnt", [(0, 1), (47, 3), (48, 3), (49, 16), (1000, 17)])
def test_input_layout(plan, payload, cnt):
    off_at = up(payload + 16)
    assert off_at - payload >= 16
    assert [int(x) for x in plan("inlayout", payload, cnt, 0)[0].split()] == [off_at, 0, off_at + (cnt + 1) * 4]
    pair_at = off_at + up(cnt * 4)
    assert [int(x) for x in plan("inlayout", payload, cnt, 1)[0].split()] == [off_at, pair_at, pair_at + cnt * 8]


# ---------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("pairs", [0, 1])
@pytest.mark.parametrize("lens, first, cnt", [([3, 0, 5, 0], 0, 4), ([9, 3, 0, 0, 40, 2], 1, 4), ([0], 0, 1), ([48], 0, 1), ([47, 1, 0], 0, 3)])
def test_pack(plan, lens, first, cnt, pairs):
    out = plan("pack", pairs, first, cnt, *lens)
    block = bytes.fromhex(out[1])
    taken = lens[first:first + cnt]
    payload = sum(taken)
    assert int(out[0]) == payload
    off_at = up(payload + 16)
    want = b"".join(bytes([ord("a") + (first + i) % 26]) * n for i, n in enumerate(taken))
    assert block[:payload] == want
    assert block[payload:off_at] == b"\0" * (off_at - payload) and off_at - payload >= 16
    starts = [sum(taken[:i]) for i in range(cnt)]
    assert list(struct.unpack_from("<%dI" % cnt, block, off_at)) == starts
    if pairs:
        pair_at = off_at + up(cnt * 4)
        assert len(block) == pair_at + cnt * 8
        assert list(struct.unpack_from("<%di" % (2 * cnt), block, pair_at)) == [x for n in taken for x in (0, n)]
        assert block[off_at + cnt * 4:pair_at] == b"\xee" * (pair_at - off_at - cnt * 4)       # (never written)
    else:
        assert len(block) == off_at + (cnt + 1) * 4
        assert block[off_at + cnt * 4:] == b"\xee" * 4      # (the cnt + 1-th offset is the caller's to store: the returned count)


# ---------------------------------------------------------------------------------------------- coalesce
def coalesce(plan, gap, *ranges):
    got = [int(x) for x in plan("coalesce", gap, *[x for r in ranges for x in r])[0].split()]
    return got[0], list(zip(got[1::2], got[2::2]))


def test_coalesce_merges_at_a_gap_of_4096_and_not_at_4097(plan):
    assert coalesce(plan, 4096, (10, 20), (20 + 4096, 5000)) == (4990, [(10, 5000)])
    assert coalesce(plan, 4096, (10, 20), (20 + 4097, 5000)) == (10 + 5000 - 4117, [(10, 20), (4117, 5000)])


def test_coalesce_skips_empty_and_inverted_ranges(plan):
    assert coalesce(plan, 4, (5, 5), (9, 7), (100, 110), (111, 111), (200, 100), (120, 130)) == (20, [(100, 110), (120, 130)])
    assert coalesce(plan, 16, (5, 5), (100, 110), (111, 111), (120, 130)) == (30, [(100, 130)])
    assert coalesce(plan, 4096, (5, 5), (9, 7)) == (0, [])


def test_coalesce_of_one_range_and_of_none(plan):
    assert coalesce(plan, 4096, (7, 9)) == (2, [(7, 9)])
    assert coalesce(plan, 4096) == (0, [])


def test_coalesce_moves_the_sum_of_the_merged_lengths(plan):
    ranges = [(i * 3000, i * 3000 + 100) for i in range(4)] + [(20000, 20001), (24097, 24100), (28197, 28200)]
    moved, copies = coalesce(plan, 4096, *ranges)
    assert copies == [(0, 9100), (20000, 24100), (28197, 28200)]
    assert moved == sum(e - b for b, e in copies) == 13203
