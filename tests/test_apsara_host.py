"""processor_parse_apsara_gpu on the CPU: the product's real host code (Init, stitch, cache replay, second trip, counters, alarms) over
the device trip answered by the per-line routine compiled for the host (tests/native/apsara_double.cpp), against the recorded output of
the reference's own processor compiled from source (tests/golden/apsara_reference_outputs.json, apsara_unittest_vectors.json; how they
were made: tests/golden/README_apsara.md)."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

from helpers import apsara_double as ad

ROOT = ad.ROOT


@pytest.fixture(scope="module")
def L():
    return ad.double()


@pytest.fixture(scope="module")
def fixtures():
    return ad.load_fixtures()


@pytest.fixture(autouse=True)
def _zone_back(L):
    old = os.environ.get("TZ")
    yield
    if old is None:
        os.environ.pop("TZ", None)
        ad._libc.tzset()
        L.lc_timestamp_zone_reset()
    else:
        ad.set_zone(L, old)


all_lines = ad.all_lines


def test_every_fixture_run_equals_the_reference(L, fixtures):
    ref, unit = fixtures
    bad = []
    runs = ad.fixture_runs(ref, unit)
    assert len(runs) > 100
    for run in runs:
        bad += ad.check_run(L, ref["now"], run)[0]
    assert not bad, "\n".join(bad[:20])


def test_small_first_trip_gives_the_same_events(L, fixtures):
    ref, unit = fixtures
    runs = [r for r in ad.fixture_runs(ref, unit) if r[1] == "UTC"]
    bad, trips = [], 0
    for W in (1, 3):
        for run in runs:
            b, p = ad.check_run(L, ref["now"], run, first_trip_pairs=W)
            bad += b
            trips += p.replayed()[1]
    assert not bad, "\n".join(bad[:20])
    assert trips > 0, "no line took the second trip"


def test_replay_statistic(L, fixtures):
    ref, unit = fixtures
    runs = {r[0]: r for r in ad.fixture_runs(ref, unit)}
    for name in ("unit_lines", "cache_equal_seconds", "pairs", "base_fields"):  # (every matched date-form line of these has a 19-byte time)
        _, p = ad.check_run(L, ref["now"], runs[name + "@UTC"])
        assert p.replayed()[0] == 0, name
    for name in ("cache_observable_one_digit", "cache_observable_blanks"):
        _, p = ad.check_run(L, ref["now"], runs[name + "@UTC"])
        assert p.replayed()[0] > 0, name


def test_init_answers_are_the_references(L, fixtures):
    ref, unit = fixtures
    ad.set_zone(L, "UTC")
    for entry in unit["init"]:
        try:
            p = ad.Product(entry["config"], now=unit["now"], L=L)
        except ValueError as e:
            assert not entry["ok"], entry
            assert entry["alarms"] and str(e) in entry["alarms"][-1], (str(e), entry)
            continue
        assert entry["ok"], entry
        assert p.zone_offset() == entry["zone_offset"], entry
        assert len(p.warnings()) == len(entry["alarms"]), (p.warnings(), entry)
        for w, a in zip(p.warnings(), entry["alarms"]):
            assert w in a, (w, a)


def test_bytes_behind_the_line_are_not_read(L, fixtures):
    rng = random.Random(5)
    for line in all_lines(*fixtures):
        want = ad.host_parse(line, 8)
        for head in (0, 1, 15):
            tail = bytes(rng.choice(b"]\t:[\n19.") for _ in range(40))
            got = ad.host_parse(line, 8, head=head, tail=tail)
            assert got[:3] == want[:3] and got[4] == want[4], (line, head)
            assert np.array_equal(got[3], want[3]) and np.array_equal(got[5], want[5]), (line, head)


def test_true_pair_count_and_nothing_behind_w(L, fixtures):
    for line in all_lines(*fixtures)[::3]:
        full = ad.host_parse(line, 400)
        for W in (0, 1, max(full[4] - 1, 0), full[4]):
            got = ad.host_parse(line, W)  # (asserts the sentinel rows behind W)
            assert got[4] == full[4] and np.array_equal(got[5], full[5][:W]), (line, W)


def test_failed_trip_leaves_the_group_untouched(L):
    ad.set_zone(L, "UTC")
    p = ad.Product({"SourceKey": "content"}, now=2000000000)
    p.set_discard(False)
    L.ad_fail_next_trips(1)
    group = ad.group_of(["[2013-03-13 18:05:09.5]\t[INFO]\tk:v"])
    rc, events = p.process_group_rc(group)
    assert rc != 0 and [e["contents"] for e in events] == [[["content", group["events"][0]["contents"][0][1]]], [["other", "x"]]]
    assert [k for k, _ in p.alarms] == [3]
    rc, events = p.process_group_rc(group)
    assert rc == 0 and events[0]["ts"] == 1363197909 and events[0]["ns"] == 500000000


def test_sanitized_host_check_program(fixtures, tmp_path):
    """tests/native/apsara_host_check.cpp under AddressSanitizer + UBSan, as a child process: every fixture line from an exactly-sized
    heap buffer, and the status / seconds it prints are the routine's"""
    exe = str(tmp_path / "apsara_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w",
                           "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "native", "apsara_host_check.cpp")])
    lines = all_lines(*fixtures)
    payload = b"".join(b"%d\n%s\n" % (len(ln), ln) for ln in lines)
    r = subprocess.run([exe], input=payload, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-2000:]
    out = r.stdout.decode().split("\n")[:-1]
    assert len(out) == len(lines)
    for ln, text in zip(lines[::7], out[::7]):
        st, secs, ns, _, npairs, _ = ad.host_parse(ln, 400)
        assert text == "%d %d %d %d" % (st, secs, ns, npairs), ln
