"""processor_parse_container_log_gpu on the CPU: the product's real host code (Init, stitch, in-place copy-back and replay, counters,
alarms) over the device trip answered by the per-line routines compiled for the host (tests/native/container_log_double.cpp), against
the recorded output of the reference's own processor compiled from source (tests/golden/container_log_reference_outputs.json,
container_log_unittest_vectors.json; how they were made: tests/golden/README_container_log.md)."""
import os
import random
import subprocess

import numpy as np
import pytest

from helpers import container_log_product as cp

ROOT = cp.ROOT


@pytest.fixture(scope="module")
def L():
    return cp.double()


@pytest.fixture(scope="module")
def fixtures():
    return cp.load_fixtures()


def _text(line, span):
    return line[span[0]:span[1]]


def test_host_routine_gives_the_references_fields(L, fixtures):
    """every line of the groups that keep every event (no ignored stream, failed lines kept): the event the reference left says whether
    the line parsed and, if so, its time, source, content and partial flag"""
    ref, unit = fixtures
    checked = 0
    for name, config, fmt, chain, group, want in cp.fixture_runs(ref, unit):
        if fmt not in ("1", "2") or chain or config.get("IgnoringStdout") or config.get("IgnoringStderr") or config.get("KeepingSourceWhenParseFail") is False:
            continue
        key = config.get("SourceKey", "content")
        assert len(group["events"]) == len(want["out"]), name
        for ev, out in zip(group["events"], want["out"]):
            src = dict(ev.get("contents", [])).get(key) if ev.get("type") == 1 else None
            if src is None:
                continue
            line = src.encode("latin-1")
            got = dict(out)
            st, fl, spans, rb, rewritten = cp.host_parse(int(fmt), line, in_place=True)
            assert (st == cp.OK) == ("_time_" in got), (name, line, st)
            if fmt == "2" and key != "content":
                assert got[key].encode("latin-1") == rewritten, (name, line)  # the reference's in-place rewrite of the source
            if st != cp.OK:
                continue
            content = _text(rewritten, spans[2])
            if fmt == "2" and content.endswith(b"\n"):
                content = content[:-1]
            assert got["_time_"].encode("latin-1") == _text(rewritten, spans[0]), (name, line)
            assert got["_source_"].encode("latin-1") == _text(rewritten, spans[1]) == (b"stderr" if fl & cp.STDERR else b"stdout"), (name, line)
            assert got["content"].encode("latin-1") == content, (name, line)
            assert ("P" in got) == bool(fl & cp.PARTIAL), (name, line)
            checked += 1
    assert checked > 150


def test_shadow_walk_equals_in_place_walk(L, fixtures):
    """the device's contract on the host: same fields; a line without REPLAY has [rewrite_begin, content end) in the shadow and nothing
    else; the source's bytes in front of rewrite_begin and the shadow's behind it are the in-place text"""
    for fmt, line in cp.all_lines(*fixtures):
        if fmt != cp.DOCKER:
            continue
        st, fl, spans, rb, shadow = cp.host_parse(fmt, line)
        st2, fl2, spans2, rb2, rewritten = cp.host_parse(fmt, line, in_place=True)
        assert (st, fl, rb) == (st2, fl2, rb2) and np.array_equal(spans, spans2), line
        if not fl & cp.ESCAPED:
            assert shadow == b"\xa5" * len(line) and rewritten == line, line
            assert rb == 0, line
        elif not fl & cp.REPLAY and st != cp.FAIL_JSON:
            end = spans[2][1]
            assert 0 < rb <= end and line[rb:rb + 1] == b"\\", line
            assert shadow[:rb] == b"\xa5" * rb and shadow[rb:end] == rewritten[rb:end] and rewritten[:rb] == line[:rb], line
            assert set(shadow[end:]) <= {0xA5}, line


def test_every_fixture_run_equals_the_reference(L, fixtures):
    ref, unit = fixtures
    bad = []
    runs = cp.fixture_runs(ref, unit)
    assert len(runs) >= 70 and sum(1 for r in runs if r[3]) >= 5
    replayed = 0
    for run in runs:
        b, p = cp.check_run(run)
        bad += b
        replayed += p.replayed()
    assert not bad, "\n".join(bad[:20])
    assert replayed > 0, "no line was finished by the host's in-place replay"


def test_stdout_chain_for_both_formats(L, fixtures):
    """the product's split, then this processor, then the product's flag-mode merge against the recorded chain of the reference"""
    ref, unit = fixtures
    chains = [r for r in cp.fixture_runs(ref, unit) if r[3]]
    assert {r[2] for r in chains} == {"1", "2"}
    for run in chains:
        bad, _ = cp.check_run(run)
        assert not bad, "\n".join(bad)
        assert len(run[5]["out"]) > 1


def test_defined_only_lines_fail_as_the_header_defines(L, fixtures):
    """the inputs on which the reference throws: LC_CLOG_FAIL_JSON; kept with the alarm, or erased"""
    ref, _ = fixtures
    entries = ref["defined_only"]
    assert len(entries) >= 5 and len({e["name"] for e in entries}) == len(entries)
    for e in entries:
        line = e["line"].encode("latin-1")
        st, fl, spans, rb, _ = cp.host_parse(cp.DOCKER, line)
        assert st == cp.FAIL_JSON and not spans.any(), e["name"]
    for keep in (True, False):
        p = cp.Product({"KeepingSourceWhenParseFail": keep})
        rc, events, _ = p.process_group_rc({"events": [{"contents": [["content", e["line"]]], "timestamp": 1, "type": 1} for e in entries]}, "2")
        assert rc == 0 and len(events) == (len(entries) if keep else 0)
        assert p.counters() == [len(entries), 0, 0] and len(p.alarms) == len(entries)
        assert all("not a valid json obejct" in m for _, m in p.alarms)


def test_init_warnings_are_the_references(L, fixtures):
    _, unit = fixtures
    assert any(e["alarms"] for e in unit["init"])
    for entry in unit["init"]:
        p = cp.Product(entry["config"])
        assert len(p.warnings()) == len(entry["alarms"]), (p.warnings(), entry)
        for w, a in zip(p.warnings(), entry["alarms"]):
            assert a.startswith(w + ":"), (w, a)
        # ... and the defaults stayed: the recorded run of one stdout line
        key = entry["config"]["SourceKey"] if isinstance(entry["config"].get("SourceKey"), str) else "content"
        rc, events, _ = p.process_group_rc({"events": [{"contents": [[key, cp_T + " stdout F x"]], "timestamp": 1, "type": 1},
                                                       {"contents": [["other", "x"]], "timestamp": 1, "type": 1}]}, "1")
        assert rc == 0 and events == entry["out"] and p.counters() == entry["counters"], entry
    with pytest.raises(ValueError):
        cp.Product([1, 2])


cp_T = "2024-01-05T23:28:06.818486411+08:00"


def test_bytes_around_the_line_are_not_read(L, fixtures):
    rng = random.Random(5)
    for fmt, line in cp.all_lines(*fixtures):
        want = cp.host_parse(fmt, line)
        for head in (1, 15):
            tail = bytes(rng.choice(b' "\\}{PF,:') for _ in range(40))
            got = cp.host_parse(fmt, line, head=head, tail=tail)
            assert got[:2] == want[:2] and got[3:] == want[3:] and np.array_equal(got[2], want[2]), (line, head)


def test_containerd_stops_behind_the_tag(L):
    """the routine reads the header only: bytes behind the byte two behind the second blank do not reach it (they are junk here)"""
    head = b"t stdout P "
    want = cp.host_parse(cp.CONTAINERD, head + b"x" * 300)
    for junk in (b" " * 300, b"P F " * 75, bytes(range(256)) + b"\0" * 44):
        got = cp.host_parse(cp.CONTAINERD, head + junk)
        assert got[:2] == want[:2] and np.array_equal(got[2], want[2])
    assert want[1] & cp.PARTIAL and list(want[2][2]) == [11, 311]


def test_failed_trip_leaves_the_group_untouched(L):
    p = cp.Product({})
    L.cd_fail_next_trips(1)
    group = {"events": [{"contents": [["content", '{"log":"a\\nb","stream":"stdout","time":"t"}']], "timestamp": 1, "type": 1},
                        {"contents": [["other", "x"]], "timestamp": 1, "type": 1}]}
    rc, events, metadata = p.process_group_rc(group, "2")
    assert rc != 0 and events == [ev["contents"] for ev in group["events"]]
    assert [k for k, _ in p.alarms] == [3] and p.counters() == [0, 0, 0]
    assert p.counter_values()[11] == 1  # LC_CNT_DEVICE_FAILED_EVENTS
    rc, events, _ = p.process_group_rc(group, "2")
    assert rc == 0 and events[0] == [["content", "a\nb"], ["_time_", "t"], ["_source_", "stdout"]]


def test_no_trip_for_other_formats_and_empty_groups(L):
    stats = (cp.ctypes.c_uint64 * 2)()
    L.cd_parse_stats(stats)
    before = int(stats[0])
    p = cp.Product({})
    for fmt in ("3", None, ""):
        rc, events, _ = p.process_group_rc({"events": [{"contents": [["content", "a stdout F x"]], "timestamp": 1, "type": 1}]}, fmt)
        assert rc == 0 and events[0] == [["content", "a stdout F x"]]
    assert p.process_group_rc({"events": []}, "1")[0] == 0
    assert p.process_group_rc({"events": [{"contents": [["other", "x"]], "timestamp": 1, "type": 1}]}, "1")[0] == 0
    L.cd_parse_stats(stats)
    assert int(stats[0]) == before


def test_sanitized_host_check_program(fixtures, tmp_path):
    """tests/native/container_log_host_check.cpp under AddressSanitizer + UBSan, as a child process: every fixture line and every
    defined_only line from exactly-sized heap buffers, the Docker rewrite in place and into an exactly-sized shadow"""
    exe = str(tmp_path / "container_log_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w",
                           "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "native", "container_log_host_check.cpp")])
    lines = cp.all_lines(*fixtures) + [(cp.DOCKER, e["line"].encode("latin-1")) for e in fixtures[0]["defined_only"]]
    payload = b"".join(b"%d %d\n%s\n" % (fmt, len(ln), ln) for fmt, ln in lines)
    r = subprocess.run([exe], input=payload, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-2000:]
    out = r.stdout.decode().split("\n")[:-1]
    assert len(out) == len(lines)
    for (fmt, ln), text in zip(lines[::5], out[::5]):
        st, fl, spans, rb, _ = cp.host_parse(fmt, ln)
        assert text == "%d %d %s %d" % (st, fl, " ".join(str(int(v)) for v in spans.ravel()), rb), ln
