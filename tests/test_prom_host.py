"""processor_prom_parse_metric_gpu on the CPU: the per-line routine of csrc/prom_vm.hpp compiled for the host, its host finish and the
product's real processor code (Init, gather, second trip, event build, counters, alarms) over the device trip answered by that routine
(tests/native/prom_double.cpp), against the recorded output of the reference's own TextParser compiled from source
(tests/golden/prom_reference_outputs.json, prom_unittest_vectors.json; how they were made: tests/golden/README_prom.md)."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from helpers import prom_product as pp

ROOT = pp.ROOT
HONOR = {"job_name": "j"}


@pytest.fixture(scope="module")
def L():
    return pp.double()


@pytest.fixture(scope="module")
def fixtures():
    return pp.load_fixtures()


@pytest.fixture(scope="module")
def cases(fixtures):
    return pp.all_cases(*fixtures)


def _walk(cases, defaults, L=None):
    bad = []
    for label, line, honor, entry in cases:
        pp.check_against_reference(label, line, honor, entry, pp.host_parse(line, honor, W=64, L=L), defaults, bad, L=L)
    return bad


def test_host_routine_and_finish_equal_the_reference(L, fixtures, cases):
    """every fixture line: ok / fail, the failure site where the generator aimed at one, and on success the name, the tags in order
    (Insert semantics over the reported labels, escaped values rewritten), the value BIT FOR BIT, seconds and nanoseconds"""
    ref, unit = fixtures
    assert len(ref["cases"]) > 2200 and len({e["case"] for e in unit["cases"]}) == 7
    sites = [e["site"] for e in ref["cases"] if e.get("site")]
    for site in pp.STATUS:
        if site not in ("COMMA_OR_BRACE", "TIMESTAMP_NAN"):  # (unreachable in the reference; defined here only)
            assert sites.count(site) >= 2, site
    bad = _walk(cases, ref["defaults"])
    assert not bad, "\n".join(bad[:20])


def _strtod_bits(token):
    libc = ctypes.CDLL(None)
    libc.strtod.restype = ctypes.c_double
    libc.strtod.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p)]
    return int(np.array([libc.strtod(token, None)], np.float64).view(np.uint64)[0])


def test_deferral_rule_is_exact(L, cases):
    """a value token is converted by the routine if and only if it meets the rule of the issue's section 1 (restated in
    helpers/prom_product.device_rule), and then its bits are strtod's; a timestamp token if and only if it is a digit string below 2^53"""
    device = host = time_device = time_host = 0
    for label, line, honor, entry in cases:
        got = pp.host_parse(line, honor, W=1, finish=False)
        vb, ve = got["value_span"]
        reached = got["status"] == pp.OK or got["status"] >= pp.STATUS["TIME_END"]
        if reached and ve > vb:
            token = line[vb:ve]
            want = pp.device_rule(token)
            assert bool(got["flags"] & pp.VALUE_HOST) == (want is None), (label, token)
            if want is None:
                host += 1
            elif got["status"] == pp.OK:
                device += 1
                assert got["value"] == want == _strtod_bits(token), (label, token, "%016x" % got["value"])
        tb, te = got["time_span"]
        if te > tb and got["status"] in (pp.OK, pp.STATUS["TIMESTAMP_SMALL"]):
            on_device = pp.time_rule(line[tb:te])
            assert bool(got["flags"] & pp.TIME_HOST) == (not on_device) or got["status"] != pp.OK, (label, line[tb:te])
            time_device += on_device
            time_host += not on_device
    assert device > 800 and host > 500 and time_device > 10 and time_host > 10, (device, host, time_device, time_host)


def test_device_path_borders():
    two53 = 1 << 53
    for token, on_device in ((str(two53 - 1), True), (str(two53), True), (str(two53 + 1), False), ("1e22", True), ("1e23", False), ("1e-22", True),
                             ("1e-23", False), ("%de22" % two53, True), ("0.1", True), ("0x1A", False), ("1e", False), ("-0", True), ("0e999", True),
                             ("iNf", True), ("-nAn", True), ("infinit", False), ("123456789012345678", False), ("1.5e23", True), ("1.5e24", False), ("15e21", True), ("15e22", True), ("15e23", False), ("0.15e-21", False), ("0.15e-20", True)):
        got = pp.host_parse(b"m " + token.encode(), finish=False)
        assert bool(got["flags"] & pp.VALUE_HOST) == (not on_device), token
        assert (pp.device_rule(token.encode()) is not None) == on_device, token
    # the host finish of what was left: 0x1A is 26, 0x1e3 is 483 (a hex float, not an exponent)
    assert pp.host_parse(b"m 0x1A")["value"] == _strtod_bits(b"26") and pp.host_parse(b"m 0x1e3")["value"] == _strtod_bits(b"483")
    assert pp.host_parse(b"m 0x1A")["finished"] == 1 and pp.host_parse(b"m 0x1A 1.7e12")["finished"] == 2 and pp.host_parse(b"m 1 1715829785083")["finished"] == 0


def test_defined_only_lines_fail_as_the_header_defines(fixtures):
    entries = fixtures[0]["defined_only"]
    assert len(entries) >= 4 and len({e["name"] for e in entries}) == len(entries)
    for e in entries:
        got = pp.host_parse(e["line"].encode("latin-1"), e["honor"])
        assert got["status"] == pp.STATUS[e["status"]] and not got["flags"] & pp.HAS_TIME, e["name"]
    p = pp.Product(HONOR)
    rc, events = p.process([e["line"].encode("latin-1") for e in entries])
    assert rc == 0 and events == [] and p.counters()[pp.OUT_FAILED] == len(entries)


def test_bytes_around_the_line_are_not_read(cases):
    rng = random.Random(5)
    for label, line, honor, _ in cases[::3]:
        want = pp.host_parse(line, honor, W=20)
        for head in (1, 15):
            tail = bytes(rng.choice(b' "\\}{=,#19e') for _ in range(40))
            got = pp.host_parse(line, honor, W=20, head=head, tail=tail)
            for k in pp.OUT_KEYS:
                assert np.array_equal(got[k], want[k]), (label, head, k)


def test_labels_above_w_keep_the_true_count():
    line = b"m{%s} 1" % b",".join(b'l%d="v%d"' % (k, k) for k in range(17))
    wide = pp.host_parse(line, W=32)
    for W in (1, 2, 16, 17):
        got = pp.host_parse(line, W=W)  # (host_parse asserts that nothing behind min(nlabels, W) was written)
        assert got["nlabels"] == 17 and got["status"] == pp.OK
        assert np.array_equal(got["labels"][:min(W, 17)], wide["labels"][:min(W, 17)])


# ---------------------------------------------------------------------------------------------- the processor
def _metric(ev):
    return (ev["name"], ev["tags"], ev["bits"], ev["secs"], ev["nanos"])


def test_processor_builds_the_references_events(L, fixtures):
    """all fixture lines of one honor setting as ONE group: a metric event per line the reference parsed, in order, with the reference's
    name, tags (plus __name__, set last), bits and time"""
    ref, unit = fixtures
    for honor in (True, False):
        entries = [e for e in ref["cases"] + unit["cases"] if e["honor"] == honor]
        p = pp.Product({"job_name": "j", "honor_timestamps": honor})
        scrape = ref["defaults"]["secs"] * 1000 + ref["defaults"]["nanos"] // 1000000
        rc, events = p.process([e["line"].encode("latin-1") for e in entries], scrape)
        assert rc == 0 and all(ev["type"] == 2 for ev in events)
        want = []
        for e in entries:
            if not e["ok"]:
                continue
            tags = [[k.encode("latin-1"), v.encode("latin-1")] for k, v in e["tags"]]
            for t in tags:
                if t[0] == b"__name__":
                    t[1] = e["name"].encode("latin-1")
                    break
            else:
                tags.append([b"__name__", e["name"].encode("latin-1")])
            want.append((e["name"].encode("latin-1"), [tuple(t) for t in tags], int(e["bits"], 16), e["secs"], e["nanos"]))
        assert [_metric(ev) for ev in events] == want
        c = p.counters()
        assert c[pp.OUT_SUCCESSFUL] == len(want) and c[pp.OUT_FAILED] == len(entries) - len(want) and c[pp.DISCARDED] == 0
        assert p.mop_up_lines() == sum(1 for e in entries if e["ok"] and e["line"].count('="') > 16) and (p.mop_up_lines() > 0 or not honor)
        assert p.deferred_tokens() > 100 or not honor


def test_processor_drops_other_events_and_failed_lines_and_keeps_order(L):
    lines = [b'a{x="1"} 1', None, b"broken{", b'b{y="2"} 2 1715829785083', None, b'c 0x1A', b"", b'd{__name__="other",z="3"} 4']
    p = pp.Product(HONOR)
    rc, events = p.process(lines, 1700000000123)
    assert rc == 0
    assert [_metric(ev) for ev in events] == [
        (b"a", [(b"x", b"1"), (b"__name__", b"a")], _strtod_bits(b"1"), 1700000000, 123000000),
        (b"b", [(b"y", b"2"), (b"__name__", b"b")], _strtod_bits(b"2"), 1715829785, 83000000),
        (b"c", [(b"__name__", b"c")], _strtod_bits(b"26"), 1700000000, 123000000),
        (b"d", [(b"__name__", b"d"), (b"z", b"3")], _strtod_bits(b"4"), 1700000000, 123000000)]  # (overwritten in place)
    c = p.counters()
    assert (c[pp.DISCARDED], c[pp.OUT_FAILED], c[pp.OUT_SUCCESSFUL]) == (2, 2, 4) and p.deferred_tokens() == 1 and not p.alarms
    # unescaped values are views into the raw event's content; escaped ones and __name__ are copies
    rc, events = p.process([b'm{a="plain",b="x\\\\y",c=""} 1'])
    assert events[0]["tags"] == [(b"a", b"plain"), (b"b", b"x\\y"), (b"c", b""), (b"__name__", b"m")] and events[0]["views"] == [True, False, True, False]
    # honor_timestamps off: the line's own timestamp is not even looked at
    off = pp.Product({"job_name": "j", "honor_timestamps": False})
    rc, events = off.process([b"m 1 1715829785083", b"m 2 bar"], 1700000000123)
    assert [(ev["secs"], ev["nanos"]) for ev in events] == [(1700000000, 123000000)] * 2


@pytest.mark.parametrize("W", [1, 2, 16])
def test_processor_second_trip_for_lines_wider_than_the_first(L, W):
    stats = (ctypes.c_uint64 * 2)()
    lines = [b"m%d{%s} %d" % (n, b",".join(b'l%d="v\\\\%d"' % (k, k) if k % 5 == 4 else b'l%d="v%d"' % (k, k) for k in range(n)), n) for n in (0, W - 1, W, W + 1, 3 * W + 2)]
    lines.insert(2, b"fails{%s" % b",".join(b'l%d="v"' % k for k in range(W + 3)))  # (a failed line above W takes no second trip)
    p = pp.Product(HONOR)
    p.set_first_trip_labels(W)
    L.pd_parse_stats(stats)
    before = int(stats[0])
    rc, events = p.process(lines, 1700000000123)
    L.pd_parse_stats(stats)
    assert rc == 0 and int(stats[0]) - before == 2 and p.mop_up_lines() == 2
    assert [_metric(ev) for ev in events] == pp.expected_events(lines, True, 1700000000123)
    assert [len(ev["tags"]) for ev in events] == [1, W, W + 1, W + 2, 3 * W + 3]


@pytest.mark.parametrize("scrape", [None, "", "17x", "-5", "1e3", " 1700000000123", "18446744073709551616"])
def test_missing_or_garbled_scrape_timestamp_is_zero_and_warned(L, scrape):
    p = pp.Product(HONOR)
    rc, events = p.process([b"m 1", b"m 2 1715829785083"], scrape)
    assert rc == 0 and [(ev["secs"], ev["nanos"]) for ev in events] == [(0, 0), (1715829785, 83000000)]
    assert [k for k, _ in p.alarms] == [1] and "parse scrape timestamp failed" in p.alarms[0][1]


def test_failed_trip_leaves_the_group_untouched(L):
    p = pp.Product(HONOR)
    L.pd_fail_next_trips(1)
    rc, events = p.process([b"m 1", None, b"m 2"])
    assert rc != 0 and [ev["type"] for ev in events] == [4, 1, 4]
    assert [k for k, _ in p.alarms] == [3] and p.counters()[pp.DEVICE_FAILED] == 2 and p.counters()[pp.OUT_SUCCESSFUL] == 0
    rc, events = p.process([b"m 1", None, b"m 2"])
    assert rc == 0 and [ev["type"] for ev in events] == [2, 2]


def test_no_trip_without_raw_events(L):
    stats = (ctypes.c_uint64 * 2)()
    L.pd_parse_stats(stats)
    before = int(stats[0])
    p = pp.Product(HONOR)
    assert p.process([]) == (0, [])
    assert p.process([None, None]) == (0, [])  # (dropped all the same: the reference swaps in an empty container)
    L.pd_parse_stats(stats)
    assert int(stats[0]) == before and p.counters()[pp.DISCARDED] == 2


INIT_CASES = [
    ({"job_name": "j"}, True), ({"job_name": "j", "honor_timestamps": False}, True), ({"job_name": "j", "honor_timestamps": "no"}, True),
    ({}, False), ({"job_name": ""}, False), ({"job_name": 5}, False), ([1, 2], False),
    ({"job_name": "j", "scrape_interval": "15s", "scrape_timeout": "1m", "max_scrape_size": "10MB"}, True),
    ({"job_name": "j", "scrape_interval": "0s"}, False), ({"job_name": "j", "scrape_interval": "15"}, False), ({"job_name": "j", "scrape_interval": "15h"}, False),
    ({"job_name": "j", "scrape_interval": "s"}, False), ({"job_name": "j", "scrape_interval": 15}, True), ({"job_name": "j", "scrape_timeout": "00m"}, False),
    ({"job_name": "j", "scrape_timeout": "1.5s"}, False), ({"job_name": "j", "max_scrape_size": "0MB"}, False), ({"job_name": "j", "max_scrape_size": "10"}, False),
    ({"job_name": "j", "max_scrape_size": ""}, False), ({"job_name": "j", "max_scrape_size": "1GiB"}, True), ({"job_name": "j", "max_scrape_size": "5B"}, True),
    ({"job_name": "j", "max_scrape_size": "xKB"}, False), ({"job_name": "j", "max_scrape_size": "7K"}, True),
    ({"job_name": "j", "relabel_configs": [{"action": "no such action"}], "metric_relabel_configs": "ignored"}, True),
]


@pytest.mark.parametrize("config,accepted", INIT_CASES)
def test_init_cases(L, config, accepted):
    if not accepted:
        with pytest.raises(ValueError):
            pp.Product(config)
        return
    p = pp.Product(config)
    honor = config.get("honor_timestamps") is not False
    rc, events = p.process([b"m 1 1715829785083"], 1700000000123)
    assert rc == 0 and events[0]["secs"] == (1715829785 if honor else 1700000000)


def test_bench_corpus_defers_and_fails_nothing():
    """the condition of tools/prom_bench.py's kernel row: the generator's lines are all decided on the device"""
    from loongcollector_amd import corpus
    lines = corpus.prom_exposition_lines(20000)
    assert all(10 <= len(ln.split(b"{")[0].split(b" ")[0]) <= 40 for ln in lines) and max(ln.count(b'="') for ln in lines) == 8
    escaped = 0
    for ln in lines:
        got = pp.host_parse(ln, W=8, finish=False)
        assert got["status"] == pp.OK and not got["flags"] & (pp.VALUE_HOST | pp.TIME_HOST), ln
        escaped += bool(got["flags"] & pp.ANY_ESCAPE)
    assert escaped > 50
    mixed = corpus.prom_exposition_lines(20000, deferred=0.05, failing=0.05)
    res = [pp.host_parse(ln, W=8, finish=False) for ln in mixed]
    assert 800 < sum(1 for r in res if r["flags"] & pp.VALUE_HOST) < 1200 and 800 < sum(1 for r in res if r["status"] != pp.OK) < 1200


def test_sanitized_host_check_program(cases, fixtures, tmp_path):
    """tests/native/prom_host_check.cpp under AddressSanitizer + UBSan, as a child process: every fixture line and every defined_only
    line from exactly-sized heap buffers, at three heads, with exactly W label entries to write into"""
    exe = str(tmp_path / "prom_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w",
                           "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "native", "prom_host_check.cpp")])
    lines = [(honor, ln) for _, ln, honor, _ in cases] + [(e["honor"], e["line"].encode("latin-1")) for e in fixtures[0]["defined_only"]]
    payload = b"".join(b"%d %d\n%s\n" % (honor, len(ln), ln) for honor, ln in lines)
    r = subprocess.run([exe], input=payload, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-2000:]
    out = r.stdout.decode().split("\n")[:-1]
    assert len(out) == len(lines)
    for (honor, ln), text in zip(lines[::5], out[::5]):
        g = pp.host_parse(ln, honor, W=64)
        want = "%d %d %d %d %016x %d %d %d %d %d %d %d" % (g["status"], g["flags"], g["name"][0], g["name"][1], g["value"], g["value_span"][0], g["value_span"][1],
                                                         g["time_span"][0], g["time_span"][1], g["secs"], g["nanos"], g["nlabels"])
        assert text.rsplit(" ", 1)[0] == want, ln


# value-only mutations of csrc/prom_vm.hpp; each must fail the test named beside it (tests/golden/README_prom.md lists them)
MUTATIONS = {
    "escape_read_from_the_byte_behind_the_backslash": ("switch (line[vb + 1]) {", "switch (line[p + 1]) {", "test_host_routine_and_finish_equal_the_reference"),
    "exponent_bound_23": ("constexpr int32_t kPromExponentBound = 22;", "constexpr int32_t kPromExponentBound = 23;", "test_deferral_rule_is_exact"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutations_are_caught(name, fixtures, cases, tmp_path):
    old, new, caught_by = MUTATIONS[name]
    M = pp.mutated_routines(tmp_path, old, new)
    if caught_by == "test_host_routine_and_finish_equal_the_reference":
        bad = _walk(cases, fixtures[0]["defaults"], L=M)
        assert len(bad) >= 5 and all("\\\\" in b for b in bad), bad[:5]  # (only lines that hold a backslash, shown doubled by %r)
    else:
        wrong = 0
        for label, line, honor, entry in cases:
            got = pp.host_parse(line, honor, W=1, finish=False, L=M)
            vb, ve = got["value_span"]
            if got["status"] == pp.OK and ve > vb:
                wrong += bool(got["flags"] & pp.VALUE_HOST) != (pp.device_rule(line[vb:ve]) is None)
        assert wrong >= 5
    assert not _walk(cases[:50], fixtures[0]["defaults"])  # (the unmutated routine, same walk)
