"""processor_parse_timestamp_gpu on a machine without a GPU: the product's HOST code (csrc/processor_parse_timestamp_gpu.cpp: Init, the
zone, the year modes, the cache walk, counters, alarms), the format compiler (csrc/strptime_program.cpp) and the product's PER-VALUE
ROUTINE (strptimeRun of csrc/strptime_vm.hpp, what strptime_kernel runs per lane, compiled for the host).
tests/native/timestamp_double.cpp stands in for the device trip.

Pinned on tests/golden/timestamp_strptime_vectors.json (the reference's own strptime_ns and glibc's mktime under three TZ settings), on
the cases of the reference's ProcessorParseTimestampNativeUnittest.cpp read as data, and on the Python model of ParseLogTime
(helpers/timestamp_model.py) whose arithmetic the vectors pin.

The value-only mutation named in the pull request -- tsIsLeap() of strptime_vm.hpp without its 100-year rule -- fails
test_floor_vectors and test_zone_equals_mktime here (the rule only matters from March on: the random vectors of 2100, such as
"13/Nov/2100:22:42:09 EDT") and test_kernel_floor_vectors on the GPU."""
import ctypes
import json
import os
import random
import time

import pytest

from helpers import timestamp_model as model
from helpers.timestamp_double import INT_MIN, LC_TS_OK, Format, Product, check_vector, double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "timestamp_strptime_vectors.json")) as _f:
    _GOLD = json.load(_f)
VECTORS, TZS = _GOLD["vectors"], _GOLD["tz"]
with open(os.path.join(ROOT, "tests", "golden", "timestamp_unittest_vectors.json")) as _f:
    UNIT = json.load(_f)


@pytest.fixture
def tz():
    """sets the process's zone (libc's too: time.tzset calls tzset) and puts it back"""
    old = os.environ.get("TZ")

    def use(name):
        os.environ["TZ"] = name
        time.tzset()
        double().lc_timestamp_zone_reset()
    yield use
    if old is None:
        os.environ.pop("TZ", None)
    else:
        os.environ["TZ"] = old
    time.tzset()
    double().lc_timestamp_zone_reset()


def test_floor_vectors():
    formats, bad = {}, []
    for v in VECTORS:
        f = formats.get(v["format"]) or formats.setdefault(v["format"], Format(v["format"]))
        for b in check_vector(v, f.parse(v["value"].encode("latin-1"))):
            bad.append((v["format"], v["value"], b))
    assert not bad, bad[:10]
    assert len(VECTORS) > 400


def test_routine_stops_at_the_span_end():
    # the same bytes with digits, names and white space BEHIND the span: the result may not change
    for v in VECTORS[::3]:
        f = Format(v["format"])
        val = v["value"].encode("latin-1")
        for tail in (b"0123456789", b" \t", b"ember", b":30"):
            buf = ctypes.create_string_buffer(val + tail)
            st, secs, ns, m, fl = ctypes.c_uint8(), ctypes.c_int64(), ctypes.c_uint32(), ctypes.c_int32(), ctypes.c_int32()
            f.L.td_parse_one(f.h, buf, len(val), ctypes.byref(st), ctypes.byref(secs), ctypes.byref(ns), ctypes.byref(m), ctypes.byref(fl))
            assert (st.value, secs.value, ns.value, m.value, fl.value) == f.parse(val), (v["format"], v["value"], tail)


@pytest.mark.parametrize("zone", TZS)
def test_zone_equals_mktime(tz, zone):
    tz(zone)
    L = double()
    libc = ctypes.CDLL(None)

    class Tm(ctypes.Structure):
        _fields_ = [(n, ctypes.c_int) for n in ("sec", "min", "hour", "mday", "mon", "year", "wday", "yday", "isdst")] + [
            ("gmtoff", ctypes.c_long), ("zone", ctypes.c_char_p)]
    libc.mktime.restype = ctypes.c_int64
    libc.mktime.argtypes = [ctypes.POINTER(Tm)]
    # every floor vector with a year: the device's civil seconds through the product's zone code = glibc's mktime of the fields
    n = 0
    for v in VECTORS:
        tm = v["tm"]
        if tm is None or tm["year"] == INT_MIN:
            continue
        st, secs, _, _, _ = Format(v["format"]).parse(v["value"].encode("latin-1"))
        assert L.lc_timestamp_zone_seconds(secs, tm["isdst"]) == v["mktime"][zone], (v["format"], v["value"])
        n += 1
    assert n > 200
    # and a sweep against mktime itself: every half hour of 2023 and of the transition days' neighbours, both tm_isdst values
    base = 1672531200  # 2023-01-01 00:00:00 as civil seconds
    for k in range(0, 366 * 48):
        civil = base + k * 1800 + (k % 7)
        t = time.gmtime(civil)
        for dst in (0, 1):
            tm = Tm(t.tm_sec, t.tm_min, t.tm_hour, t.tm_mday, t.tm_mon - 1, t.tm_year - 1900, 0, 0, dst, 0, None)
            assert L.lc_timestamp_zone_seconds(civil, dst) == libc.mktime(ctypes.byref(tm)), (zone, civil, dst)


def test_init_answers(tz):
    tz("CST-8")
    for case in UNIT["init"]:
        if case["error"] is not None:
            with pytest.raises(ValueError) as e:
                Product(case["config"], now=1700000000)
            assert str(e.value) == case["error"], case
            continue
        p = Product(case["config"], now=1700000000)
        assert p.warnings() == case["warnings"], case
        assert p.zone_offset() == case["zone_offset_under_cst8"], case


def test_program_window_is_refused_loudly():
    with pytest.raises(ValueError) as e:
        Product({"SourceKey": "time", "SourceFormat": "%c %c %c %c %c"})
    assert "program window" in str(e.value) and "74 steps" in str(e.value)
    with pytest.raises(ValueError):
        Format("%Y" * 65)
    assert len(Format("%Y" * 64).program()) == 64
    assert len(Format("%c").program()) == 14


@pytest.mark.parametrize("zone", TZS)
def test_processor_equals_model_on_unit_cases(tz, zone):
    """the reference's unit-test cases and the issue's cases, as data: groups of values under a config and a fixed clock; the expectation
    comes from the model (ParseLogTime over the floor-pinned arithmetic, glibc's mktime for the zone)"""
    tz(zone)
    for case in UNIT["groups"]:
        cfg, now = case["config"], case["now"]
        p = Product(cfg, now=now)
        p.set_discard(case.get("discard", True), case.get("interval", 43200))
        m = model.Processor(cfg, now, discard=case.get("discard", True), interval=case.get("interval", 43200))
        for values in case["groups"]:
            got = p.process_values(values)
            want = m.process_values(values)
            assert got == want, (zone, cfg, values)
        assert p.counters() == m.counters, (zone, cfg)
        assert p.alarms == m.alarms, (zone, cfg)
        if zone in case.get("expect", {}):  # literal expectations taken from the reference's unit test
            p2 = Product(cfg, now=now)
            p2.set_discard(case.get("discard", True), case.get("interval", 43200))
            assert [list(x) for x in p2.process_values(case["groups"][0])] == case["expect"][zone], (zone, cfg)


@pytest.mark.parametrize("zone", TZS)
def test_unit_test_literals(tz, zone):
    """the cases of ProcessorParseTimestampNativeUnittest.cpp with the seconds and nanoseconds the unit test itself states"""
    tz(zone)
    n = 0
    for case in UNIT["unit_test_literals"]:
        if zone not in case["zones"]:
            continue
        p = Product(case["config"], now=case["now"])
        p.set_discard(False)
        assert [list(x) for x in p.process_values(case["values"])] == case["expect"], (zone, case["from"])
        assert p.alarms == [], (zone, case["from"])
        n += 1
    assert n >= 16


@pytest.mark.parametrize("zone", TZS)
def test_unit_test_process_cases(tz, zone):
    """TestProcessRegularFormat, TestProcessNoYearFormat, TestProcessRegularFormatFailed, TestProcessHistoryDiscard: values rendered from
    the clock in the local zone, as the unit test renders them; the expected second is now - mLogTimeZoneOffsetSecond"""
    tz(zone)
    now = 1703500000
    lt = time.localtime(now)
    # regular
    p = Product({"SourceKey": "time", "SourceFormat": "%Y-%m-%d %H:%M:%S", "SourceTimezone": "GMT+08:00"}, now=now)
    # (the unit test's "will not be discarded by history timeout" holds where the local zone is within 12 h of GMT+08:00; the rule is
    # switched off here so that the case reads the same under every zone -- TestProcessHistoryDiscard below keeps it on)
    p.set_discard(False)
    v = time.strftime("%Y-%m-%d %H:%M:%S", lt)
    assert p.process_values([v, v]) == [(v, now - p.zone_offset(), 0)] * 2
    assert p.counters() == {"discarded": 0, "out_failed": 0, "key_not_found": 0, "out_successful": 2, "history_failure": 0}
    # no year
    p = Product({"SourceKey": "time", "SourceFormat": "%m-%d %H:%M:%S.%f", "SourceTimezone": "GMT+08:00", "SourceYear": lt.tm_year}, now=now)
    p.set_discard(False)
    v = time.strftime("%m-%d %H:%M:%S.999999999", lt)
    assert p.process_values([v, v]) == [(v, now - p.zone_offset(), 999999999)] * 2
    assert p.counters()["discarded"] == 0 and p.counters()["out_failed"] == 0
    # failed: the value holds a date only; both events stay, both counted failed
    p = Product({"SourceKey": "time", "SourceFormat": "%Y-%m-%d %H:%M:%S", "SourceTimezone": "GMT+08:00"}, now=now)
    v = time.strftime("%Y-%m-%d", time.localtime(now - 43200 - 1))
    assert p.process_values([v, v]) == [(v, 1, None)] * 2
    assert p.counters()["discarded"] == 0 and p.counters()["out_failed"] == 2
    # history discard: one second beyond the interval (the local zone = the source zone, so that the offset is zero)
    p = Product({"SourceKey": "time", "SourceFormat": "%Y-%m-%d %H:%M:%S"}, now=now)
    v = time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(now - 43200 - 1))
    assert p.process_values([v, v]) == []
    assert p.counters() == {"discarded": 2, "out_failed": 0, "key_not_found": 0, "out_successful": 0, "history_failure": 2}


def test_event_outcomes_and_counters(tz):
    tz("UTC")
    p = Product({"SourceKey": "time", "SourceFormat": "%Y-%m-%d %H:%M:%S"}, now=1703466123 + 100)
    group = {"events": [
        {"contents": {"time": "2023-12-25 01:02:03"}, "timestamp": 1, "type": 1},   # success
        {"contents": {"other": "x"}, "timestamp": 1, "type": 1},                     # key not found: kept
        {"contents": {"time": "garbage"}, "timestamp": 1, "type": 1},                # parse failure: kept, alarm
        {"contents": {"time": "2023-12-24 01:02:03"}, "timestamp": 1, "type": 1},   # older than 12 h: dropped, alarm
        {"contents": {"time": "1969-12-31 23:59:59"}, "timestamp": 1, "type": 1},   # tv_sec <= 0: dropped
        {"name": "m", "timestamp": 1, "type": 2, "value": {"type": "untyped_single_value", "detail": 1.0}},  # unsupported: kept, counted failed
    ]}
    left = p.process_group(group)
    assert [e["timestamp"] for e in left] == [1703466123, 1, 1, 1]
    assert p.counters() == {"discarded": 2, "out_failed": 2, "key_not_found": 1, "out_successful": 1, "history_failure": 2}
    assert p.alarms == [(0, "garbage %Y-%m-%d %H:%M:%S"), (1, "logTime: 1703379723"), (1, "logTime: -1")]


def test_a_failed_trip_is_reported_counted_and_a_healthy_call_behind_it_parses(tz, capfd):
    """one parsable event, one without the key, one that is no log event: this processor counts those two in the walk, so a failed trip
    adds nothing but device_failed_events_total"""
    tz("UTC")
    L = double()
    events = [{"contents": {"time": "2023-12-25 01:02:03"}, "timestamp": 1, "type": 1}, {"contents": {"other": "x"}, "timestamp": 1, "type": 1},
              {"content": "no log event", "timestamp": 1, "type": 4}]
    text = "GPU timestamp parse failed (rc=4: the timestamp double has no device); 1 events left without a parsed time"
    zero = {"discarded": 0, "out_failed": 0, "key_not_found": 0, "out_successful": 0, "history_failure": 0}

    def all_counters(p):
        c = (ctypes.c_uint64 * 12)()
        L.lc_timestamp_processor_counters(p.h, c)
        return [int(x) for x in c]
    p = Product({"SourceKey": "time", "SourceFormat": "%Y-%m-%d %H:%M:%S"}, now=1703466123 + 100)
    L.td_fail_next_trips(1)
    assert p.process_group_rc({"events": events}) == (4, events)
    assert p.alarms == [(3, text)]
    assert p.counters() == zero and all_counters(p)[4:6] == [3, 3] and all_counters(p)[11] == 1
    # no sink: exactly one line on stderr
    L.lc_timestamp_processor_set_alarm_sink(p.h, None, None)
    capfd.readouterr()
    L.td_fail_next_trips(1)
    assert p.process_group_rc({"events": events}) == (4, events)
    assert capfd.readouterr().err == "[processor_parse_timestamp_gpu] " + text + "\n"
    assert len(p.alarms) == 1 and p.counters() == zero and all_counters(p)[11] == 2
    rc, left = p.process_group_rc({"events": events})
    assert rc == 0 and left == [dict(events[0], timestamp=1703466123, timestampNanosecond=0)] + events[1:]
    assert p.counters() == dict(zero, out_failed=1, key_not_found=1, out_successful=1) and all_counters(p)[11] == 2


def _random_group(rng, fmt_kind):
    """values of one format with planted collisions: repeats, values that extend a predecessor, failures in between"""
    vals = []
    sec = rng.randrange(1703400000, 1703500000)
    for _ in range(rng.randrange(1, 120)):
        r = rng.random()
        if r < 0.5 and vals:
            pass                       # the same second again
        elif r < 0.8:
            sec += rng.randrange(0, 3)
        else:
            sec = rng.randrange(1703400000, 1703500000)
        t = time.gmtime(sec)
        if fmt_kind == "plain":
            v = time.strftime("%Y-%m-%d %H:%M:%S", t)
        elif fmt_kind == "frac":
            v = time.strftime("%Y-%m-%d %H:%M:%S", t) + "." + str(rng.randrange(10 ** rng.randrange(1, 10)))
        elif fmt_kind == "short":
            v = "%d:%d" % (t.tm_hour, t.tm_min) if rng.random() < 0.5 else time.strftime("%H:%M", t)
        else:
            v = str(sec) + rng.choice(["", "", "123", "123456", " x", "9"])
        k = rng.random()
        if k < 0.08:
            v = v[:rng.randrange(len(v) + 1)]               # a prefix: may fail, may parse shorter
        elif k < 0.16:
            v = v + rng.choice(["5", " tail", "0", ":"])   # an extension of what the cache may hold
        elif k < 0.2:
            v = "x" + v
        vals.append(v)
    return vals


@pytest.mark.parametrize("fmt_kind,fmt", [("plain", "%Y-%m-%d %H:%M:%S"), ("frac", "%Y-%m-%d %H:%M:%S.%f"), ("short", "%H:%M"), ("epoch", "%s")])
def test_run_head_walk_equals_plain_walk_and_model(tz, fmt_kind, fmt):
    tz("EST5EDT,M3.2.0,M11.1.0")
    rng = random.Random({"plain": 1, "frac": 2, "short": 3, "epoch": 4}[fmt_kind])
    cfg = {"SourceKey": "time", "SourceFormat": fmt, "SourceYear": 2023}
    now = 1703500000
    fast, plain = Product(cfg, now=now), Product(cfg, now=now)
    plain.set_plain_walk(True)
    for p in (fast, plain):
        p.set_discard(False)
    m = model.Processor(cfg, now, discard=False)
    for _ in range(60):
        vals = _random_group(rng, fmt_kind)
        a, b, c = fast.process_values(vals), plain.process_values(vals), m.process_values(vals)
        assert a == b, (fmt, vals)
        assert a == c, (fmt, vals)
    assert fast.counters() == plain.counters() == m.counters
    assert fast.alarms == plain.alarms == m.alarms
    walked, in_run = fast.walk_stats()
    assert in_run > 0 and plain.walk_stats()[1] == 0
    if fmt_kind in ("plain", "frac"):
        assert in_run > walked / 4   # the repeats are taken from runs, not walked
