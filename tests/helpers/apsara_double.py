"""Loads tests/native/apsara_double.cpp (built on first use into tests/_build/libapsara_double.so): the product's host code of
processor_parse_apsara_gpu with the device trip answered by the __host__ instantiation of the per-line routine; and the fixture walk
the CPU and the GPU suite share."""
import ctypes
import json
import os

import numpy as np

from helpers import plugin_double
from helpers.native_build import load_double

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TIME_OK, EPOCH, CANON19 = 1, 2, 4
_libc = ctypes.CDLL(None)


def set_zone(L, tz):
    os.environ["TZ"] = tz
    _libc.tzset()
    L.lc_timestamp_zone_reset()


def double():
    vp, cp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    return load_double("apsara_double", ("apsara_double.cpp", "processor_parse_apsara_gpu.cpp", "processor_parse_timestamp_gpu.cpp", "strptime_program.cpp",
                                         "processor_parse_regex_gpu.cpp", "event_model.cpp"), {
        "ad_process_json_rc": (vp, [vp, cp, ctypes.POINTER(i32), cp, sz]),
        "ad_fail_next_trips": (i32, [i32]),
        "ad_free": (i32, [vp]),
        "ad_parse_one": (None, [cp, u32, u32, u32, cp, u32, vp, vp, vp, vp, vp, vp]),
        "ad_parse_resident": (None, [vp, vp, u32, u32, vp]),
        "ad_parse_stats": (i32, [ctypes.POINTER(ctypes.c_uint64)]),
    })


def host_parse(line, W, head=0, tail=b""):
    """one line through the product's routine on the host -> (status, secs, nanos, base int32[8], npairs, pairs int32[min(npairs, W)][3])"""
    L = double()
    st, secs, ns, npairs = ctypes.c_uint8(), ctypes.c_int64(), ctypes.c_uint32(), ctypes.c_uint32()
    base = np.full(8, -7, np.int32)
    pairs = np.full((W + 2, 3), -7, np.int32)  # two sentinel rows behind W
    L.ad_parse_one(line, len(line), W, head, tail, len(tail), ctypes.byref(st), ctypes.byref(secs), ctypes.byref(ns), base.ctypes.data,
                   ctypes.byref(npairs), pairs.ctypes.data)
    assert (pairs[W:] == -7).all(), "the routine wrote behind W"
    return st.value, secs.value, ns.value, base, npairs.value, pairs[:min(npairs.value, W)].copy()


class Product(plugin_double.Product):
    """processor_parse_apsara_gpu of library L (the double by default) with a fixed clock.  process: (product, group dict) -> group
    dict, for a library that has no ad_process_json_rc (the real one goes through lc_group_from_json)"""
    PREFIX = "lc_apsara_processor"

    def __init__(self, config, now=None, L=None, process=None):
        plugin_double.Product.__init__(self, config, L or double(), *plugin_double.clock_arg(self, now), create="create_with_clock")
        self._process = process

    def zone_offset(self):
        return self.L.lc_apsara_processor_zone_offset(self.h)

    def set_discard(self, enabled=True, interval=43200):
        self.L.lc_apsara_processor_set_discard(self.h, int(enabled), interval)

    def set_first_trip_pairs(self, n):
        self.L.lc_apsara_processor_set_first_trip_pairs(self.h, n)

    def replayed(self):
        s = (ctypes.c_uint64 * 2)()
        self.L.lc_apsara_processor_replayed_lines(self.h, s)
        return int(s[0]), int(s[1])

    def process_group_rc(self, group):
        """(the processor's return code, the events left: [{contents: [[k, v], ...], ts, ns}])"""
        text = json.dumps(group, ensure_ascii=False).encode("latin-1")
        if self._process:
            rc, out = self._process(self, text)
        else:
            err = ctypes.create_string_buffer(512)
            c_rc = ctypes.c_int(0)
            p = self.L.ad_process_json_rc(self.h, text, ctypes.byref(c_rc), err, 512)
            assert p, err.value
            try:
                rc, out = c_rc.value, ctypes.string_at(p).decode("latin-1")
            finally:
                self.L.ad_free(p)
        d = dict(json.loads(out, object_pairs_hook=list) or [])
        events = []
        for ev in d.get("events", []):
            ev = dict(ev)
            events.append({"contents": [list(kv) for kv in ev.get("contents", [])], "ts": ev.get("timestamp"), "ns": ev.get("timestampNanosecond", 0)})
        return rc, events

    def counters(self):
        return self.counter_values()[:4] + [int(self.L.lc_apsara_processor_history_failures(self.h))]


def load_fixtures():
    with open(os.path.join(GOLDEN, "apsara_reference_outputs.json")) as f:
        ref = json.load(f)
    with open(os.path.join(GOLDEN, "apsara_unittest_vectors.json")) as f:
        unit = json.load(f)
    return ref, unit


def all_lines(ref, unit):
    """every source value of both fixture files, as bytes"""
    lines = []
    for case in ref["cases"]:
        lines += case["lines"]
    for case in unit["cases"]:
        for ev in case["in"].get("events", []):
            lines += [v for k, v in ev.get("contents", []) if k == case["config"]["SourceKey"]]
    return [ln.encode("latin-1") for ln in lines]


def group_of(lines):
    events = [{"contents": [["content", ln]], "timestamp": 1, "type": 1} for ln in lines]
    events.append({"contents": [["other", "x"]], "timestamp": 1, "type": 1})
    return {"events": events}


def fixture_runs(ref, unit):
    """-> [(id, zone, config, discard, group, expected ref dict)] over both files"""
    runs = []
    for case in ref["cases"]:
        for zone, want in case["ref"].items():
            for tz in (ref["zones"] if zone == "*" else [zone]):
                runs.append((case["name"] + "@" + tz, tz, case["config"], case["discard"], group_of(case["lines"]), want))
    for case in unit["cases"]:
        for zone, want in case["ref"].items():
            for tz in (unit["zones"] if zone == "*" else [zone]):
                runs.append(("unit:" + case["name"] + "@" + tz, tz, case["config"], False, case["in"], want))
    return runs


def check_run(L, now, run, process=None, first_trip_pairs=None):
    """one fixture run through the product; returns (list of disagreements, product)"""
    name, tz, config, discard, group, want = run
    set_zone(L, tz)
    p = Product(config, now=now, L=L, process=process)
    p.set_discard(discard)
    if first_trip_pairs is not None:
        p.set_first_trip_pairs(first_trip_pairs)
    rc, events = p.process_group_rc(group)
    bad = []
    if rc != 0:
        bad.append("%s: rc %d" % (name, rc))
    if events != want["out"]:
        for i, (g, w) in enumerate(zip(events, want["out"])):
            if g != w:
                bad.append("%s: event %d: %r != reference %r" % (name, i, g, w))
                break
        else:
            bad.append("%s: %d events, reference %d" % (name, len(events), len(want["out"])))
    if p.counters() != want["counters"]:
        bad.append("%s: counters %r != reference %r" % (name, p.counters(), want["counters"]))
    if [m for k, m in p.alarms if k in (0, 1)] != want["alarms"]:
        bad.append("%s: alarms %r != reference %r" % (name, p.alarms, want["alarms"]))
    if p.zone_offset() != want["zone_offset"]:
        bad.append("%s: zone offset %d != reference %d" % (name, p.zone_offset(), want["zone_offset"]))
    return bad, p
