"""Loads tests/native/timestamp_double.cpp (built on first use into tests/_build/libtimestamp_double.so): the product's host code of
processor_parse_timestamp_gpu with the device calls answered by the __host__ instantiation of the per-value routine."""
import ctypes
import json

from helpers import plugin_double
from helpers.native_build import load_double

INT_MIN = -2 ** 31
LC_TS_OK, LC_TS_HAS_YEAR, LC_TS_DST, LC_TS_EPOCH, LC_TS_ABSENT = 1, 2, 4, 8, 0x80


def double():
    vp, cp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    return load_double("timestamp_double", ("timestamp_double.cpp", "processor_parse_timestamp_gpu.cpp", "strptime_program.cpp", "event_model.cpp"), {
        "td_process_json": (vp, [vp, cp, cp, sz]),
        "td_process_json_rc": (vp, [vp, cp, ctypes.POINTER(i32), cp, sz]),
        "td_fail_next_trips": (i32, [i32]),
        "td_fail_after": (i32, [i32]),
        "td_free": (i32, [vp]),
        "td_parse_one": (None, [vp, cp, u32, vp, vp, vp, vp, vp]),
        "td_parse_stats": (i32, [ctypes.POINTER(ctypes.c_uint64)]),
    })


class Format:
    """a compiled SourceFormat; parse(value bytes) -> (status, secs, nanos, matched, frac_len) through the product's routine on the host"""

    def __init__(self, fmt, L=None):
        self.L = L or double()
        self.h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(256)
        rc = self.L.lc_strptime_create(fmt.encode("latin-1"), ctypes.byref(self.h), err, 256)
        if rc != 0:
            self.h = None
            raise ValueError(err.value.decode())

    def program(self):
        w = (ctypes.c_uint32 * 64)()
        n = self.L.lc_strptime_program(self.h, w)
        return list(w)[:n]

    def parse(self, value):
        st, secs, ns, m, fl = ctypes.c_uint8(), ctypes.c_int64(), ctypes.c_uint32(), ctypes.c_int32(), ctypes.c_int32()
        self.L.td_parse_one(self.h, value, len(value), ctypes.byref(st), ctypes.byref(secs), ctypes.byref(ns), ctypes.byref(m), ctypes.byref(fl))
        return st.value, secs.value, ns.value, m.value, fl.value

    def __del__(self):
        if getattr(self, "h", None):
            self.L.lc_strptime_destroy(self.h)
            self.h = None


class Product(plugin_double.Product):
    """processor_parse_timestamp_gpu of library L (the double by default) with a fixed clock"""
    PREFIX = "lc_timestamp_processor"

    def __init__(self, config, now=None, L=None, process=None):
        plugin_double.Product.__init__(self, config, L or double(), *plugin_double.clock_arg(self, now), create="create_with_clock")
        self._process = process

    def zone_offset(self):
        return self.L.lc_timestamp_processor_zone_offset(self.h)

    def set_discard(self, enabled=True, interval=43200, onetime=False):
        self.L.lc_timestamp_processor_set_discard(self.h, int(enabled), interval, int(onetime))

    def set_plain_walk(self, on):
        self.L.lc_timestamp_processor_set_plain_walk(self.h, int(on))

    def walk_stats(self):
        s = (ctypes.c_uint64 * 2)()
        self.L.lc_timestamp_processor_walk_stats(self.h, s)
        return int(s[0]), int(s[1])

    def process_group(self, group):
        if self._process:
            d = self._process(self, group)
        else:
            err = ctypes.create_string_buffer(512)
            p = self.L.td_process_json(self.h, json.dumps(group, ensure_ascii=False).encode("latin-1"), err, 512)
            assert p, err.value
            try:
                d = json.loads(ctypes.string_at(p).decode("latin-1"))
            finally:
                self.L.td_free(p)
        return (d or {}).get("events", [])

    def process_group_rc(self, group):
        """the double only: (the processor's return code, the events that are left)"""
        err = ctypes.create_string_buffer(512)
        rc = ctypes.c_int(0)
        p = self.L.td_process_json_rc(self.h, json.dumps(group, ensure_ascii=False).encode("latin-1"), ctypes.byref(rc), err, 512)
        assert p, err.value
        try:
            return rc.value, (json.loads(ctypes.string_at(p).decode("latin-1")) or {}).get("events", [])
        finally:
            self.L.td_free(p)

    def process_values(self, values, key="time"):
        """-> per event left: (value, timestamp, nanoseconds or None)"""
        events = [{"contents": {key: v}, "timestamp": 1, "type": 1} for v in values]
        out = []
        for ev in self.process_group({"events": events}):
            out.append((ev["contents"][key], ev["timestamp"], ev.get("timestampNanosecond")))
        return out

    def counters(self):
        d = dict(zip(["discarded", "out_failed", "key_not_found", "out_successful"], self.counter_values()))
        d["history_failure"] = int(self.L.lc_timestamp_processor_history_failures(self.h))
        return d


def check_vector(vec, got):
    """one floor vector (tests/golden/timestamp_strptime_vectors.json) against (status, secs, nanos, matched, frac_len); returns the
    list of disagreements"""
    st, secs, ns, matched, flen = got
    bad = []
    ok = vec["matched"] >= 0
    if bool(st & LC_TS_OK) != ok:
        return ["ok %s, reference %s" % (bool(st & LC_TS_OK), ok)]
    if ok:
        if matched != vec["matched"]:
            bad.append("matched %d != %d" % (matched, vec["matched"]))
        if flen != max(vec["nanos_len"], 0):
            bad.append("frac_len %d != %d" % (flen, vec["nanos_len"]))
    if ok or vec["format"] != "%s":
        if ns != vec["nanos"] % 2 ** 32:
            bad.append("nanos %d != %d" % (ns, vec["nanos"]))
    tm = vec["tm"]
    if tm is None:  # "%s"
        if ok:
            if not st & LC_TS_EPOCH:
                bad.append("no epoch flag")
            for tz, t in vec["mktime"].items():
                if secs != t:
                    bad.append("epoch secs %d != %d (%s)" % (secs, t, tz))
        return bad
    if bool(st & LC_TS_HAS_YEAR) != (tm["year"] != INT_MIN):
        bad.append("has_year")
    if bool(st & LC_TS_DST) != bool(tm["isdst"]):
        bad.append("dst")
    tod = tm["hour"] * 3600 + tm["min"] * 60 + tm["sec"]
    if tm["year"] != INT_MIN:
        # (tm_isdst = 1 under a zone without summer time: glibc's mktime refuses, -1 is no calendar arithmetic -- the zone tests hold it)
        if not tm["isdst"] and secs != vec["mktime"]["UTC"]:
            bad.append("civil secs %d != mktime under UTC %d" % (secs, vec["mktime"]["UTC"]))
    elif secs != (tm["mon"] << 40 | tm["mday"] << 32 | tod):
        bad.append("month/day/second-of-day %x" % secs)
    return bad
