"""Loads tests/native/container_log_double.cpp (built on first use into tests/_build/libcontainer_log_double.so): the product's host
code of processor_parse_container_log_gpu with the device trip answered by the __host__ instantiation of the per-line routines, plus
the product's flag-mode merge behind a host model of its line split for the stdout chain; and the fixture walk the CPU and the GPU suite share."""
import ctypes
import json
import os

import numpy as np

from helpers import plugin_double
from helpers.native_build import load_double, oracle_link

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT_FAILED = 1  # LC_CNT_OUT_FAILED_EVENTS
CONTAINERD, DOCKER = 1, 2
OK, FAIL_TIME, FAIL_SOURCE, FAIL_STREAM, FAIL_JSON = 0, 1, 2, 3, 4
STDERR, PARTIAL, ESCAPED, REPLAY = 1, 2, 4, 8
FORMAT_NAMES = {"1": "containerd_text", "2": "docker_json-file"}


def double():
    vp, cp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    return load_double("container_log_double", ("container_log_double.cpp", "multiline_double.cpp", "processor_parse_container_log_gpu.cpp",
                                                "multiline_events.cpp", "multiline_gpu.cpp", "event_model.cpp"), {
        "cd_process_json_rc": (vp, [vp, cp, ctypes.POINTER(i32), cp, sz]),
        "cd_chain_json": (vp, [vp, vp, cp, cp, sz, ctypes.POINTER(i32), cp, sz]),
        "cd_fail_next_trips": (i32, [i32]),
        "cd_free": (i32, [vp]),
        "cd_parse_one": (None, [i32, cp, u32, u32, cp, u32, vp, vp, vp, vp, vp, vp]),
        "cd_parse_resident": (None, [i32, vp, vp, u32, vp, vp]),
        "cd_parse_stats": (i32, [ctypes.POINTER(ctypes.c_uint64)]),
    }, extra=oracle_link())


def host_parse(fmt, line, head=0, tail=b"", in_place=False):
    """one line through the product's routine on the host -> (status, flags, spans int32[3][2], rewrite_begin, text): text = the shadow
    (pre-filled with 0xA5), or with in_place the line as the reference's in-place rewrite leaves it"""
    L = double()
    st, fl, rb = ctypes.c_uint8(), ctypes.c_uint8(), ctypes.c_int32()
    spans = np.full(8, -7, np.int32)  # one sentinel pair behind the three
    shadow = np.full(len(line) + 2, 0xA5, np.uint8)
    rewritten = np.zeros(len(line) + 1, np.uint8)
    L.cd_parse_one(fmt, line, len(line), head, tail, len(tail), ctypes.byref(st), ctypes.byref(fl), spans.ctypes.data, ctypes.byref(rb),
                   None if in_place or fmt == CONTAINERD else shadow.ctypes.data, rewritten.ctypes.data)
    assert (spans[6:] == -7).all() and (shadow[len(line):] == 0xA5).all(), "the routine wrote behind its results"
    return st.value, fl.value, spans[:6].reshape(3, 2).copy(), rb.value, bytes(rewritten[:len(line)]) if in_place else bytes(shadow[:len(line)])


def _events_of(out_json):
    d = dict(json.loads(out_json, object_pairs_hook=list) or [])
    events = []
    for ev in d.get("events", []):
        ev = dict(ev)
        if ev.get("type") == 1:
            events.append([list(kv) for kv in ev.get("contents", [])])
        else:
            events.append({"content": ev.get("content"), "type": ev.get("type")})
    return events, dict(d.get("metadata", []))


class Product(plugin_double.Product):
    """processor_parse_container_log_gpu of library L (the double by default).  process: (product, group JSON bytes) -> (rc, group
    JSON) and chain: (product, format, read buffer bytes) -> (rc, group JSON), for a library that has no cd_process_json_rc /
    cd_chain_json (the real one goes through lc_group_from_json, and lc_split_lines_device + lc_group_from_lines)"""
    PREFIX = "lc_container_log_processor"

    def __init__(self, config, L=None, process=None, chain=None):
        plugin_double.Product.__init__(self, config, L or double())
        self.L.lc_container_log_processor_set_config_name(self.h, b"test_config")
        self._process, self._chain = process, chain
        self._merge = None

    def __del__(self):
        plugin_double.Product.__del__(self)
        if getattr(self, "_merge", None):
            self.L.lc_merge_multiline_free(self._merge)
            self._merge = None

    def merge_handle(self):
        """the product's flag-mode merge"""
        if not self._merge:
            err = ctypes.create_string_buffer(512)
            m = ctypes.c_void_p()
            cfg = b'{"SourceKey":"content","MergeType":"flag","UnmatchedContentTreatment":"single_line"}'
            assert self.L.lc_merge_multiline_create(cfg, len(cfg), ctypes.byref(m), err, 512) == 0, err.value
            self._merge = m
        return self._merge

    def process_group_rc(self, group, fmt, chain=False):
        """(the processor's return code, the events left, the group's metadata as the fixture writer names it).  chain: the group is ONE
        read buffer; the product's line split in front, its flag-mode merge behind"""
        err = ctypes.create_string_buffer(512)
        c_rc = ctypes.c_int(0)
        if chain:
            (key, buf), = group["events"][0]["contents"]
            assert key == "content" and len(group["events"]) == 1
            data = buf.encode("latin-1")
            if self._chain:
                rc, out = self._chain(self, fmt, data)
            else:
                p = self.L.cd_chain_json(self.h, self.merge_handle(), fmt.encode(), data, len(data), ctypes.byref(c_rc), err, 512)
                assert p, err.value
                try:
                    rc, out = c_rc.value, ctypes.string_at(p).decode("latin-1")
                finally:
                    self.L.cd_free(p)
        else:
            group = dict(group)
            if fmt is not None:
                group["metadata"] = {"container.type": fmt}
            text = json.dumps(group, ensure_ascii=False).encode("latin-1")
            if self._process:
                rc, out = self._process(self, text)
            else:
                p = self.L.cd_process_json_rc(self.h, text, ctypes.byref(c_rc), err, 512)
                assert p, err.value
                try:
                    rc, out = c_rc.value, ctypes.string_at(p).decode("latin-1")
                finally:
                    self.L.cd_free(p)
        events, metadata = _events_of(out)
        return rc, events, metadata

    def counters(self):
        """out_failed, parse_stdout_total, parse_stderr_total"""
        s = (ctypes.c_uint64 * 2)()
        self.L.lc_container_log_processor_stream_counts(self.h, s)
        return [self.counter_values()[OUT_FAILED], int(s[0]), int(s[1])]

    def replayed(self):
        return int(self.L.lc_container_log_processor_replayed_lines(self.h))


def load_fixtures():
    with open(os.path.join(GOLDEN, "container_log_reference_outputs.json")) as f:
        ref = json.load(f)
    with open(os.path.join(GOLDEN, "container_log_unittest_vectors.json")) as f:
        unit = json.load(f)
    return ref, unit


def expand(group):
    """a case's compact group {key, lines, extra} -> one log event {key: line} per line, with extra one event {other: x} behind them"""
    if "lines" not in group:
        return group
    events = [{"contents": [[group["key"], ln]], "timestamp": 1, "type": 1} for ln in group["lines"]]
    if group["extra"]:
        events.append({"contents": [["other", "x"]], "timestamp": 1, "type": 1})
    return {"events": events}


def fixture_runs(ref, unit):
    """-> [(id, config, format, chain, group, expected ref dict)] over both files"""
    runs = [(c["name"], c["config"], c["format"], c.get("chain", False), expand(c["group"]), c["ref"]) for c in ref["cases"]]
    runs += [("unit:" + c["name"], c["config"], c["format"], c["chain"], c["in"], c["ref"]) for c in unit["cases"]]
    return runs


def all_lines(ref, unit):
    """every (format, source value) of both fixture files whose group has one of the two formats, as (int, bytes); chain groups give
    their lines"""
    lines = []
    for _, config, fmt, chain, group, _ in fixture_runs(ref, unit):
        if fmt not in ("1", "2"):
            continue
        key = config.get("SourceKey", "content") if isinstance(config.get("SourceKey", "content"), str) else "content"
        for ev in group.get("events", []):
            for k, v in ev.get("contents", []) if ev.get("type") == 1 else []:
                if k == key:
                    lines += [(int(fmt), ln.encode("latin-1")) for ln in (v.split("\n") if chain else [v])]
    return lines


def check_run(run, L=None, process=None, chain_fn=None):
    """one fixture run through the product; returns (list of disagreements, product)"""
    name, config, fmt, chain, group, want = run
    p = Product(config, L=L, process=process, chain=chain_fn)
    rc, events, metadata = p.process_group_rc(group, fmt, chain)
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
    # (the reference's fixture writer does not show LOG_FORMAT; the stand-in shows it by name)
    shown = dict(metadata)
    if fmt is not None:
        if shown.pop("container.type", None) != FORMAT_NAMES.get(fmt, fmt):
            bad.append("%s: container.type is shown as %r" % (name, metadata.get("container.type")))
    if shown != want["metadata"]:
        bad.append("%s: metadata %r != reference %r" % (name, shown, want["metadata"]))
    if p.counters() != want["counters"]:
        bad.append("%s: counters %r != reference %r" % (name, p.counters(), want["counters"]))
    if [m for k, m in p.alarms if k == 0] != want["alarms"]:
        bad.append("%s: alarms %r != reference %r" % (name, p.alarms, want["alarms"]))
    return bad, p
