"""The real library and the ten host doubles in ONE process (what two prototype copies of one entry point used to forbid): each of the
seven plugin classes over a three-event group from its own golden fixture gives what its double gives for the same group, and each
engine host entry crosses the wrapper with a real pointer in every argument.  Nothing about the kernels is at stake here."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LINES = [b"", b"0123456789abcde", b"0123456789abcdefg"]   # 0, 15 and 17 bytes
FILL = 0xA5


@pytest.fixture(scope="module")
def doubles():
    from helpers.all_doubles import load_all
    from loongcollector_amd import binding
    loaded = load_all()
    assert len(loaded) == 10 and binding.load().lc_desens_apply_host.argtypes[-1] is loaded["desensitize"].lc_desens_apply_host.argtypes[-1]
    return loaded


def _golden(name):
    with open(os.path.join(GOLDEN, name), encoding="utf-8") as f:
        return json.load(f)


def _log_group(lines, key="content"):
    return {"events": [{"contents": [[key, ln]], "timestamp": 1, "type": 1} for ln in lines]}


def _pairs(group_json):
    """a group's JSON -> per event its contents as an ordered list of [key, value]"""
    d = dict(json.loads(group_json, object_pairs_hook=list) or [])
    return [[list(kv) for kv in dict(ev).get("contents", [])] for ev in d.get("events", [])]


def _delimiter():
    import test_delimiter_host
    from loongcollector_amd import delimiter
    from loongcollector_amd.processor import EventGroup
    case = next(c for c in _golden("delimiter_reference_outputs.json")["cases"] if len(c["lines"]) >= 3 and len(c["out"]) >= 3)
    group = _log_group(case["lines"][:3])
    want = [ev["contents"] for ev in test_delimiter_host.Product(case["config"]).process_group(group)]
    g = EventGroup(json.dumps(group))
    delimiter.DelimiterProcessor(case["config"]).process(g)
    return want, _pairs(g.to_json())


def _json():
    import test_json_host
    from helpers import json_cases as jc
    from loongcollector_amd import json_parse
    from loongcollector_amd.processor import EventGroup
    text = lambda ev: {jc.expand(k).decode("latin-1"): jc.expand(v).decode("latin-1") for k, v in ev.items()}      # noqa: E731
    ascii_only = lambda ev: all(max(k.encode("latin-1") + v.encode("latin-1") + b" ") < 128 for k, v in ev.items())      # noqa: E731
    cases = jc.unittest_doc()["cases"]
    case = next(c for c in cases if c["expect"] and all(ascii_only(text(ev)) for ev in c["in"]))
    events = [text(ev) for ev in case["in"]]
    group = {"events": [{"contents": events[i % len(events)], "timestamp": 12345678901, "type": 1} for i in range(3)]}
    want = [ev.get("contents", {}) for ev in test_json_host.Product(case["config"]).process_group(group)]
    g = EventGroup(group)
    json_parse.JsonProcessor(case["config"]).process(g)
    return want, [ev.get("contents", {}) for ev in g.to_dict()["events"]]


def _timestamp():
    from helpers import timestamp_double
    from loongcollector_amd import timestamp
    from loongcollector_amd.processor import EventGroup
    case = next(c for c in _golden("timestamp_unittest_vectors.json")["groups"] if len(c["groups"][0]) >= 3)
    values, key = case["groups"][0][:3], case["config"]["SourceKey"]
    double = timestamp_double.Product(case["config"], now=case["now"])
    double.set_discard(case.get("discard", True), case.get("interval", 43200))
    want = double.process_values(values, key=key)
    p = timestamp.TimestampProcessor(case["config"], clock=lambda: case["now"])
    p.set_discard(case.get("discard", True), case.get("interval", 43200))
    g = EventGroup({"events": [{"contents": {key: v}, "timestamp": 1, "type": 1} for v in values]})
    p.process(g)
    return want, [(ev["contents"][key], ev["timestamp"], ev.get("timestampNanosecond")) for ev in g.to_dict()["events"]]


def _apsara():
    from helpers import apsara_double as ad
    from loongcollector_amd import apsara
    from loongcollector_amd.processor import EventGroup
    ref = _golden("apsara_reference_outputs.json")
    case = next(c for c in ref["cases"] if len(c["lines"]) >= 3)
    group = _log_group(case["lines"][:3])
    double = ad.Product(case["config"], now=ref["now"])
    double.set_discard(case["discard"])
    rc, want = double.process_group_rc(group)
    assert rc == 0
    p = apsara.ApsaraProcessor(case["config"], clock=lambda: ref["now"])
    p.set_discard(case["discard"])
    g = EventGroup(json.dumps(group, ensure_ascii=False))
    p.process(g)
    got = []
    for ev in dict(json.loads(g.to_json(), object_pairs_hook=list)).get("events", []):
        ev = dict(ev)
        got.append({"contents": [list(kv) for kv in ev.get("contents", [])], "ts": ev.get("timestamp"), "ns": ev.get("timestampNanosecond", 0)})
    return want, got


def _container_log():
    from helpers import container_log_product as cp
    from loongcollector_amd import container_log
    from loongcollector_amd.processor import EventGroup
    ref = _golden("container_log_reference_outputs.json")
    case = next(c for c in ref["cases"] if c["format"] in ("1", "2") and not c.get("chain", False) and len(cp.expand(c["group"])["events"]) >= 3)
    group = dict(cp.expand(case["group"]))
    group["events"] = group["events"][:3]
    rc, want, want_meta = cp.Product(case["config"]).process_group_rc(group, case["format"])
    assert rc == 0
    p = container_log.ContainerLogProcessor(case["config"], config_name="test_config")
    g = EventGroup(json.dumps(dict(group, metadata={"container.type": case["format"]}), ensure_ascii=False))
    p.process(g)
    got, got_meta = cp._events_of(g.to_json())
    return (want, want_meta), (got, got_meta)


def _desensitize():
    from helpers import desensitize_product as dp
    from loongcollector_amd import desensitize
    from loongcollector_amd.processor import EventGroup
    case = next(c for c in dp.load_fixtures()["cases"] if any(s["kind"] == "desensitize" for s in c["stages"]))
    config = next(s["config"] for s in case["stages"] if s["kind"] == "desensitize")
    events = case["at_desensitize"]["events"]
    group = {"events": [events[i % len(events)] for i in range(3)]}
    rc, want = dp.Product(config).process(group)
    assert rc == 0
    g = EventGroup(group)
    desensitize.DesensitizeProcessor(config).process(g)
    contents = lambda d: [ev.get("contents", ev.get("content")) for ev in d["events"]]      # noqa: E731
    return contents(want), contents(g.to_dict())


def _prom():
    from helpers import prom_product as pp
    from loongcollector_amd import prom
    ref, _ = pp.load_fixtures()
    lines = [c["line"].encode("latin-1") for c in ref["cases"] if c["ok"] and c.get("tags")][:3]
    assert len(lines) == 3
    config = {"job_name": "j", "honor_timestamps": True}
    rc, want = pp.Product(config).process(lines, 1700000000123)
    assert rc == 0 and len(want) == 3
    group = prom.RawGroup(lines, 1700000000123)
    prom.PromProcessor(config).process(group)
    metric = lambda ev: (ev["type"], ev["name"], ev["tags"], ev["bits"], ev["secs"], ev["nanos"])      # noqa: E731
    return [metric(ev) for ev in want], [metric(ev) for ev in group.events()]


@pytest.mark.parametrize("plugin", [_delimiter, _json, _timestamp, _apsara, _container_log, _desensitize, _prom], ids=lambda f: f.__name__[1:])
def test_plugin_class_equals_its_double_beside_all_ten_doubles(doubles, plugin):
    want, got = plugin()
    assert want and got == want


def _packed():
    """LINES as the host entries take them -> (array of line addresses, uint32 lengths, the blob that keeps them alive)"""
    blob = np.frombuffer(b"".join(LINES) + b"\0", np.uint8).copy()
    lens = np.array([len(v) for v in LINES], np.uint32)
    at = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    return (blob.ctypes.data + at).astype(np.uint64), lens, blob


def _filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def test_engine_host_entries_cross_the_wrapper_with_real_pointers(doubles):
    from loongcollector_amd import abi, apsara, binding, container_log, delimiter, desensitize, json_parse, prom, timestamp
    L = binding.load()
    ptrs, lens, blob = _packed()
    n, W = len(LINES), 4
    # lc_delim_split_host
    dl = delimiter.GpuDelimiter(b",", b'"', "extend", 2)
    status, ncols, spans = _filled(n, np.uint8), _filled(n, np.uint32), _filled((n, W, 2), np.int32)
    binding._check(L.lc_delim_split_host(dl.handle, ptrs.ctypes.data, lens.ctypes.data, n, W, status.ctypes.data, ncols.ctypes.data, spans.ctypes.data),
                   "lc_delim_split_host")
    assert not (status == FILL).any()
    # lc_strptime_parse_host
    ts = timestamp.GpuStrptime("%Y")
    res = {k: _filled(n, t) for k, t in zip(abi.TS_OUT_KEYS, (np.uint8, np.int64, np.uint32, np.int32, np.int32, np.uint8))}
    o = abi.LcTsOut(*(res[k].ctypes.data for k in abi.TS_OUT_KEYS))
    binding._check(L.lc_strptime_parse_host(ts.handle, ptrs.ctypes.data, lens.ctypes.data, n, ctypes.byref(o)), "lc_strptime_parse_host")
    assert not (res["status"] == FILL).any()
    # lc_json_walk_host
    st, nm, err = _filled(n, np.uint8), _filled(n, np.uint32), _filled(n, np.uint32)
    rec, shadow, moved = _filled((n, W), json_parse.MEMBER), _filled(len(blob), np.uint8), ctypes.c_uint64(0)
    binding._check(L.lc_json_walk_host(ptrs.ctypes.data, lens.ctypes.data, n, W, st.ctypes.data, nm.ctypes.data, err.ctypes.data, rec.ctypes.data,
                                       shadow.ctypes.data, ctypes.byref(moved)), "lc_json_walk_host")
    assert not (st == FILL).any()
    # lc_apsara_parse_host, lc_container_log_parse_host, lc_prom_parse_host: the package's wrappers pre-fill their arrays
    ap = apsara.parse_host(LINES, W, fill=FILL)
    assert not (ap["status"] == FILL).any()
    cl = container_log.parse_host(container_log.LC_CLOG_CONTAINERD, LINES, fill=FILL)
    assert not (cl["status"] == FILL).any()
    pm = prom.parse_host(LINES, True, W, fill=FILL)
    assert not (pm["status"] == FILL).any()
    # lc_desens_apply_host
    new, flags, stats = desensitize.GpuDesensitize("const", "9a", "bc", "#").apply_host(LINES)
    assert new == [None, b"0123456789a#de", b"0123456789a#defg"] and list(flags) == [0, desensitize.LC_DESENS_CHANGED, desensitize.LC_DESENS_CHANGED]
    assert stats["rounds"] == 1
