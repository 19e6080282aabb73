"""processor_parse_timestamp_gpu on the device: strptime_kernel over every floor vector of tests/golden/timestamp_strptime_vectors.json
(the reference's own strptime_ns), the processor over every group of tests/golden/timestamp_unittest_vectors.json against the model,
64 Ki random values per format against the model, the fused path (regex parse -> timestamp with the capture table left in device
memory) against the two-step path, and sentinel-guarded outputs."""
import ctypes
import json
import os
import random
import time

import numpy as np
import pytest

from helpers import fresh_thread
from helpers import timestamp_model as model
from helpers.timestamp_double import INT_MIN, LC_TS_ABSENT, LC_TS_EPOCH, LC_TS_HAS_YEAR, LC_TS_OK, Product, check_vector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "timestamp_strptime_vectors.json")) as _f:
    _GOLD = json.load(_f)
VECTORS, TZS = _GOLD["vectors"], _GOLD["tz"]
with open(os.path.join(ROOT, "tests", "golden", "timestamp_unittest_vectors.json")) as _f:
    UNIT = json.load(_f)
KEYS = ("status", "secs", "nanos", "matched", "frac_len", "same_as_prev")


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _upload(torch, values, pad_front=0):
    """values back to back behind pad_front bytes -> (d_data, d_off i32[n], d_spans i32[n, 2])"""
    blob = b"#" * pad_front + b"".join(values)
    data = np.frombuffer(blob + b"\0" * (16 - len(blob) % 16), np.uint8).copy()
    off = np.zeros(len(values), np.int32)
    lens = np.array([len(v) for v in values], np.int32)
    off[:] = pad_front + np.concatenate(([0], np.cumsum(lens)[:-1]))
    spans = np.stack([np.zeros(len(values), np.int32), lens], axis=1)
    dev = torch.device("cuda:0")
    return torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(spans.copy()).to(dev)


def _model_row(fmt, value):
    """what the kernel must report for one value, from the model: (ok, has_year, epoch, secs, nanos, matched, frac_len)"""
    matched, tm, ns, ns_len, epoch = model.strptime_ns(value, fmt)
    ok = matched >= 0
    tod = tm["hour"] * 3600 + tm["min"] * 60 + tm["sec"]
    if epoch is not None:
        secs, has_year = epoch, True
    elif tm["year"] != INT_MIN:
        y, m = tm["year"] + 1900, tm["mon"] + 1   # days from civil (proleptic Gregorian), first of the month
        y -= m <= 2
        era = y // 400
        yoe = y - era * 400
        doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5
        days = era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719468
        secs, has_year = (days + tm["mday"] - 1) * 86400 + tod, True
    else:
        secs, has_year = tm["mon"] << 40 | tm["mday"] << 32 | tod, False
    return ok, has_year, epoch is not None, secs, ns, matched if ok else 0, max(ns_len, 0) if ok else 0


def test_kernel_floor_vectors():
    torch = _torch()
    from loongcollector_amd import binding, timestamp
    by_format = {}
    for v in VECTORS:
        by_format.setdefault(v["format"], []).append(v)
    bad = []
    binding.launched_kernels()
    for fmt, vecs in by_format.items():
        values = [v["value"].encode("latin-1") for v in vecs]
        t = timestamp.GpuStrptime(fmt)
        d_data, d_off, d_spans = _upload(torch, values, pad_front=3)
        out = t.device_outputs(len(values), d_data.device)
        t.parse_spans_device(d_data, d_off, d_spans, len(values), out)
        torch.cuda.synchronize()
        res = {k: out[k].cpu().numpy() for k in KEYS}
        res["nanos"] = res["nanos"].view(np.uint32)
        host = t.parse_host(values)  # the same values through the pinned staging
        for i, v in enumerate(vecs):
            got = tuple(int(res[k][i]) for k in KEYS[:5])
            for b in check_vector(v, got):
                bad.append((fmt, v["value"], b))
            assert got == tuple(int(host[k][i]) for k in KEYS[:5]), (fmt, v["value"])
            assert int(res["same_as_prev"][i]) == int(host["same_as_prev"][i]), (fmt, v["value"])
    assert "strptime_kernel" in binding.launched_kernels()
    assert not bad, bad[:10]


@pytest.mark.parametrize("zone", TZS)
def test_processor_groups_on_device(zone):
    _torch()
    from loongcollector_amd import timestamp
    from loongcollector_amd.processor import EventGroup
    L = timestamp._lib()

    def run(p, group):
        g = EventGroup(group)
        rc = L.lc_timestamp_processor_process(p.h, g._h)
        assert rc == 0
        return json.loads(g.to_json())
    old = os.environ.get("TZ")
    os.environ["TZ"] = zone
    time.tzset()
    L.lc_timestamp_zone_reset()
    try:
        for case in UNIT["groups"]:
            cfg, now = case["config"], case["now"]
            p = Product(cfg, now=now, L=L, process=run)
            p.set_discard(case.get("discard", True), case.get("interval", 43200))
            m = model.Processor(cfg, now, discard=case.get("discard", True), interval=case.get("interval", 43200))
            for values in case["groups"]:
                assert p.process_values(values) == m.process_values(values), (zone, cfg, values)
            assert p.counters() == m.counters and p.alarms == m.alarms, (zone, cfg)
            if zone in case.get("expect", {}):
                p2 = Product(cfg, now=now, L=L, process=run)
                p2.set_discard(case.get("discard", True), case.get("interval", 43200))
                assert [list(x) for x in p2.process_values(case["groups"][0])] == case["expect"][zone]
        for case in UNIT["unit_test_literals"]:  # the reference's unit-test cases with the seconds it states
            if zone not in case["zones"]:
                continue
            p = Product(case["config"], now=case["now"], L=L, process=run)
            p.set_discard(False)
            assert [list(x) for x in p.process_values(case["values"])] == case["expect"], (zone, case["from"])
    finally:
        if old is None:
            os.environ.pop("TZ", None)
        else:
            os.environ["TZ"] = old
        time.tzset()
        L.lc_timestamp_zone_reset()


MONTHS = ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"]


def _random_value(rng, fmt):
    y, mo, d = rng.choice([1970, 1999, 2000, 2023, 2024, 2100, rng.randrange(1, 10000)]), rng.randrange(1, 13), rng.randrange(1, 32)
    h, mi, s = rng.randrange(24), rng.randrange(60), rng.randrange(62)
    if fmt == "%Y-%m-%d %H:%M:%S.%f":
        v = "%04d-%02d-%02d %02d:%02d:%02d.%s" % (y, mo, d, h, mi, s, str(rng.randrange(10 ** rng.randrange(1, 12))))
    elif fmt == "%d/%b/%Y:%H:%M:%S %z":
        v = "%02d/%s/%04d:%02d:%02d:%02d %s" % (d, rng.choice([MONTHS[mo - 1], MONTHS[mo - 1].upper()]), y, h, mi, s,
                                                rng.choice(["+0800", "-0330", "Z", "EDT", "+05:45", "GMT", "PST", "K"]))
    elif fmt == "%b %d %H:%M:%S":
        v = "%s %2d %02d:%02d:%02d" % (MONTHS[mo - 1], d, h, mi, s)
    elif fmt == "%s":
        v = str(rng.randrange(10 ** rng.randrange(1, 21)))
    else:
        v = "%02d%02d%02d %d:%02d:%02d %s" % (y % 100, mo, d, h % 12 + 1, mi, s, rng.choice(["AM", "pm", "Pm"]))
    r = rng.random()
    if r < 0.1:
        k = rng.randrange(len(v))
        v = v[:k] + rng.choice("x:/ 9-") + v[k + 1:]
    elif r < 0.15:
        v = v[:rng.randrange(len(v) + 1)]
    return v.encode()


@pytest.mark.parametrize("fmt", ["%Y-%m-%d %H:%M:%S.%f", "%d/%b/%Y:%H:%M:%S %z", "%b %d %H:%M:%S", "%s", "%y%m%d %I:%M:%S %p"])
def test_random_values_against_model(fmt):
    torch = _torch()
    from loongcollector_amd import timestamp
    rng = random.Random(len(fmt) * 7919)
    n = 64 * 1024
    distinct = [_random_value(rng, fmt) for _ in range(4096)]
    values = []
    while len(values) < n:   # runs of equal values and fresh ones, so that same_as_prev has both answers
        v = rng.choice(distinct)
        values.extend([v] * rng.choice([1, 1, 1, 2, 5]))
    values = values[:n]
    t = timestamp.GpuStrptime(fmt)
    d_data, d_off, d_spans = _upload(torch, values)
    out = t.device_outputs(n, d_data.device)
    t.parse_spans_device(d_data, d_off, d_spans, n, out)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in KEYS}
    res["nanos"] = res["nanos"].view(np.uint32)
    want = {v: _model_row(fmt, v) for v in set(values)}
    prev = None
    for i, v in enumerate(values):
        ok, has_year, epoch, secs, ns, matched, flen = want[v]
        st = int(res["status"][i])
        assert bool(st & LC_TS_OK) == ok and bool(st & LC_TS_HAS_YEAR) == has_year and bool(st & LC_TS_EPOCH) == epoch, (fmt, v)
        assert (int(res["secs"][i]), int(res["matched"][i]), int(res["frac_len"][i])) == (secs, matched, flen), (fmt, v)
        if ok:
            assert int(res["nanos"][i]) == ns, (fmt, v)
        same = bool(prev is not None and ok and want[prev][0] and matched - flen == want[prev][5] - want[prev][6]
                    and v[:matched - flen] == prev[:matched - flen])
        assert bool(res["same_as_prev"][i]) == same, (fmt, i, prev, v)
        prev = v


def test_fused_regex_then_timestamp_equals_two_steps():
    """the capture table of lc_regex_match_device stays in device memory and feeds the timestamp kernel on the same stream"""
    torch = _torch()
    from loongcollector_amd import binding, corpus, timestamp
    n = 8192
    data, off, length = corpus.apache_batch(n, "A", poison_every=13)
    rx = binding.GpuRegex(corpus.REGEX_A)
    G = rx.groups
    dev = torch.device("cuda:0")
    d_data = torch.from_numpy(data).to(dev)
    d_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    d_caps = torch.empty((n, 2 * G), dtype=torch.int32, device=dev)
    d_status = torch.empty((n,), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    fmt = "%d/%b/%Y:%H:%M:%S"
    t = timestamp.GpuStrptime(fmt)
    # which group holds the time: the one whose first capture looks like dd/Mon/yyyy
    rx.match_device(d_data, d_off, None, n, d_caps, d_status, sep_bytes=1, stream=stream)
    torch.cuda.synchronize()
    caps, status = d_caps.cpu().numpy(), d_status.cpu().numpy()
    first = int(np.nonzero(status == 1)[0][0])
    line0 = bytes(data[off[first]:off[first] + length[first]])
    group = next(g for g in range(G) if len(line0[caps[first, 2 * g]:caps[first, 2 * g + 1]]) > 11 and line0[caps[first, 2 * g] + 2:caps[first, 2 * g] + 3] == b"/")
    # fused: both launches queued back to back, nothing read in between
    out = t.device_outputs(n, dev)
    rx.match_device(d_data, d_off, None, n, d_caps, d_status, sep_bytes=1, stream=stream)
    t.parse_captures_device(d_data, d_off, d_caps, G, group, d_status, 1, n, out, stream=stream)
    torch.cuda.synchronize()
    fused = {k: out[k].cpu().numpy() for k in KEYS}
    # two steps: the spans come to the host, the values go up again on their own
    matched_lines = np.nonzero(status == 1)[0]
    values = [bytes(data[off[i] + caps[i, 2 * group]:off[i] + caps[i, 2 * group + 1]]) for i in matched_lines]
    two = t.parse_host(values)
    assert len(matched_lines) == n - len(range(0, n, 13))
    for k in KEYS[:5]:
        assert np.array_equal(fused[k][matched_lines].view(two[k].dtype), two[k]), k
    assert np.all(fused["status"][status != 1] == LC_TS_ABSENT)
    assert np.all(fused["status"][matched_lines] & LC_TS_OK)
    ok, has_year, epoch, secs, ns, m, fl = _model_row(fmt, values[0])
    assert int(two["secs"][0]) == secs and ok


def test_outputs_are_sentinel_guarded():
    """n values in buffers of n + 64 entries painted with a sentinel: entries at and behind n stay as they were; n on both sides of a
    workgroup's 255 new values"""
    torch = _torch()
    from loongcollector_amd import timestamp
    t = timestamp.GpuStrptime("%Y-%m-%d %H:%M:%S")
    dev = torch.device("cuda:0")
    for n in (1, 254, 255, 256, 510, 511, 1000):
        values = [b"2023-12-25 01:02:%02d" % (i % 60) for i in range(n)]
        d_data, d_off, d_spans = _upload(torch, values, pad_front=5)
        out = {k: torch.full((n + 64,), 0x5A, dtype=v.dtype, device=dev) for k, v in t.device_outputs(1, dev).items()}
        t.parse_spans_device(d_data, d_off, d_spans, n, out)
        torch.cuda.synchronize()
        for k in KEYS:
            a = out[k].cpu().numpy()
            assert np.all(a[n:] == 0x5A), (n, k)
        assert np.all(out["status"].cpu().numpy()[:n] == (LC_TS_OK | LC_TS_HAS_YEAR)), n
        secs = out["secs"].cpu().numpy()[:n]
        assert np.array_equal(secs, 1703466120 + np.arange(n) % 60), n
        assert not out["same_as_prev"].cpu().numpy()[:n].any(), n  # neighbours always differ in their seconds


def test_slot_builds_the_timestamp_processor():
    _torch()
    from loongcollector_amd import binding
    from loongcollector_amd.processor import EventGroup
    L = binding.load()

    class Instance(ctypes.Structure):
        _fields_ = [("plugin", ctypes.c_void_p), ("plugin_state", ctypes.c_void_p)]

    class Interface(ctypes.Structure):
        _fields_ = [("version", ctypes.c_int), ("name", ctypes.c_char_p), ("language", ctypes.c_char_p),
                    ("init", ctypes.CFUNCTYPE(ctypes.c_int, ctypes.POINTER(Instance), ctypes.c_void_p, ctypes.c_void_p)),
                    ("finalize", ctypes.CFUNCTYPE(None, ctypes.c_void_p)), ("process", ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p))]
    iface = Interface.in_dll(L, "processor_interface")
    ins = Instance()
    cfg = json.dumps({"Type": "processor_parse_timestamp_gpu", "SourceKey": "time", "SourceFormat": "%s"}).encode()
    assert iface.init(ctypes.byref(ins), ctypes.c_char_p(cfg), None) == 0
    now = int(time.time())
    g = EventGroup({"events": [{"contents": {"time": str(now - 5)}, "timestamp": 1, "type": 1}]})
    iface.process(ins.plugin_state, L.lc_group_native(g._h))
    assert json.loads(g.to_json())["events"][0]["timestamp"] == now - 5
    iface.finalize(ins.plugin_state)


# ---------------------------------------------------------------------------------------------- the host entry's chunk limits
def _host_equals_device(torch, fmt, values):
    """lc_strptime_parse_host against lc_strptime_parse_spans_device over the same packed values, all six arrays"""
    from loongcollector_amd import timestamp
    t = timestamp.GpuStrptime(fmt)
    d_data, d_off, d_spans = _upload(torch, values)
    out = t.device_outputs(len(values), d_data.device)
    t.parse_spans_device(d_data, d_off, d_spans, len(values), out)
    torch.cuda.synchronize()
    host = t.parse_host(values)
    for k in KEYS:
        assert np.array_equal(out[k].cpu().numpy().view(host[k].dtype), host[k]), k
    return host


def test_parse_host_second_chunk_behind_two_to_the_20_values_starts_one_value_early():
    torch = _torch()
    n = (1 << 20) + 1
    values = [b"%d" % (1700000000 + (i + 1) // 2) for i in range(n)]      # equal pairs (1, 2), (3, 4) .. (2^20 - 1, 2^20)
    assert values[n - 1] == values[n - 2] != values[n - 3]
    host = _host_equals_device(torch, "%s", values)
    assert host["same_as_prev"][n - 1] == 1 and host["same_as_prev"][n - 2] == 0 and host["same_as_prev"][:5].tolist() == [0, 0, 1, 0, 1]
    assert int(host["secs"][n - 1]) == 1700000000 + (1 << 19) and np.all(host["status"] & LC_TS_OK)


def test_parse_host_forty_values_of_one_mib_cross_the_payload_limit():
    torch = _torch()
    values = []
    for i in range(40):
        values += [b"%d" % (1700000000 + i // 2) + b"x" * ((1 << 20) - 10), b"%d" % (1700000000 + i), b"%d" % (1700000000 + i)]
    host = _host_equals_device(torch, "%s", values)
    assert host["secs"][:6].tolist() == [1700000000, 1700000000, 1700000000, 1700000000, 1700000001, 1700000001]
    assert host["matched"][:3].tolist() == [10, 10, 10] and host["same_as_prev"][:6].tolist() == [0, 1, 1, 1, 0, 1]


def test_parse_host_after_thread_release_gives_the_same_answer():
    _torch()
    from loongcollector_amd import binding, timestamp
    t = timestamp.GpuStrptime("%Y-%m-%d %H:%M:%S")
    values = [b"2023-12-25 01:02:03", b"2023-12-25 01:02:03", b"x", b""]

    def body():
        first = t.parse_host(values)
        binding.load().lc_thread_release()
        return first, t.parse_host(values), binding.load().lc_last_error()

    first, second, error = fresh_thread.run(body)
    assert all(np.array_equal(first[k], second[k]) for k in KEYS) and first["secs"][:2].tolist() == [1703466123] * 2
    assert first["same_as_prev"].tolist() == [0, 1, 0, 0] and not error


def test_four_threads_share_one_processor():
    """three groups of 64 events per thread: 62 values (runs of three equal seconds), one that does not parse and one event without the
    key"""
    _torch()
    from loongcollector_amd import timestamp
    from helpers.shared_processor import four_threads_equal_one_thread
    base = 1703466123      # 2023-12-25 01:02:03 UTC

    def log(contents):
        return {"contents": contents, "timestamp": 1, "type": 1}

    def group(t, g):
        events = [log({"time": time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime(base + 1000 * t + 100 * g + i // 3))}) for i in range(62)]
        # (at the head of a run: behind a value that does not parse, a value equal to the one before it would hit the string cache and take
        # the second the failed parse left behind, as in the reference)
        events.insert(g * 21 + 3 * t, log({"time": "garbage"}))
        return {"events": events + [log({"other": "x"})]}

    def make():
        p = timestamp.TimestampProcessor({"SourceKey": "time", "SourceFormat": "%Y-%m-%d %H:%M:%S"}, clock=lambda: base)
        p.set_discard(False)
        return p

    groups = [[group(t, g) for g in range(3)] for t in range(4)]
    L = timestamp._lib()
    old = os.environ.get("TZ")
    os.environ["TZ"] = "UTC"
    time.tzset()
    L.lc_timestamp_zone_reset()
    try:
        want, c = four_threads_equal_one_thread(make, groups)
    finally:
        if old is None:
            os.environ.pop("TZ", None)
        else:
            os.environ["TZ"] = old
        time.tzset()
        L.lc_timestamp_zone_reset()
    stamps = [e["timestamp"] for e in want[2][1]]
    assert stamps == [base + 2100 + i // 3 for i in range(27)] + [1] + [base + 2100 + i // 3 for i in range(27, 62)] + [1]
    assert [c[k] for k in ("discarded_events_total", "out_failed_events_total", "out_key_not_found_events_total", "out_successful_events_total",
                           "in_events_total", "out_events_total", "history_failure_total")] == [0, 12, 12, 12 * 62, 12 * 64, 12 * 64, 0]
