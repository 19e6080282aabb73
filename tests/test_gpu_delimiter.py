"""The delimiter parser on the device (include/lc_delimiter.h): delim_split_kernel against tests/helpers/delimiter_model.py -- which
tests/test_delimiter_model.py holds to the reference's own output -- and processor_parse_delimiter_gpu against
tests/golden/delimiter_reference_outputs.json itself."""
import json
import os
import random
import threading

import numpy as np
import pytest

from helpers import fresh_thread
from helpers.delimiter_model import Engine

pytestmark = pytest.mark.gpu

CONFIGS = [(b",", b'"', "extend", 10), (b"|", b"'", "keep", 4), (b"\t", b"\t", "discard", 3), (b"||", b'"', "keep", 3), (b"@@@@", b'"', "extend", 5)]


def _batch(rng, sep, quote, n, max_len=4096):
    """n random lines, lengths 0 .. max_len: plain and quoted fields, empty columns, doubled quotes, stray quotes, blanks and \\r at
    both ends, up to 40 columns, all-blank and empty lines"""
    lines = []
    pool = bytes(rng.choice(b"abcdefgh 0123456789.-/") for _ in range(1 << 16))
    for i in range(n):
        kind = rng.random()
        if kind < 0.02:
            lines.append(b"" if rng.random() < 0.5 else b" " * rng.randrange(1, 40) + b"\r" * rng.randrange(0, 3))
            continue
        target = rng.choice([rng.randrange(0, 64), rng.randrange(0, 600), rng.randrange(0, max_len)]) if kind < 0.9 else rng.randrange(0, 100)
        fields = []
        size = 0
        ncols = rng.randrange(1, 41) if kind < 0.5 else rng.randrange(1, 8)
        while len(fields) < ncols and size < target:
            width = rng.randrange(0, max(2, target // max(1, ncols) * 2))
            at = rng.randrange(0, len(pool) - 4096)
            body = pool[at:at + width]
            r = rng.random()
            if r < 0.2:
                inner = body.replace(quote, b"") + (sep if rng.random() < 0.5 else b"") + (quote + quote if rng.random() < 0.4 else b"")
                body = quote + inner + quote
            elif r < 0.205:
                body = body[: len(body) // 2] + quote + body[len(body) // 2:]          # a stray quote
            elif r < 0.21:
                body = quote + body                                                    # an unterminated quote
            elif r < 0.215:
                body = quote + body.replace(quote, b"") + quote + b"x"                 # data behind a closing quote
            fields.append(body)
            size += len(body) + len(sep)
        line = sep.join(fields)[:max_len - 8]
        line = b" " * rng.choice([0, 0, 1, 3]) + line + rng.choice([b"", b"", b" ", b"\r", b" \r ", sep])
        lines.append(line)
    return lines


def _pack(lines):
    off = np.zeros(len(lines) + 1, np.int32)
    if lines:
        off[1:] = np.cumsum([len(ln) for ln in lines])
    data = np.frombuffer(b"".join(lines) or b"\0", np.uint8).copy()
    return data, off


def _device_split(dl, lines, W):
    import torch
    dev = torch.device("cuda:0")
    data, off = _pack(lines)
    n = len(lines)
    d_data = torch.from_numpy(data).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_st = torch.full((max(n, 1),), 77, dtype=torch.uint8, device=dev)
    d_nc = torch.full((max(n, 1),), -5, dtype=torch.int32, device=dev)
    d_sp = torch.full((max(n, 1), W, 2), -9, dtype=torch.int32, device=dev)
    dl.split_device(d_data, d_off, n, W, d_st, d_nc, d_sp, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy()[:n], d_nc.cpu().numpy()[:n].astype(np.int64), d_sp.cpu().numpy()[:n]


def _check(model, lines, st, nc, sp, W):
    for i, ln in enumerate(lines):
        status, count, cols = model.split_line(ln)
        assert (int(st[i]), int(nc[i])) == (status, count), (i, ln[:200])
        for c, (b, e, doubled) in enumerate(cols[:W]):
            assert (int(sp[i, c, 0]) & 0x7FFFFFFF, int(sp[i, c, 1]), bool(sp[i, c, 0] < 0)) == (b, e, doubled), (i, c, ln[:200])


@pytest.mark.parametrize("k", range(len(CONFIGS)))
def test_engine_64_ki_random_lines_equal_the_model_and_wide_lines_take_the_mop_up(k):
    from loongcollector_amd import delimiter
    sep, quote, mode, nk = CONFIGS[k]
    rng = random.Random(1000 + k)
    lines = _batch(rng, sep, quote, 65536)
    model = Engine(sep, quote, mode, nk)
    dl = delimiter.GpuDelimiter(sep, quote, mode, nk)
    W = nk + 10 if mode == "extend" else nk + 1
    st, nc, sp = _device_split(dl, lines, W)
    _check(model, lines, st, nc, sp, W)
    # the mop-up: the kernel reported the TRUE count of the lines that did not fit; they run again, once, with room for the widest
    wide = [i for i in range(len(lines)) if nc[i] > W]
    if mode == "extend" or model.use_quote:
        assert len(wide) > 100
    if wide:
        W2 = int(max(nc[i] for i in wide))
        sub = [lines[i] for i in wide]
        st2, nc2, sp2 = _device_split(dl, sub, W2)
        _check(model, sub, st2, nc2, sp2, W2)
        assert all(int(nc2[j]) == int(nc[i]) for j, i in enumerate(wide))


def test_engine_batches_of_one_and_of_zero_lines_and_a_64_kib_line():
    from loongcollector_amd import delimiter
    dl = delimiter.GpuDelimiter(b",", b'"', "extend", 3)
    model = Engine(b",", b'"', "extend", 3)
    st, nc, sp = _device_split(dl, [], 4)
    assert len(st) == 0
    for one in (b"a,b,c", b"", b'"x,y",z'):
        st, nc, sp = _device_split(dl, [one], 4)
        _check(model, [one], st, nc, sp, 4)
    rng = random.Random(5)
    long_line = b",".join(bytes(rng.choice(b"abcdefgh") for _ in range(rng.randrange(0, 30))) for _ in range(6000))[:65536]
    long_line = long_line + b"x" * (65536 - len(long_line))
    assert len(long_line) == 65536
    lines = [b"k,l", long_line, b'"q""q",r', long_line[:40000] + b'"']
    W = 16
    st, nc, sp = _device_split(dl, lines, W)
    _check(model, lines, st, nc, sp, W)
    assert nc[1] > 4000


def test_split_host_equals_split_device_and_eight_threads_give_the_single_thread_answer():
    from loongcollector_amd import delimiter
    sep, quote, mode, nk = CONFIGS[0]
    rng = random.Random(77)
    lines = _batch(rng, sep, quote, 20000, max_len=1024)
    dl = delimiter.GpuDelimiter(sep, quote, mode, nk)
    W = 12
    st, nc, sp = _device_split(dl, lines, W)
    data, off = _pack(lines)

    def same(hst, hnc, hsp):
        assert np.array_equal(hst, st) and np.array_equal(hnc.astype(np.int64), nc)
        for i in range(len(lines)):
            m = min(int(nc[i]), W)
            assert np.array_equal(hsp[i, :m], sp[i, :m]), i

    same(*dl.split_host(data, off, W))
    # eight threads on ONE handle, each with its own rotation of the lines: a mix-up of two threads' staging would show
    results, errors = [None] * 8, []

    def worker(t):
        try:
            r = (t * 2503) % len(lines)
            mine = lines[r:] + lines[:r]
            d, o = _pack(mine)
            for _ in range(3):
                hst, hnc, hsp = dl.split_host(d, o, W)
            results[t] = (np.roll(hst, r), np.roll(hnc, r), np.roll(hsp, r, axis=0))
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r in results:
        same(*r)


def test_launched_kernels_names_the_delimiter_kernel():
    from loongcollector_amd import binding, delimiter
    dl = delimiter.GpuDelimiter(b",")
    binding.launched_kernels()
    data, off = _pack([b"a,b", b"c"])
    dl.split_host(data, off, 4)
    assert "delim_split_kernel" in binding.launched_kernels()


def test_processor_the_reference_s_recorded_outputs_on_the_device(golden_dir):
    from loongcollector_amd import delimiter
    from loongcollector_amd.processor import EventGroup
    with open(os.path.join(golden_dir, "delimiter_reference_outputs.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 100
    for k, case in enumerate(cases):
        for first_trip in (None, 2):                    # the reference's reserve, and a first trip so small that the mop-up runs
            p = delimiter.DelimiterProcessor(case["config"], first_trip_columns=first_trip or 0)
            alarms = p.collect_alarms()
            events = [{"contents": [["content", ln]], "timestamp": 1, "type": 1} for ln in case["lines"]]
            events.append({"contents": [["other", "x"]], "timestamp": 1, "type": 1})
            g = EventGroup(json.dumps({"events": events}))
            p.process(g)
            got = [[list(kv) for kv in ev] for ev in g.contents()]
            assert got == case["out"], (k, first_trip, case["config"])
            c = p.counters()
            assert [c["discarded_events_total"], c["out_failed_events_total"], c["out_key_not_found_events_total"],
                    c["out_successful_events_total"]] == case["counters"], (k, case["config"])
            assert c["in_events_total"] == len(events) and c["out_events_total"] == len(case["out"]) and c["device_failed_events_total"] == 0
            assert [m.decode("latin-1") for _, m in alarms] == case["alarms"], (k, case["config"])
            g.close()
            p.close()


def test_processor_the_cases_of_the_reference_s_unit_test_on_the_device(golden_dir):
    from loongcollector_amd import delimiter
    from loongcollector_amd.processor import EventGroup
    with open(os.path.join(golden_dir, "delimiter_unittest_vectors.json"), encoding="utf-8") as f:
        doc = json.load(f)
    assert len(doc["cases"]) >= 30
    names = {"mDiscardedEventsTotal": "discarded_events_total", "mOutFailedEventsTotal": "out_failed_events_total",
             "mInEventsTotal": "in_events_total", "mOutEventsTotal": "out_events_total"}
    for case in doc["cases"]:
        for first_trip in (0, 1):
            p = delimiter.DelimiterProcessor(case["config"], first_trip_columns=first_trip)
            alarms = p.collect_alarms()
            g = EventGroup(json.dumps(case["in"]))
            p.process(g)
            got = g.to_dict() or {}
            norm = lambda ev: (ev.get("contents", {}), ev.get("timestamp"), ev.get("timestampNanosecond", 0), ev.get("type"))   # noqa: E731
            assert [norm(e) for e in got.get("events", [])] == [norm(e) for e in case["expect"].get("events", [])], case["name"]
            c = p.counters()
            for member, value in case["asserted"].items():
                assert c[names[member]] == value, (case["name"], member)
            assert [c["discarded_events_total"], c["out_failed_events_total"], c["out_key_not_found_events_total"],
                    c["out_successful_events_total"]] == case["reference_counters"], case["name"]
            assert [m.decode("latin-1") for _, m in alarms] == case["reference_alarms"], case["name"]
            g.close()
            p.close()
    for case in doc["init_only"]:
        delimiter.DelimiterProcessor(case["config"]).close()


def test_the_plugin_slot_builds_the_delimiter_parser_for_its_type_name():
    import ctypes
    from loongcollector_amd import processor as proc_mod
    from loongcollector_amd.processor import EventGroup
    L = proc_mod._lib()

    class Iface(ctypes.Structure):
        _fields_ = [("version", ctypes.c_int), ("name", ctypes.c_char_p), ("language", ctypes.c_char_p),
                    ("init", ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p)),
                    ("finalize", ctypes.CFUNCTYPE(None, ctypes.c_void_p)), ("process", ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p))]

    class Instance(ctypes.Structure):
        _fields_ = [("plugin", ctypes.c_void_p), ("plugin_state", ctypes.c_void_p)]

    iface = Iface.in_dll(L, "processor_interface")
    ins = Instance()
    config = {"Type": "processor_parse_delimiter_gpu", "SourceKey": "content", "Separator": ",", "Keys": ["a", "b"]}
    assert iface.init(ctypes.addressof(ins), json.dumps(config).encode(), None) == 0
    g = EventGroup({"events": [{"contents": {"content": '"x,1",y,z'}, "timestamp": 1, "type": 1}]})
    iface.process(ins.plugin_state, L.lc_group_native(g._h))
    assert [[list(kv) for kv in ev] for ev in g.contents()] == [[["a", "x,1"], ["b", "y"], ["__column2__", "z"]]]
    iface.finalize(ins.plugin_state)
    bad = Instance()
    assert iface.init(ctypes.addressof(bad), json.dumps(dict(config, Separator="12345")).encode(), None) != 0 and not bad.plugin_state


# ---------------------------------------------------------------------------------------------- the host entry's chunk limits
def _host_equals_device(dl, lines, W):
    """lc_delim_split_host against lc_delim_split_device over the same packed lines: status, counts and the spans that count"""
    st, nc, sp = _device_split(dl, lines, W)
    data, off = _pack(lines)
    hst, hnc, hsp = dl.split_host(data, off, W)
    assert np.array_equal(hst, st) and np.array_equal(hnc.astype(np.int64), nc)
    kmax = int(min(nc.max(), W))
    live = np.arange(kmax)[None, :] < np.minimum(nc, W)[:, None]
    assert np.array_equal(hsp[:, :kmax][live], sp[:, :kmax][live])
    return hst, hnc, hsp


def test_split_host_second_chunk_behind_two_to_the_18_lines():
    from loongcollector_amd import delimiter
    dl = delimiter.GpuDelimiter(b",", b'"', "extend", 3)
    n = (1 << 18) + 1
    lines = [b"%d,b" % (i % 1000) if i % 7 else b'"q,%d",x,y' % (i % 10) for i in range(n)]
    hst, hnc, hsp = _host_equals_device(dl, lines, 4)
    assert (int(hnc[n - 1]), int(hnc[n - 2])) == (2, 3) and list(hsp[n - 1, 0]) == [0, len(lines[n - 1]) - 2]


def test_split_host_forty_lines_of_one_mib_cross_the_payload_limit():
    from loongcollector_amd import delimiter
    dl = delimiter.GpuDelimiter(b",", b'"', "extend", 3)
    lines = []
    for i in range(40):
        body = b"abcdefg," * (1 << 17) if i % 2 else b"k," + b"v" * ((1 << 20) - 4) + b",z"
        assert len(body) == 1 << 20
        lines += [body, b"s%d,t" % i, b""]
    hst, hnc, hsp = _host_equals_device(dl, lines, 4)
    assert [int(c) for c in hnc[:6]] == [3, 2, 0, (1 << 17) + 1, 2, 0]


def test_split_host_64_mib_of_spans_per_chunk_at_w_8192():
    from loongcollector_amd import delimiter
    dl = delimiter.GpuDelimiter(b",", b'"', "extend", 3)
    lines = [b",".join(b"c%d" % (i + c) for c in range(1 + i % 5)) for i in range(1100)]      # (1023 lines fill a chunk)
    hst, hnc, hsp = _host_equals_device(dl, lines, 8192)
    assert [int(c) for c in hnc[1020:1030]] == [1 + i % 5 for i in range(1020, 1030)]


def test_split_host_after_thread_release_gives_the_same_answer():
    from loongcollector_amd import binding, delimiter
    dl = delimiter.GpuDelimiter(b",", b'"', "extend", 3)
    data, off = _pack([b"a,b", b'"x,y",z', b"", b"k"])

    def body():
        first = dl.split_host(data, off, 4)
        binding.load().lc_thread_release()
        return first, dl.split_host(data, off, 4), binding.load().lc_last_error()

    first, second, error = fresh_thread.run(body)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]) and list(first[1]) == [2, 2, 0, 1]
    # the spans that count: columns from ncols[i] on are written by nobody (include/lc_delimiter.h), and the staging the second call
    # allocates need not hold what the first one's held
    live = np.arange(4)[None, :] < first[1][:, None]
    assert np.array_equal(first[2][live], second[2][live]) and first[2][live].tolist() == [[0, 1], [2, 3], [1, 4], [6, 7], [0, 1]]
    assert not error


def test_four_threads_share_one_processor_and_every_group_takes_the_mop_up():
    """three groups of 64 events per thread at a first trip of ONE column: 62 one-column lines, one line of six columns (the mop-up's)
    and one event without the key"""
    from loongcollector_amd import delimiter
    from helpers.shared_processor import four_threads_equal_one_thread

    def log(contents):
        return {"contents": contents, "timestamp": 1, "type": 1}

    def group(t, g):
        tag = "t%dg%d" % (t, g)
        events = [log({"content": "%s-%d" % (tag, i)}) for i in range(62)]
        events.insert(g * 20 + t, log({"content": '%s,"q,""1""",c,d,e,f' % tag}))
        return {"events": events + [log({"other": tag})]}

    groups = [[group(t, g) for g in range(3)] for t in range(4)]
    config = {"SourceKey": "content", "Separator": ",", "Keys": ["a", "b"], "AllowingShortenedFields": True}
    want, c = four_threads_equal_one_thread(lambda: delimiter.DelimiterProcessor(config, first_trip_columns=1), groups)
    assert want[2][1][22]["contents"] == {"a": "t2g1", "b": 'q,"1"', "__column2__": "c", "__column3__": "d", "__column4__": "e", "__column5__": "f"}
    assert want[2][1][0]["contents"] == {"a": "t2g1-0"}
    assert [c[k] for k in ("discarded_events_total", "out_failed_events_total", "out_key_not_found_events_total", "out_successful_events_total",
                           "in_events_total", "out_events_total")] == [0, 0, 12, 12 * 63, 12 * 64, 12 * 64]
