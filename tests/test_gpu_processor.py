"""processor_parse_regex_gpu on the device, through the C ABI: every case of the reference's unit test, a randomized
policy matrix against the processor oracle, and the dlsym slot (processor_interface) end to end."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

from loongcollector_amd import binding as B
from loongcollector_amd.processor import EventGroup, Processor, _lib
from oracle.processor_oracle import LogEventModel, ProcessorOracle

pytestmark = pytest.mark.gpu


def vectors(golden_dir):
    with open(os.path.join(golden_dir, "reference_unittest_vectors.json")) as f:
        return json.load(f)["cases"]


def test_every_reference_unit_test_case(golden_dir):
    assert B.device_count() >= 1
    for case in vectors(golden_dir):
        p = Processor(case["config"])
        if "expect_keys" in case:
            assert p.keys == case["expect_keys"], case["name"]
        if not case["events"]:
            continue
        g = EventGroup({"events": case["events"]})
        p.process(g)
        if "expect_contents" in case:
            assert [dict(c) for c in g.contents()] == case["expect_contents"], case["name"]
        c = p.counters()
        for name, want in case.get("expect_counters", {}).items():
            assert c[name] == want, (case["name"], name, c)
        if case.get("expect_out_size_bytes_nonzero"):
            assert c["out_size_bytes"] != 0, case["name"]
        # and the oracle agrees on the full ordered content lists
        po = ProcessorOracle(case["config"])
        out = po.process_group([LogEventModel([(k, v.encode()) for k, v in sorted(e["contents"].items())])
                                for e in case["events"]])
        assert g.contents() == [[(k, v.decode()) for k, v in ev.live()] for ev in out], case["name"]


@pytest.mark.parametrize("engine", ["tdfa", "nfa"])
def test_policy_matrix_against_the_oracle(engine):
    rng = np.random.default_rng(11)
    lines = ["v1\tv2", "value3\tvalue4 tail", "nomatch", "", "a\tb\nc", "x\t", "\ty", "k\tv"]
    for keep_fail, keep_ok, coping, renamed, keys in itertools.product(
            [False, True], [False, True], [False, True], ["", "rawLog", "content", "key2"],
            [["key1", "key2"], ["content", "key2"], ["key1", "key2", "key3"], ["rawLog", "x"]]):
        cfg = {"SourceKey": "content", "Regex": r"(\w+)\t(\w*).*", "Keys": keys, "KeepingSourceWhenParseFail": keep_fail,
               "KeepingSourceWhenParseSucceed": keep_ok, "CopingRawLog": coping, "RenamedSourceKey": renamed,
               "_Engine": engine}
        events, models = [], []
        for _ in range(12):
            kind = rng.integers(0, 10)
            if kind == 0:
                events.append({"content": "raw", "timestamp": 1, "type": 4})
                models.append(None)
                continue
            contents = []
            if rng.integers(0, 2):
                contents.append(["__file_offset__", "123"])
            if kind != 1:
                contents.append(["content", lines[int(rng.integers(0, len(lines)))]])
            if rng.integers(0, 3) == 0:
                contents.append(["key2", "preexisting"])
            events.append({"contents": contents, "timestamp": 1, "type": 1})
            models.append(LogEventModel([(k, v.encode()) for k, v in contents]))
        fixture = {"events": events, "metadata": {"log.file.offset": "__file_offset__"}}
        p, g = Processor(cfg), EventGroup(fixture)
        p.process(g)
        ocfg = {k: v for k, v in cfg.items() if k != "_Engine"}
        po = ProcessorOracle(ocfg)
        out = po.process_group(models, file_offset_key="__file_offset__")
        want = [None if ev is None else [(k, v.decode()) for k, v in ev.live()] for ev in out]
        assert g.contents() == want, cfg
        c = p.counters()
        assert (c["discarded_events_total"], c["out_failed_events_total"], c["out_key_not_found_events_total"],
                c["out_successful_events_total"], c["in_events_total"], c["out_events_total"]) == (
            po.counters["discarded"], po.counters["out_failed"], po.counters["out_key_not_found"],
            po.counters["out_successful"], po.counters["in_events"], po.counters["out_events"]), cfg


def test_unmatched_optional_group_yields_empty_value_like_boost():
    # what[i+1] of a group that did not participate is {last,last,matched=false}: an EMPTY value (cpp:249-251)
    p = Processor({"SourceKey": "content", "Regex": r"(\d+)(?: (\w+))?", "Keys": ["num", "word"]})
    g = EventGroup({"events": [{"contents": {"content": "12"}, "timestamp": 1, "type": 1},
                               {"contents": {"content": "12 ab"}, "timestamp": 1, "type": 1}]})
    p.process(g)
    assert g.contents() == [[("num", "12"), ("word", "")], [("num", "12"), ("word", "ab")]]


def test_large_group_of_apache_lines_zero_copy_stitch():
    from loongcollector_amd import corpus
    from oracle.oracle import OracleRegex
    n = 3000
    data, off, length = corpus.apache_batch(n, "A", poison_every=50)
    raw = data.tobytes()
    lines = [raw[off[i]:off[i] + length[i]].decode("latin-1") for i in range(n)]
    p = Processor({"SourceKey": "content", "Regex": corpus.REGEX_A, "Keys": corpus.KEYS_A,
                   "KeepingSourceWhenParseFail": True, "RenamedSourceKey": "__raw__"})
    g = EventGroup({"events": [{"contents": {"content": s}, "timestamp": 1, "type": 1} for s in lines]})
    p.process(g)
    caps, status = OracleRegex(corpus.REGEX_A).fullmatch_batch(data, off[:-1], length)
    got = g.contents()
    for i in range(n):
        if status[i]:
            want = [(k, lines[i][caps[i][2 * j]:caps[i][2 * j + 1]]) for j, k in enumerate(corpus.KEYS_A)]
        else:
            want = [("__raw__", lines[i])]
        assert got[i] == want
    c = p.counters()
    assert c["out_failed_events_total"] == n // 50 and c["out_successful_events_total"] == n


def test_dlsym_slot_end_to_end():
    """PluginRegistry::LoadProcessorPlugin's protocol: dlsym("processor_interface"), version check, init/process/finalize
    (PluginRegistry.cpp:270-290, DynamicCProcessorProxy.cpp:25-40)."""
    class Iface(ctypes.Structure):
        _fields_ = [("version", ctypes.c_int), ("name", ctypes.c_char_p), ("language", ctypes.c_char_p),
                    ("init", ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)),
                    ("finalize", ctypes.CFUNCTYPE(None, ctypes.c_void_p)),
                    ("process", ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p))]

    class Instance(ctypes.Structure):
        _fields_ = [("plugin", ctypes.c_void_p), ("plugin_state", ctypes.c_void_p)]

    lib = B.load()
    iface = Iface.in_dll(lib, "processor_interface")
    assert iface.version == 100
    ins = Instance()
    cfg = json.dumps({"SourceKey": "content", "Regex": r"(\w+)\t(\w+).*", "Keys": ["key1", "key2"]}).encode()
    assert iface.init(ctypes.addressof(ins), ctypes.c_char_p(cfg), None) == 0
    g = EventGroup({"events": [{"contents": {"content": "value1\tvalue2"}, "timestamp": 1, "type": 1}]})
    L = _lib()
    iface.process(ins.plugin_state, L.lc_group_native(g._h))
    assert g.contents() == [[("key1", "value1"), ("key2", "value2")]]
    iface.finalize(ins.plugin_state)
    bad = Instance()
    assert iface.init(ctypes.addressof(bad), ctypes.c_char_p(b'{"SourceKey":"c"}'), None) != 0


def test_concurrent_process_calls_on_one_instance():
    """Up to process_thread_count runner threads may call Process on the same instance
    (core/collection_pipeline/queue/ProcessQueueManager.cpp:167-205): device tables are shared, staging is per thread."""
    import threading
    from loongcollector_amd import corpus
    n_threads, groups_per_thread, lines_per_group = 4, 6, 700
    data, off, length = corpus.apache_batch(n_threads * groups_per_thread * lines_per_group, "B", poison_every=29)
    raw = data.tobytes()
    lines = [raw[off[i]:off[i] + length[i]].decode("latin-1") for i in range(len(length))]
    p = Processor({"SourceKey": "content", "Regex": corpus.REGEX_B, "Keys": corpus.KEYS_B})
    groups = [[EventGroup({"events": [{"contents": {"content": s}, "timestamp": 1, "type": 1}
                                      for s in lines[(t * groups_per_thread + g) * lines_per_group:
                                                     (t * groups_per_thread + g + 1) * lines_per_group]]})
               for g in range(groups_per_thread)] for t in range(n_threads)]
    errors = []

    def run(t):
        try:
            for g in groups[t]:
                p.process(g)
        except Exception as e:  # noqa
            errors.append(e)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors
    po = ProcessorOracle({"SourceKey": "content", "Regex": corpus.REGEX_B, "Keys": corpus.KEYS_B})
    idx = 0
    for t in range(n_threads):
        for g in groups[t]:
            part = lines[idx:idx + lines_per_group]
            idx += lines_per_group
            out = po.process_group([LogEventModel([("content", s.encode("latin-1"))]) for s in part])
            assert g.contents() == [[(k, v.decode("latin-1")) for k, v in ev.live()] for ev in out]
    c = p.counters()
    assert c["in_events_total"] == len(lines) and c["out_failed_events_total"] == po.counters["out_failed"]


def test_columnar_hand_off_equals_the_stitched_events():
    """lc_processor_parse_columnar (f4): the (begin, end) table + base pointers a serializer could consume directly.  For the same
    group, the fields read through it equal the contents lc_processor_process stitches, and content_bytes equals what
    SLSEventGroupSerializer::CalculateLogEventSize adds up for those contents (LogGroupSerializer.cpp:227-252)."""
    import numpy as np
    from loongcollector_amd import corpus
    from loongcollector_amd.processor import EventGroup, Processor

    def varint(v):
        n = 1
        while v >= 128:
            v >>= 7
            n += 1
        return n

    def content_size(k, v):
        inner = (1 + varint(len(k)) + len(k)) + (1 + varint(len(v)) + len(v))
        return inner + 1 + varint(inner)

    data, off, length = corpus.apache_batch(300, "A", poison_every=7)
    cfg = {"SourceKey": "content", "Regex": corpus.REGEX_A, "Keys": corpus.KEYS_A, "KeepingSourceWhenParseFail": True}
    p = Processor(cfg)
    g1 = EventGroup.from_lines(data, off[:-1], length)
    cols = p.parse_columnar(g1)
    assert len(g1) == 300 and g1.contents()[0][0][0] == "content"            # the group itself is untouched
    g2 = EventGroup.from_lines(data, off[:-1], length)
    p.process(g2)
    stitched = g2.contents()
    assert len(cols) == len(stitched) == 300
    n_parsed = 0
    for i, (col, ev) in enumerate(zip(cols, stitched)):
        if col is False:                                                   # poisoned line: parse failure, source kept by the policy
            assert i % 7 == 0 and [k for k, _ in ev] == ["content"]
            continue
        fields, nbytes = col
        assert [(k, v.decode("latin-1")) for k, v in fields] == [tuple(kv) for kv in ev], i
        assert nbytes == sum(content_size(k.encode(), v) for k, v in fields)
        n_parsed += 1
    assert n_parsed == 300 - len(range(0, 300, 7))
    # events the processor does not parse are reported as skipped
    g3 = EventGroup({"events": [{"contents": {"msg": "x"}, "timestamp": 1, "type": 1}, {"content": "raw", "timestamp": 1, "type": 4}]})
    assert p.parse_columnar(g3) == [None, None]


def test_regex_match_alarms_carry_the_reference_texts():
    """RegexLogLineParser raises REGEX_MATCH_ALARM for every event that does not match ("errorlog:<line>",
    ProcessorParseRegexNative.cpp:208-226) and for every event whose regex has fewer groups than Keys ("parse key count not
    match<what.size()>errorlog:<line>", :227-244): the same events, the same texts, in event order, through the alarm sink."""
    lines = ["value1\tvalue2", "nomatch", "a\tb tail", "", "x"]
    events = [{"timestamp": 1, "contents": {"content": l}} for l in lines]
    p = Processor({"SourceKey": "content", "Regex": r"(\w+)\t(\w+).*", "Keys": ["key1", "key2"], "KeepingSourceWhenParseFail": True})
    alarms = p.collect_alarms()
    p.process(EventGroup({"events": events}))
    assert alarms == [(0, b"errorlog:" + l.encode()) for l in lines if "\t" not in l]
    assert p.counters()["out_failed_events_total"] == 3
    # three keys, two groups: what.size() == 3 <= keys.size() -- every MATCHING event alarms, out_failed stays 0 (:652)
    p3 = Processor({"SourceKey": "content", "Regex": r"(\w+)\t(\w+).*", "Keys": ["key1", "key2", "key3"]})
    alarms3 = p3.collect_alarms()
    p3.process(EventGroup({"events": [{"timestamp": 1, "contents": {"content": l}} for l in lines[:1] + lines[2:3]]}))
    assert alarms3 == [(2, b"parse key count not match3errorlog:" + l.encode()) for l in (lines[0], lines[2])]
    assert p3.counters()["out_failed_events_total"] == 0
