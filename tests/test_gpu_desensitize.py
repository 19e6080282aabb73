"""processor_desensitize_gpu on the device: the match kernels in rounds, desens_collect_kernel, desens_size_kernel, the scan and
desens_write_kernel through lc_desens_apply_device, lc_desens_apply_host and lc_desensitize_process, bit for bit against the model of
tests/helpers/desensitize_model.py -- every rule of the list, the edge corpus (cuts that begin and end on the chunk edges, every residue
of a value's first byte, every digest size, every match count and batch size), the two disciplines and the empty-match rules, sentinel
bytes in front of and behind the output bytes, out_off and the flags, one seeded batch of 64 Ki values, and the processor over the
unit-test fixtures, mixed groups, two threads, a parse -> desensitize chain, the plugin slot and the pass-through handle."""
import ctypes
import hashlib
import json
import threading

import numpy as np
import pytest

from helpers import desensitize_model as model
from helpers import desensitize_product as dp

pytestmark = pytest.mark.gpu
SENT = 0xA5
GUARD = 4
METHODS = ("const", "md5")


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def device_apply(torch, eng, values, want, pad_front=0, cap_short=0):
    """values back to back behind pad_front bytes, through lc_desens_apply_device into an output of EXACTLY the needed size (the model
    gives it); flags, out_off and the output bytes are sentinel-guarded on both sides.  -> (new value or None per value, flags, stats)"""
    from loongcollector_amd import desensitize
    n = len(values)
    blob = b"#" * pad_front + b"".join(values)
    size = max((len(blob) + 15) // 16 * 16, 16)
    data = np.frombuffer(blob + b"," * (size - len(blob)), np.uint8).copy()
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(v) for v in values])
    off += pad_front
    total = sum(len(w) for w in want if w is not None)
    dev = torch.device("cuda:0")
    flags = torch.full((n + 2 * GUARD,), SENT, dtype=torch.uint8, device=dev)
    out_off = torch.full((n + 1 + 2 * GUARD,), -7, dtype=torch.int64, device=dev)
    out = torch.full((total + 64,), SENT, dtype=torch.uint8, device=dev)
    d_out = out[32:32 + total - cap_short]
    try:
        needed, stats = eng.apply_device(torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev), None, n, flags[GUARD:], out_off[GUARD:],
                                         d_out if total - cap_short > 0 else None, stream=torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    f, o, b = flags.cpu().numpy(), out_off.cpu().numpy(), out.cpu().numpy()
    assert (f[:GUARD] == SENT).all() and (f[GUARD + n:] == SENT).all(), "flags: a guard byte was written"
    assert (o[:GUARD] == -7).all() and (o[GUARD + n + 1:] == -7).all(), "out_off: a guard row was written"
    assert (b[:32] == SENT).all() and (b[32 + total:] == SENT).all(), "the output was written outside its range"
    f, o = f[GUARD:GUARD + n], o[GUARD:GUARD + n + 1]
    assert needed == total == int(o[n]) and int(o[0]) == 0
    got = [bytes(b[32 + o[i]:32 + o[i + 1]]) if f[i] & dp.CHANGED else None for i in range(n)]
    for i in range(n):
        if not f[i] & dp.CHANGED:
            assert o[i + 1] == o[i], "an unchanged value took output bytes"
    return got, f, stats


def check(torch, name, method, replacing_all, values, pad_front=0, expected=None):
    from loongcollector_amd import binding, desensitize
    _, before, content, replacing = dp.RULE[name]
    rule = model.Rule(method, before, content, replacing, replacing_all)
    want = expected if expected is not None else [rule.apply(v) for v in values]
    eng = desensitize.GpuDesensitize(method, before, content, replacing, replacing_all)
    binding.launched_kernels()
    got, flags, stats = device_apply(torch, eng, values, want, pad_front)
    kernels = binding.launched_kernels()
    bad = [i for i in range(len(values)) if got[i] != want[i]]
    assert not bad, "%s %s all=%s: value %d %r: got %r, want %r" % (name, method, replacing_all, bad[0], values[bad[0]][:80], got[bad[0]] and got[bad[0]][:120],
                                                                    want[bad[0]] and want[bad[0]][:120])
    assert not (flags & dp.GAVE_UP).any()
    if values:
        assert "desens_collect_kernel" in kernels and "desens_size_kernel" in kernels
        assert ("desens_write_kernel" in kernels) == any(w is not None for w in want)
        if expected is None:
            assert stats["rounds"] == rule.rounds(values), (name, method, replacing_all)
        if not replacing_all:  # exactly ONE match launch
            assert stats["rounds"] == 1 and "desens_search_again" not in kernels
        assert ("desens_search_again" in kernels) == (stats["rounds"] > 1)
    return eng, stats


def corpus_of(name):
    values = list(dp.RULE_VALUES[name])
    if name == "edge":
        values += dp.edge_values()
    if name == "digest":
        values += dp.digest_values()
    if name == "pwd":
        values += dp.counted_values()
    return values


# ---------------------------------------------------------------------------------------------- rules
@pytest.mark.parametrize("name", [r[0] for r in dp.RULES])
def test_every_rule_both_methods(name):
    """the unit test's pwd= rule, the card rule with \\2 in the replacement, \\bkey\\b, the ^a / b pair, a rule that can match empty, a
    rule with $, a rule whose content holds a newline '.' must not cross; plus the edge, digest and counted corpora of their rules"""
    torch = _torch()
    values = corpus_of(name)
    for method in METHODS:
        for replacing_all in (False, True):
            for pad_front in (0, 5):
                check(torch, name, method, replacing_all, values, pad_front)


def test_handles_cover_the_tagged_dfa_and_the_thread_list_engine():
    _torch()
    from loongcollector_amd import binding, desensitize
    engines = {name: desensitize.GpuDesensitize("const", before, content, replacing, True).info()["engine"] for name, before, content, replacing in dp.RULES}
    assert engines["pwd"] == binding.LC_ENGINE_TDFA and engines["threads"] == binding.LC_ENGINE_NFA, engines


def test_the_two_disciplines_differ_on_the_anchor_pair():
    torch = _torch()
    digest = hashlib.md5(b"b").hexdigest().upper().encode()
    values = [b"abab", b"ab", b"xab"]
    check(torch, "anchor", "const", True, values, expected=[b"aXab", b"aX", None])
    check(torch, "anchor", "md5", True, values, expected=[b"a" + digest + b"a" + digest, b"a" + digest, None])


# ---------------------------------------------------------------------------------------------- edges
def test_cuts_begin_and_end_on_every_chunk_edge_and_residue():
    torch = _torch()
    values = dp.edge_values()
    at, residues = 0, set()
    for v in values:
        residues.add(at % 16)
        at += len(v)
    assert residues == set(range(16))
    for method in METHODS:
        check(torch, "edge", method, True, values)
        check(torch, "edge", method, True, values, pad_front=9)
    # a cut that ends on byte 0: the empty match at 0 (const: legal; md5: the me == s rule)
    check(torch, "empty", "const", False, [b".", b"x."], expected=[b"-.", b"-."])
    check(torch, "empty", "md5", False, [b".", b"x."], expected=[None, hashlib.md5(b"x").hexdigest().upper().encode() + b"."])


def test_digest_sizes_under_md5():
    torch = _torch()
    values = dp.digest_values()
    _, stats = check(torch, "digest", "md5", True, values)
    assert stats["rounds"] >= 1
    empty = hashlib.md5(b"").hexdigest().upper().encode()
    check(torch, "digest", "md5", True, [b"head k=;tail"], expected=[b"head k=" + empty + b";tail"])  # a legal empty content


def test_replacements_shorter_equal_and_longer_than_the_content():
    torch = _torch()
    from loongcollector_amd import desensitize
    values = [b"a pwd=12345678, b pwd=abcdefgh,", b"pwd=12345678", b"none"] * 23
    for replacing in (b"*", b"*" * 8, b"*" * 40):
        rule = model.Rule("const", "pwd=", "[^,]+", replacing, True)
        want = [rule.apply(v) for v in values]
        got, _, _ = device_apply(torch, desensitize.GpuDesensitize("const", "pwd=", "[^,]+", replacing, True), values, want, pad_front=3)
        assert got == want, replacing


def test_match_counts_mixed_inside_one_wavefront():
    torch = _torch()
    values = dp.counted_values()
    rule = model.Rule("const", *dp.RULE["pwd"][1:], True)
    assert sorted({len(rule.cuts(v)[0]) for v in values}) == list(dp.MATCH_COUNTS) and len(values) > 64
    for method in METHODS:
        _, stats = check(torch, "pwd", method, True, values)
        assert stats["rounds"] >= 65


@pytest.mark.parametrize("n", dp.BATCH_SIZES)
def test_batch_sizes(n):
    torch = _torch()
    values = [(b"x" * (i % 37) + b"pwd=%d," % i) * (i % 3) + b"tail" for i in range(n)]
    for method in METHODS:
        check(torch, "pwd", method, True, values)


# ---------------------------------------------------------------------------------------------- semantics
def test_values_that_end_inside_or_with_a_match():
    torch = _torch()
    # the buffer goes on behind the value with bytes the rule would take (device_apply pads with ','; here the next value starts with them)
    values = [b"a pwd=abc", b"defgh,", b"pwd=", b"x,pwd=zz", b"pw", b"d=1,"]
    for method in METHODS:
        check(torch, "pwd", method, True, values)
        check(torch, "dollar", method, True, [b"end=abc", b"end=abc end=def", b"x end=q1"])


def test_me_equals_s_leaves_the_whole_value_unchanged():
    torch = _torch()
    digest = hashlib.md5(b"xx").hexdigest().upper().encode()
    values = [b"abc", b"xxabc", b"xx", b"ax", b"xxxxa"]
    _, stats = check(torch, "empty", "md5", True, values, expected=[None, None, digest, None, None])
    assert stats["rounds"] == 2  # (the rule struck on the first search of "abc" and on the SECOND of "xxabc")


def test_const_steps_one_byte_behind_an_empty_match():
    torch = _torch()
    want = {b"xaxx": b"-a-", b"abc": b"-a-b-c-", b"xx": b"-", b"ax": b"-a-", b"xxxxa": b"-a-"}
    check(torch, "empty", "const", True, list(want), expected=list(want.values()))


def test_output_that_does_not_fit_is_refused_before_anything_is_written():
    torch = _torch()
    from loongcollector_amd import desensitize
    values = [b"pwd=abc,", b"none", b"pwd=d,pwd=e,"]
    rule = model.Rule("const", *dp.RULE["pwd"][1:], True)
    want = [rule.apply(v) for v in values]
    eng = desensitize.GpuDesensitize("const", *dp.RULE["pwd"][1:], True)
    with pytest.raises(desensitize.DesensitizeOverflow) as e:
        device_apply(torch, eng, values, want, cap_short=1)  # (the guards are checked on the way out: nothing was written)
    assert e.value.needed == sum(len(w) for w in want if w)
    got, _, _ = device_apply(torch, eng, values, want)
    assert got == want


def test_host_entry_equals_device_entry():
    _torch()
    from loongcollector_amd import desensitize
    values = corpus_of("pwd") + corpus_of("edge")
    for method in METHODS:
        rule = model.Rule(method, *dp.RULE["pwd"][1:], True)
        got, flags, stats = desensitize.GpuDesensitize(method, *dp.RULE["pwd"][1:], True).apply_host(values)
        assert got == [rule.apply(v) for v in values] and stats["rounds"] == rule.rounds(values)
    assert desensitize.GpuDesensitize("const", *dp.RULE["pwd"][1:], True).apply_host([])[0] == []


# ---------------------------------------------------------------------------------------------- the random batch
@pytest.mark.parametrize("method", METHODS)
def test_random_batch_of_64k_values(method):
    torch = _torch()
    values, want = dp.random_expected(method)
    check(torch, "pwd", method, True, values, expected=want)


# ---------------------------------------------------------------------------------------------- the processor
def _real():
    from loongcollector_amd import desensitize
    from loongcollector_amd.processor import EventGroup
    L = desensitize._lib()
    return L, EventGroup, desensitize


def _contents(group):
    return [ev.get("contents", ev.get("content")) for ev in group.to_dict()["events"]]


def test_fixture_groups_through_the_processor():
    _torch()
    L, EventGroup, desensitize = _real()
    fixtures = dp.load_fixtures()
    assert len(fixtures["cases"]) >= 28
    for case in fixtures["cases"]:
        g = EventGroup(case["at_desensitize"])
        for stage in case["stages"]:
            if stage["kind"] != "desensitize":
                continue
            p = desensitize.DesensitizeProcessor(stage["config"])
            p.process(g)
            c = p.counters()
            for k, v in stage["counters"].items():
                assert c[k] == v, (case["name"], k)
        got = [{"type": ev.get("type"), "contents": sorted(ev.get("contents", {}).items())} for ev in g.to_dict()["events"]]
        want = [{"type": ev["type"], "contents": [tuple(kv) for kv in ev["contents"]]} for ev in case["out"]]
        assert got == want, case["name"]


BASE = {"SourceKey": "cast1", "Method": "const", "ReplacingString": "********", "ContentPatternBeforeReplacedString": "pwd=",
        "ReplacedContentPattern": "[^,]+", "ReplacingAll": True}


def test_mixed_groups_counters_and_views():
    _torch()
    L, EventGroup, desensitize = _real()
    group = {"events": [{"type": 1, "timestamp": 1, "contents": {"cast1": "a pwd=x1, pwd=y2,", "other": "pwd=keep,"}},
                        {"type": 4, "timestamp": 1, "content": "raw pwd=z,"},
                        {"type": 1, "timestamp": 1, "contents": {"other": "pwd=no-key,"}},
                        {"type": 1, "timestamp": 1, "contents": {"cast1": ""}},
                        {"type": 1, "timestamp": 1, "contents": {"cast1": "no secret"}}]}
    for method in METHODS:
        config = dict(BASE, Method=method)
        g = EventGroup(group)
        before = [L.lc_group_content_address(g._h, i, b"cast1") for i in range(5)]
        p = desensitize.DesensitizeProcessor(config)
        p.process(g)
        want, counters = model.process_group(config, group)
        assert _contents(g) == [ev.get("contents", ev.get("content")) for ev in want["events"]]
        c = p.counters()
        assert {k: c[k] for k in counters} == counters and c["in_events_total"] == c["out_events_total"] == 5
        assert c["complexity_exceeded_events_total"] == 0 and c["device_failed_events_total"] == 0
        after = [L.lc_group_content_address(g._h, i, b"cast1") for i in range(5)]
        assert after[0] != before[0] and after[1:] == before[1:]  # unchanged values keep their views


def test_me_equals_s_value_keeps_its_view_in_the_original_buffer():
    _torch()
    L, EventGroup, desensitize = _real()
    _, before, content, _ = dp.RULE["empty"]
    config = {"SourceKey": "k", "Method": "md5", "ContentPatternBeforeReplacedString": before, "ReplacedContentPattern": content, "ReplacingAll": True}
    values = ["abc", "xxabc", "xx"]  # the rule on the first search, on a later one, and a value that does change
    g = EventGroup({"events": [{"type": 1, "timestamp": 1, "contents": {"k": v}} for v in values]})
    at = [L.lc_group_content_address(g._h, i, b"k") for i in range(3)]
    desensitize.DesensitizeProcessor(config).process(g)
    assert [c["k"] for c in _contents(g)] == ["abc", "xxabc", hashlib.md5(b"xx").hexdigest().upper()]
    now = [L.lc_group_content_address(g._h, i, b"k") for i in range(3)]
    assert now[0] == at[0] and now[1] == at[1] and now[2] != at[2]


def test_two_groups_on_two_threads_through_one_handle():
    _torch()
    L, EventGroup, desensitize = _real()
    p = desensitize.DesensitizeProcessor(BASE)
    groups = [{"events": [{"type": 1, "timestamp": 1, "contents": {"cast1": "t%d line %d pwd=s%d, pwd=%d," % (t, i, i, t)}} for i in range(300 + 50 * t)]}
              for t in range(2)]
    handles, errors = [EventGroup(g) for g in groups], []

    def run(g):
        try:
            p.process(g)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=run, args=(g,)) for g in handles]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for g, src in zip(handles, groups):
        want, _ = model.process_group(BASE, src)
        assert _contents(g) == [ev["contents"] for ev in want["events"]]
    assert p.counters()["out_successful_events_total"] == 650


def test_chain_regex_parse_then_desensitize_a_parsed_key():
    """the value is a view into the MIDDLE of the source buffer: the parser's capture"""
    _torch()
    L, EventGroup, desensitize = _real()
    from loongcollector_amd.processor import Processor
    lines = [b"10.0.0.%d GET /login?user=u%d&pwd=secret%d,next 200" % (i % 250, i, i * 7) for i in range(200)] + [b"1.1.1.1 GET /plain 200"]
    data = np.frombuffer(b"".join(lines), np.uint8)
    length = np.array([len(v) for v in lines], np.uint32)
    off = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.uint32)
    g = EventGroup.from_lines(data, off, length)
    parser = Processor({"SourceKey": "content", "Regex": r"(\S+) (\S+) (\S+) (\d+)", "Keys": ["ip", "verb", "url", "status"]})
    parser.process(g)  # (the parsed keys are views into the parser's own strings: it has to outlive the group)
    config = dict(BASE, SourceKey="url")
    desensitize.DesensitizeProcessor(config).process(g)
    rule = model.Rule.from_config(config)
    for ev, line in zip(_contents(g), lines):
        ip, verb, url, status = line.split(b" ")
        new = rule.apply(url)
        assert ev["url"].encode() == (new if new is not None else url) and ev["ip"].encode() == ip and ev["status"].encode() == status
    assert b"secret" not in json.dumps(_contents(g)).encode()
    parser.close()


def test_slot_builds_the_desensitize_processor():
    _torch()
    L, EventGroup, _ = _real()

    class Instance(ctypes.Structure):
        _fields_ = [("plugin", ctypes.c_void_p), ("plugin_state", ctypes.c_void_p)]

    class Interface(ctypes.Structure):
        _fields_ = [("version", ctypes.c_int), ("name", ctypes.c_char_p), ("language", ctypes.c_char_p),
                    ("init", ctypes.CFUNCTYPE(ctypes.c_int, ctypes.POINTER(Instance), ctypes.c_void_p, ctypes.c_void_p)),
                    ("finalize", ctypes.CFUNCTYPE(None, ctypes.c_void_p)), ("process", ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p))]
    iface = Interface.in_dll(L, "processor_interface")
    ins = Instance()
    cfg = json.dumps(dict(BASE, Type="processor_desensitize_gpu")).encode()
    assert iface.init(ctypes.byref(ins), ctypes.c_char_p(cfg), None) == 0
    g = EventGroup({"events": [{"contents": {"cast1": "x pwd=abc, y"}, "timestamp": 1, "type": 1}]})
    iface.process(ins.plugin_state, L.lc_group_native(g._h))
    assert _contents(g) == [{"cast1": "x pwd=********, y"}]
    iface.finalize(ins.plugin_state)
    bad = Instance()
    assert iface.init(ctypes.byref(bad), ctypes.c_char_p(json.dumps({"Type": "processor_desensitize_gpu", "SourceKey": "k"}).encode()), None) != 0
    assert not bad.plugin_state


def test_pass_through_handle():
    _torch()
    L, EventGroup, desensitize = _real()
    from loongcollector_amd import binding
    entry = dp.load_fixtures()["defined_only"][0]
    p = desensitize.DesensitizeProcessor(entry["config"])
    assert len(p.warnings()) == 1
    g = EventGroup(entry["in"])
    at = L.lc_group_content_address(g._h, 0, b"cast1")
    binding.launched_kernels()
    p.process(g)
    assert binding.launched_kernels() == ""
    assert _contents(g) == [entry["in"]["events"][0]["contents"]] and L.lc_group_content_address(g._h, 0, b"cast1") == at
    assert p.counters()["out_successful_events_total"] == 1
    eng = desensitize.GpuDesensitize("const", "pwd=", "[^,]+", r"\x", True)
    assert eng.pass_through and eng.apply_host([b"pwd=a,", b"b"])[0] == [None, None]


# ---------------------------------------------------------------------------------------------- the host entry's chunk limits
def _host_raw(eng, values):
    """lc_desens_apply_host itself -> (flags, out_off uint64[n + 1], the output bytes); both arrays hold a sentinel beforehand"""
    n = len(values)
    blob = np.frombuffer(b"".join(values) + b"\0", np.uint8).copy()
    lens = np.array([len(v) for v in values], np.uint32)
    at = np.zeros(n, np.uint64)
    at[1:] = np.cumsum(lens[:-1])
    ptrs = (blob.ctypes.data + at).astype(np.uint64)
    flags = np.full(n, SENT, np.uint8)
    out_off = np.full(n + 1, 7, np.uint64)
    out = ctypes.c_void_p()
    rc = eng._L.lc_desens_apply_host(eng._h, ptrs.ctypes.data, lens.ctypes.data, n, flags.ctypes.data, out_off.ctypes.data, ctypes.byref(out), None)
    assert rc == 0
    try:
        return flags, out_off, ctypes.string_at(out, int(out_off[n])) if out.value else b""
    finally:
        eng._L.lc_free(out)


def _host_equals_device(eng, values, want):
    """lc_desens_apply_host against lc_desens_apply_device over the same packed values (device_apply: into an output of exactly the
    size `want` gives): the flags, every value's output bytes, and an out_off that is monotone over the whole call"""
    torch = _torch()
    dev, dev_flags, _ = device_apply(torch, eng, values, want)
    flags, out_off, new = _host_raw(eng, values)
    assert np.array_equal(flags, dev_flags)
    assert np.array_equal(flags, np.array([dp.CHANGED if w is not None else 0 for w in want], np.uint8)), "the flags are not the model's"
    assert int(out_off[0]) == 0 and np.array_equal(np.diff(out_off.astype(np.int64)), np.array([len(w) if w is not None else 0 for w in want], np.int64))
    host = [new[int(out_off[i]):int(out_off[i + 1])] if flags[i] & dp.CHANGED else None for i in np.flatnonzero(flags)]
    assert host == [dev[i] for i in np.flatnonzero(flags)]
    return host, out_off


@pytest.mark.parametrize("method", METHODS)
def test_apply_host_second_chunk_behind_two_to_the_18_values(method):
    from loongcollector_amd import desensitize
    _, before, content, replacing = dp.RULE["pwd"]
    rule = model.Rule(method, before, content, replacing, True)
    eng = desensitize.GpuDesensitize(method, before, content, replacing, True)
    n = (1 << 18) + 1
    fill = [b"user=u%d ip=10.0.0.%d" % (k, k) for k in range(16)]
    values = [fill[i % 16] for i in range(n)]
    for i in (0, 3, 64, 4097, 200000):           # a handful in the first chunk ...
        values[i] = b"v%d pwd=one%d, then pwd=two," % (i, i)
    values[n - 1] = b"last pwd=secret9, and pwd=again"          # ... and the one-value second chunk
    cache = {v: rule.apply(v) for v in set(values)}
    want = [cache[v] for v in values]
    assert [i for i, w in enumerate(want) if w is not None] == [0, 3, 64, 4097, 200000, n - 1]
    host, out_off = _host_equals_device(eng, values, want)
    assert host[-1] == want[n - 1] and host[:5] == [want[i] for i in (0, 3, 64, 4097, 200000)]
    if method == "const":
        assert host[-1] == b"last pwd=********, and pwd=********"
    assert int(out_off[n - 1]) == sum(len(want[i]) for i in (0, 3, 64, 4097, 200000)) and int(out_off[n]) == int(out_off[n - 1]) + len(want[n - 1])


def test_apply_host_forty_values_of_one_mib_cross_the_payload_limit():
    from loongcollector_amd import desensitize
    _, before, content, replacing = dp.RULE["pwd"]
    eng = desensitize.GpuDesensitize("const", before, content, replacing, True)
    values, want = [], []
    for i in range(40):           # every other 1 MiB value with one match near its end
        tail = b" pwd=topsecret%02d, end" % i if i % 2 else b""
        body = b"x" * ((1 << 20) - len(tail)) + tail
        assert len(body) == 1 << 20
        values += [body, b"s%d pwd=k%d," % (i, i), b""]
        want += [body.replace(b"topsecret%02d" % i, b"********") if i % 2 else None, b"s%d pwd=********," % i, None]
    host, out_off = _host_equals_device(eng, values, want)
    assert len(host) == 60 and int(out_off[-1]) == sum(len(w) for w in want if w is not None)
