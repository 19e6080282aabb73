"""The SLS encoder on the CPU: the per-event routines of csrc/sls_vm.hpp compiled for the host (a stand-alone program,
tests/native/sls_host_check.cpp, plain and under AddressSanitizer + UBSan) and the product's processor level
(csrc/processor_sls_gpu.cpp) over the host double of the device trip (tests/native/sls_double.cpp) -- against the reference's bytes of
tests/golden/sls_wire_vectors.json, against the reference itself where its tree is present, and against tests/helpers/sls_wire.py, the
model.  The routine is never its own reference.  Fixtures: tests/golden/README_sls.md."""
import ctypes
import json
import os
import random
import threading

import pytest

from helpers import sls_cases as sc
from helpers import sls_wire
from loongcollector_amd import sls

needs_reference = pytest.mark.skipif(not os.path.isdir(sc.REF), reason="needs the reference tree (/root/reference)")


# ---------------------------------------------------------------------------------------------- the routine, stand-alone
def _golden_batches():
    """the golden vectors whose events hold the source content alone, as engine batches (plan_of + the CPU oracle's match)"""
    out = []
    for v in sc.load_golden():
        if any(len(e["contents"]) != 1 for e in v["group"]["events"]):
            continue
        keys, matched, unmatched = sc.plan_of(v["config"])
        rows, _ = sc.engine_rows(v["config"], v["group"])
        out.append(((keys, matched, unmatched, rows, v["enable_ns"]), bytes.fromhex(v["bytes"])))
    return out


def _edge_batches():
    """hand-made batches against the model: value lengths around the varint borders, rows of (-1, -1), nested and overlapping groups, a
    group that ends at the line's last byte, every status byte, an empty unmatched list, long keys"""
    rng = random.Random(3)
    out = []
    keys = [b"k", b"key", b"four", b"fiver", b"K" * 130, b""]
    for vlen in [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 126, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 65537]:
        line = bytes(rng.randrange(256) for _ in range(vlen + 7))
        rows = []
        for head in range(4):
            caps = [head, head + vlen, -1, -1, 0, len(line), head, len(line), 1, 3]
            rows.append((line, 1, caps, rng.choice(sc.TIMES), rng.choice([-1, 0, 999999999])))
            rows.append((line[:head + vlen], head % 6, [head, head + vlen] + [-1] * 8, 5, -1))
        matched = [(0, 1), (1, 2), (2, 3), (4, 4), (5, 5), (3, 0)]
        out.append((keys, matched[:1], [], rows, 1))
        out.append((keys, matched[:3], [(4, 0)], rows, 0))
        out.append((keys, matched, [(0, 0), (5, 0)], rows, 1))
    return [(b, sc.model_batch(*b)[1]) for b in out]


@pytest.fixture(scope="module")
def batches():
    return _golden_batches() + _edge_batches()


def test_host_routine_equals_the_reference_s_bytes_and_the_model(batches, tmp_path):
    """every batch at all 16 residues of its first record's offset (the program compares them among themselves)"""
    assert len(batches) == 52 + 75
    got, _ = sc.run_host_check(sc.build_host_check(tmp_path), [b for b, _ in batches])
    bad = [(i, b[:3]) for i, ((b, want), (sizes, data)) in enumerate(zip(batches, got)) if data != want or sum(sizes) != len(want)]
    assert not bad, bad[:5]
    for (b, _), (sizes, _) in zip(batches, got):
        assert sizes == sc.model_batch(*b)[0]


def test_sanitized_host_check_program(batches, tmp_path):
    """the same stand-alone program under AddressSanitizer + UBSan, as a child process, once: every line, row and table from an
    exactly-sized heap copy, an output that ends with the last record"""
    got, err = sc.run_host_check(sc.build_host_check(tmp_path, sanitize=True), [b for b, _ in batches])
    assert [data for _, data in got] == [want for _, want in batches]
    assert err.strip() == "%d batches" % len(batches)


# ---------------------------------------------------------------------------------------------- the plan and the tags (host code of the product)
def test_plan_bounds_and_arguments():
    L = sc.double()
    sls.Plan([b"k"], [(0, 1)] * 256, [(0, 0)] * 256, lib=L)
    with pytest.raises(sls.SlsPlanError, match="rc=2 .*256 items"):
        sls.Plan([b"k"], [(0, 1)] * 257, lib=L)
    with pytest.raises(sls.SlsPlanError, match="rc=2 .*256 items"):
        sls.Plan([b"k"], [], [(0, 0)] * 257, lib=L)
    sls.Plan([b"k" * 65536], [(0, 1)], lib=L)
    with pytest.raises(sls.SlsPlanError, match="rc=2 .*65536 bytes of keys"):
        sls.Plan([b"k" * 65536, b"x"], [(0, 1)], lib=L)
    with pytest.raises(sls.SlsPlanError, match="rc=5 .*key 1 of 1"):
        sls.Plan([b"k"], [(1, 1)], lib=L)


def test_append_tags_equals_the_model_and_reports_the_room_it_needs():
    L = sc.double()
    rng = random.Random(5)
    for _ in range(50):
        pairs = []
        for _ in range(rng.randint(0, 6)):
            key = rng.choice([b"__topic__", b"__source__", b"__machine_uuid__", b"host", b"", b"__tag__:__path__", b"k" * 200, b"__topic_"])
            pairs.append((key, bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 5, 127, 128, 300, 16384])))))
        want = sls_wire.tags(pairs)
        assert sls.append_tags(pairs, lib=L) == want
        if want:
            with pytest.raises(OverflowError, match="%d bytes needed" % len(want)):
                sls.append_tags(pairs, cap=len(want) - 1, lib=L)


# ---------------------------------------------------------------------------------------------- the processor over the double
def _serialize(L, proc, fixture, enable_ns):
    g = sc.group_handle(L, fixture)
    before = sc.group_json(L, g)
    data, fused = proc.serialize(g, enable_ns)
    assert sc.group_json(L, g) == before     # the group is left untouched
    L.lc_group_free(g)
    return data, fused


def test_both_paths_give_the_reference_s_bytes_on_the_golden_file_and_the_twin_s_counters():
    L = sc.double()
    procs, twins, device_groups, host_groups = {}, {}, 0, 0
    for v in sc.load_golden():
        name = json.dumps(v["config"], sort_keys=True)
        if name not in procs:
            procs[name], twins[name] = sls.Processor(v["config"], lib=L), sc.Twin(L, v["config"])
        data, fused = _serialize(L, procs[name], v["group"], v["enable_ns"])
        assert data == bytes.fromhex(v["bytes"]), (v["config"], v["group"])
        assert fused == (1 if all(len(e["contents"]) == 1 for e in v["group"]["events"]) else 0)
        device_groups += fused
        host_groups += 1 - fused
        g = sc.group_handle(L, v["group"])
        twins[name].process(g)
        L.lc_group_free(g)
    assert (device_groups, host_groups) == (52, 1)
    for name, p in procs.items():
        c = p.counters()
        assert {k: c[k] for k in sls.PARSE_COUNTERS} == twins[name].counters(), name
        assert c["failed_trips"] == 0 and c["groups_device"] + c["groups_host"] >= 2
    assert sum(p.counters()["out_failed"] for p in procs.values()) > 50 and sum(p.counters()["discarded"] for p in procs.values()) > 10


def test_the_host_path_alone_gives_the_same_bytes():
    """events with a second content, metric-free: every golden vector once more with a `host` content beside the source, which the host
    path serves; the model says what the extra content adds (it stays in front: the source's slot is a hole behind it or before it)"""
    L = sc.double()
    for v in sc.load_golden()[::5]:
        if any(len(e["contents"]) != 1 for e in v["group"]["events"]):
            continue
        proc, twin = sls.Processor(v["config"], lib=L), sc.Twin(L, v["config"])
        group = {"events": [dict(e, contents={"content": e["contents"]["content"], "zz": "extra"}) for e in v["group"]["events"]]}
        data, fused = _serialize(L, proc, group, v["enable_ns"])
        assert fused == 0
        g = sc.group_handle(L, group)
        twin.process(g)
        left = json.loads(sc.group_json(L, g), object_pairs_hook=list)
        L.lc_group_free(g)
        events = sc.model_events([dict(ev) for ev in dict(left or []).get("events", [])])
        assert data == sls_wire.records(events, v["enable_ns"])
        c = proc.counters()
        assert {k: c[k] for k in sls.PARSE_COUNTERS} == twin.counters() and c["groups_host"] == 1 and c["groups_device"] == 0


@needs_reference
def test_fresh_random_groups_equal_the_reference():
    from test_reference_neighbours import RefPlugin
    L = sc.double()
    rng = random.Random(21)
    fused_groups = 0
    for config in sc.configs()[::3]:
        proc, ref = sls.Processor(config, lib=L), RefPlugin("processor_parse_regex_native", config)
        for k in range(6):
            group = sc.group(rng.randrange(1 << 30), n=rng.randint(0, 40), two_contents=k == 5)
            enable_ns = k & 1
            data, fused = _serialize(L, proc, group, enable_ns)
            assert data == sc.reference_bytes(ref, group, enable_ns), (config, group)
            fused_groups += fused
    assert fused_groups > 30


def test_a_whole_line_regex_too_many_keys_and_a_key_named_twice_take_the_host_path():
    L = sc.double()
    group = sc.group(99, n=12)
    plain = sc.configs()[0]
    want, fused = _serialize(L, sls.Processor(plain, lib=L), group, 1)
    assert fused == 1 and want
    for config in (dict(plain, Regex="(.*)", Keys=["content2"]), dict(plain, Keys=["a", "b", "c", "d", "e"]), dict(plain, Keys=["a", "b", "a"])):
        proc, twin = sls.Processor(config, lib=L), sc.Twin(L, config)
        data, fused = _serialize(L, proc, group, 1)
        g = sc.group_handle(L, group)
        twin.process(g)
        left = json.loads(sc.group_json(L, g), object_pairs_hook=list)
        L.lc_group_free(g)
        assert fused == 0 and data == sls_wire.records(sc.model_events([dict(ev) for ev in dict(left or []).get("events", [])]), 1)
        c = proc.counters()
        assert {k: c[k] for k in sls.PARSE_COUNTERS} == twin.counters()


def test_a_failing_trip_leaves_group_and_counters_as_the_other_processors_do():
    L = sc.double()
    config = sc.configs()[5]
    proc = sls.Processor(config, lib=L)
    group = sc.group(4, n=9)
    g = sc.group_handle(L, group)
    before = sc.group_json(L, g)
    L.sd_fail_next_trips(1)
    rc, data, _ = proc.serialize_rc(g, 1)
    assert rc == 4 and data is None and sc.group_json(L, g) == before
    c = proc.counters()
    assert c["failed_trips"] == 1 and c["device_failed"] == 9 and c["groups_device"] == c["groups_host"] == 0
    assert (c["discarded"], c["out_failed"], c["out_successful"], c["out_key_not_found"]) == (0, 0, 0, 0)
    data, fused = proc.serialize(g, 1)          # the next call works, on the same group
    L.lc_group_free(g)
    assert fused == 1 and proc.counters()["groups_device"] == 1 and proc.counters()["bytes"] == len(data)


def test_eight_threads_share_one_processor_each_holding_its_view_until_its_next_call():
    L = sc.double()
    config = sc.configs()[7]
    proc = sls.Processor(config, lib=L)
    keys, matched, unmatched = sc.plan_of(config)
    errors = []

    def runner(t):
        try:
            held = None
            for k in range(6):
                group = sc.group(100 * t + k, n=1 + 37 * t + k)
                rows, _ = sc.engine_rows(config, group)
                want = sc.model_batch(keys, matched, unmatched, rows, 1)[1]
                g = sc.group_handle(L, group)
                if held is not None:          # the view of this thread's call before, while the other threads made theirs
                    assert ctypes.string_at(held[0], held[1]) == held[2]
                out, n, fused = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
                assert L.lc_sls_processor_serialize(proc._h, g, 1, ctypes.byref(out), ctypes.byref(n), ctypes.byref(fused)) == 0
                L.lc_group_free(g)
                assert fused.value == 1 and ctypes.string_at(out, n.value) == want
                held = (out, n.value, want)
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=runner, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
    assert proc.counters()["groups_device"] == 48
