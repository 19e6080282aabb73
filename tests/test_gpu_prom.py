"""processor_prom_parse_metric_gpu on the device: prom_parse_kernel over every fixture line through lc_prom_parse_device and
lc_prom_parse_host against the per-line routine compiled for the host (which tests/test_prom_host.py holds to the reference), the edges
of the stage walk with every decision byte on chosen offsets for every residue of the line's first byte, sentinel-guarded outputs,
label counts around W, argument errors, 64 Ki generated lines, and the processor on 1000-event groups against the CPU double."""
import ctypes
import random

import numpy as np
import pytest

from helpers import prom_product as pp

pytestmark = pytest.mark.gpu
SENT = 0xA5
GUARD = 4  # guard rows before and behind every output array
OFFSETS = (15, 16, 17, 63, 64, 65, 127, 128, 129)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def fixtures():
    return pp.load_fixtures()


def pack(lines, pad_front=0):
    """lines back to back behind pad_front bytes -> (data uint8 padded to whole 16-byte units with bytes the routine would react to, off)"""
    blob = b"#" * pad_front + b"".join(lines)
    size = max((len(blob) + 15) // 16 * 16 + 16, 16)
    data = np.frombuffer(blob + b'"\\}' * ((size - len(blob)) // 3 + 1), np.uint8)[:size].copy()
    off = np.zeros(len(lines) + 1, np.int32)
    off[1:] = np.cumsum([len(v) for v in lines])
    return data, off + pad_front


def host_rows(data, off, honor, W, finish=False):
    """the per-line routine on the host over the same packed bytes (the same residues), every array pre-filled with the sentinel"""
    n = len(off) - 1
    res = pp.out_arrays(n, max(W, 1), fill=SENT)
    o = pp.LcPromOut(*(res[k].ctypes.data for k in pp.OUT_KEYS))
    finished = pp.double().pd_parse_resident(int(honor), data.ctypes.data, off.ctypes.data, n, ctypes.byref(o), W, int(finish))
    if W == 0:
        res["labels"] = res["labels"][:, :0]
    res["finished"] = int(finished)
    return res


def device_rows(torch, data, off, honor, W):
    """lc_prom_parse_device over the packed bytes; every output array is pre-filled with the sentinel and guarded on both sides"""
    from loongcollector_amd import prom
    n = len(off) - 1
    dev = torch.device("cuda:0")
    full, d_out, rows = {}, {}, {}
    for k, (shape, dtype) in prom.out_shapes(n, W).items():  # byte buffers: (GUARD rows, the n rows, GUARD rows), all sentinel
        rows[k] = int(np.prod(shape[1:])) * np.dtype(dtype).itemsize
        full[k] = torch.full(((n + 2 * GUARD) * rows[k] + 16,), SENT, dtype=torch.uint8, device=dev)
        d_out[k] = full[k][GUARD * rows[k]:(GUARD + n) * rows[k]] if rows[k] else None
    prom.parse_device(honor, torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev), n, d_out, W, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = {}
    for k, (shape, dtype) in prom.out_shapes(n, W).items():
        raw = full[k].cpu().numpy()
        assert (raw[:GUARD * rows[k]] == SENT).all() and (raw[(GUARD + n) * rows[k]:] == SENT).all(), "%s: a guard row was written" % k
        res[k] = raw[GUARD * rows[k]:(GUARD + n) * rows[k]].view(dtype).reshape(shape)
    return res


def same(got, want, lines, what):
    for k in pp.OUT_KEYS:
        if np.array_equal(got[k], want[k]):
            continue
        g, w = got[k].reshape(len(lines), -1), want[k].reshape(len(lines), -1)
        i = int(np.nonzero((g != w).any(axis=1))[0][0])
        raise AssertionError("%s: %s of line %d %r: %r, the host routine %r (status %d / %d)" % (
            what, k, i, lines[i][:120], g[i][:16], w[i][:16], got["status"][i], want["status"][i]))


def check(torch, lines, honor=True, W=16, pad_front=0, what="device"):
    data, off = pack(lines, pad_front)
    want = host_rows(data, off, honor, W)
    same(device_rows(torch, data, off, honor, W), want, lines, what)
    return want


def test_fixture_lines_device_and_host_entry(fixtures):
    from loongcollector_amd import prom
    torch = _torch()
    ref, unit = fixtures
    for honor in (True, False):
        lines = [ln for _, ln, h, _ in pp.all_cases(ref, unit) if h == honor] + [e["line"].encode("latin-1") for e in ref["defined_only"] if e["honor"] == honor]
        assert len(lines) > 80
        raw = check(torch, lines, honor, W=16, what="device, honor %s" % honor)
        assert honor is False or (np.count_nonzero(raw["flags"] & pp.VALUE_HOST) > 500 and np.count_nonzero(raw["flags"] & pp.TIME_HOST) > 10)
        # the host entry: the same trip plus the host finish, against the routine plus promFinishHost line by line
        got = prom.parse_host(lines, honor, W=16, fill=SENT)
        for i, ln in enumerate(lines):
            want = pp.host_parse(ln, honor, W=16)
            for k in pp.OUT_KEYS:
                assert np.array_equal(got[k][i], want[k]), ("host entry", k, ln)
        assert got["deferred"] == sum(pp.host_parse(ln, honor, W=1)["finished"] for ln in lines)


# ---------------------------------------------------------------------------------------------- the edge corpus
# kind -> (what follows the filler name, index of the decision byte in it, failing variants of what follows)
EDGE_KINDS = {
    "name_last": ('n{a="b"} 1', 0, ["n", "n ", "n{"]),
    "open_brace": ('{a="b"} 1', 0, ["{", "{ ", "{9"]),
    "label_last": ('{abc="b"} 1', 3, ["{abc", "{abc "]),
    "equal": ('{abc="b"} 1', 4, ["{abc:", "{abc"]),
    "open_quote": ('{abc="b"} 1', 5, ["{abc='b'} 1", "{abc="]),
    "backslash": ('{a="bc\\ndef"} 1', 6, ['{a="bc\\', '{a="bc\\"} 1']),
    "close_quote": ('{a="bcd"} 1', 7, ['{a="bcd', '{a="bcd";} 1']),
    "comma": ('{a="b",c="d"} 1', 6, ['{a="b";c="d"} 1', '{a="b",', '{a="b",,}']),
    "close_brace": ('{a="b",c="d"} 1', 12, ['{a="b",c="d"', '{a="b",c="d" ']),
    "value_first": ('{a="b"} 12.5e3 1715829785083', 8, ['{a="b"} z2.5', '{a="b"} ']),
    "value_last": ('{a="b"} 12.5e3', 13, ['{a="b"} 12.5e3z', '{a="b"} 12.5e', '{a="b"} 12.5e3,']),
    "value_last_then_more": ('{a="b"} 12.5e3 1715829785', 13, []),
    "time_first": (' 12 1715829785', 4, [" 12 z715829785", " 12 -", " 12 5"]),
    "time_last": (' 1 1715829785', 12, [" 1 1715829785z", " 1 171582978x", " 1 171582978"]),
    "time_last_then_more": (' 1 1715829785 # x', 12, []),
    "hash_behind_value": (' 1234567890123 #', 15, [" 1234567890123 }"]),
    "hash_right_behind_value": (' 12345678901234#x', 15, [" 12345678901234z#"]),
    "hash_behind_time": (' 1 1715829785#', 13, []),
}


def edge_lines():
    """-> [(kind, p, residue, line)]: the decision byte of `kind` at offset p of its line, and the failing variants with the same filler;
    and the shortest lines"""
    out = []
    for kind, (after, idx, failing) in EDGE_KINDS.items():
        for p in OFFSETS:
            for variant in [after] + failing:
                out.append((kind, p, "n" * (p - idx) + variant))
    for length in (0, 1, 63, 64, 65):
        out.append(("length_ok", length, ("m" * (length - 2) + " 1") if length >= 3 else ""))
        out.append(("length_fail", length, "m" * length))
        out.append(("length_blank", length, " " * length))
        if length >= 8:
            out.append(("length_label", length, 'm{a="%s"} 1' % ("v" * (length - 9))))
            out.append(("length_open", length, 'm{a="%s' % ("v" * (length - 5))))
            out.append(("length_backslash_last", length, 'm{a="%s\\' % ("v" * (length - 6))))
    return [(kind, p, r, text.encode()) for kind, p, text in out for r in range(16)]


def with_residues(cases):
    """filler lines between the cases give every case line its residue -> (lines, indices of the case lines)"""
    lines, index, at = [], [], 0
    for _, _, r, line in cases:
        gap = (r - at) % 16
        if gap:
            lines.append((b'\\"}{=,# ' * 2)[:gap])  # (a line of its own, parsed and ignored; it must not leak into its neighbour)
            at += gap
        index.append(len(lines))
        lines.append(line)
        at += len(line)
    return lines, index


def test_edge_corpus_is_what_it_says():
    """CPU-checkable part (needs no device but lives with the corpus): the decision bytes stand where the corpus says, every status
    the failing variants aim at occurs, every residue occurs"""
    cases = edge_lines()
    for kind, p, r, line in cases:
        if kind in EDGE_KINDS and line.decode().endswith(EDGE_KINDS[kind][0]):
            after, idx, _ = EDGE_KINDS[kind]
            assert line[p:p + 1] == after[idx:idx + 1].encode(), (kind, p)
    lines, index = with_residues(cases)
    data, off = pack(lines)
    assert {int(off[i]) % 16 for i in index} == set(range(16))
    rows = host_rows(data, off, True, 4)
    ok = {kind for (kind, p, r, line), i in zip(cases, index) if rows["status"][i] == pp.OK and line.decode().endswith(EDGE_KINDS.get(kind, ("\0",))[0])}
    assert ok == set(EDGE_KINDS), set(EDGE_KINDS) - ok
    statuses = {int(rows["status"][i]) for i in index}
    assert statuses >= {pp.STATUS[s] for s in ("NAME", "NAME_END", "EQUAL", "LABEL_NAME", "QUOTE", "LABEL_VALUE_END", "LABEL_VALUE_NEXT", "VALUE_END", "VALUE",
                                               "TIME_END", "TIMESTAMP_SMALL")}, statuses


@pytest.mark.parametrize("honor", [True, False])
def test_decision_bytes_on_stage_edges_for_every_residue(honor):
    torch = _torch()
    cases = edge_lines()
    lines, index = with_residues(cases)
    assert len(lines) > 8000
    check(torch, lines, honor, W=2, what="edges")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_leave_lanes_without_a_line(fixtures, n):
    torch = _torch()
    pool = [ln for _, ln, h, _ in pp.all_cases(*fixtures) if h][::7]
    lines = [pool[i % len(pool)] for i in range(n)]
    check(torch, lines, True, W=3, pad_front=5, what="n = %d" % n)


@pytest.mark.parametrize("W", [0, 1, 2, 16])
def test_label_counts_around_w(W):
    torch = _torch()
    lines = []
    for count in sorted({0, 1, max(W - 1, 0), W, W + 1, 2 * W + 3, 40}):
        labels = ",".join('l%d="v%s%d"' % (k, "\\\\" if k % 3 == 2 else "", k) for k in range(count))
        lines += [("m{%s} %d" % (labels, count)).encode(), ("broken{%s" % labels).encode()]
    want = check(torch, lines, True, W=W, what="W = %d" % W)
    assert [int(v) for v in want["nlabels"][0::2]] == sorted({0, 1, max(W - 1, 0), W, W + 1, 2 * W + 3, 40})  # the TRUE count, also above W


def test_argument_errors():
    from loongcollector_amd import binding, prom
    torch = _torch()
    dev = torch.device("cuda:0")
    data, off = pack([b'm{a="b"} 1'] * 4)
    d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)

    def outputs(n, W, shift=()):
        out = {}
        for k, (shape, dtype) in prom.out_shapes(n, W).items():
            count = int(np.prod(shape)) + 4
            flat = torch.zeros(count * np.dtype(dtype).itemsize + 16, dtype=torch.uint8, device=dev)
            start = 4 if k in shift else 0  # (the allocation itself is aligned: 4 bytes in is not 8- or 16-byte aligned)
            out[k] = flat[start:start + int(np.prod(shape)) * np.dtype(dtype).itemsize]
        return out
    prom.parse_device(True, d_data, d_off, 4, outputs(4, 2), 2)
    torch.cuda.synchronize()
    for key in ("labels", "value", "name", "secs"):
        with pytest.raises(RuntimeError) as e:
            prom.parse_device(True, d_data, d_off, 4, outputs(4, 2, shift=(key,)), 2)
        assert "rc=%d " % binding.LC_ERR_ARG in str(e.value), key
    # n = 0 touches nothing, NULL arrays included
    L = prom._lib()
    assert L.lc_prom_parse_device(1, None, None, 0, None, 16, None) == binding.LC_OK
    assert L.lc_prom_parse_host(1, None, None, 0, None, 16, None) == binding.LC_OK
    # a missing array is refused
    missing = outputs(4, 2)
    missing["nanos"] = None
    with pytest.raises(RuntimeError):
        prom.parse_device(True, d_data, d_off, 4, missing, 2)
    torch.cuda.synchronize()


def test_a_tensor_of_another_device_is_refused():
    from loongcollector_amd import binding, prom
    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: nothing lives on another one")
    data, off = pack([b"m 1"] * 4)
    other = torch.device("cuda:1")
    d_out = {k: torch.zeros((int(np.prod(s)) * np.dtype(t).itemsize,), dtype=torch.uint8, device=other) for k, (s, t) in prom.out_shapes(4, 2).items()}
    torch.cuda.set_device(0)
    with pytest.raises(RuntimeError) as e:
        prom.parse_device(True, torch.from_numpy(data).to(other), torch.from_numpy(off).to(other), 4, d_out, 2)
    assert "rc=%d " % binding.LC_ERR_ARG in str(e.value)


def test_bulk_generated_lines_against_the_host_routine():
    from loongcollector_amd import corpus, prom
    torch = _torch()
    lines = corpus.prom_exposition_lines(65536, deferred=0.05, failing=0.05)
    data, off = pack(lines)
    want = host_rows(data, off, True, 8)
    assert 2500 < np.count_nonzero(want["flags"] & pp.VALUE_HOST) < 4000 and 2500 < np.count_nonzero(want["status"]) < 4000
    same(device_rows(torch, data, off, True, 8), want, lines, "64 Ki lines")
    finished = host_rows(data, off, True, 8, finish=True)
    got = prom.parse_host(lines, True, W=8, fill=SENT)
    same(got, finished, lines, "64 Ki lines through the host entry")
    assert got["deferred"] == finished["finished"] > 2500


# ---------------------------------------------------------------------------------------------- the processor
def _metric(ev):
    return (ev["name"], ev["tags"], ev["bits"], ev["secs"], ev["nanos"])


@pytest.mark.parametrize("honor", [True, False])
def test_processor_on_1000_event_groups_against_the_cpu_double(honor):
    from loongcollector_amd import corpus, prom
    _torch()
    rng = random.Random(3)
    lines = corpus.prom_exposition_lines(1000, seed=77, deferred=0.05, failing=0.05)
    events = [None if rng.randrange(10) == 0 else ln for ln in lines]
    events[10] = b'up{__name__="shadowed",job="x"} 1'
    events[11] = b"m{%s} 7 1715829785083" % b",".join(b'l%d="v%d"' % (k, k) for k in range(23))
    config = {"job_name": "j", "honor_timestamps": honor}
    double = pp.Product(config)
    rc, want = double.process(events, 1700000000123)
    assert rc == 0 and 700 < len(want) < 950
    p = prom.PromProcessor(config)
    alarms = p.collect_alarms()
    group = prom.RawGroup(events, 1700000000123)
    p.process(group)
    got = group.events()
    assert [ev["type"] for ev in got] == [2] * len(want)
    assert [_metric(ev) for ev in got] == [_metric(ev) for ev in want]  # order, names, tags with __name__ last, bits, time
    assert got[0]["tags"][-1][0] == b"__name__" and any(ev["tags"][0] == (b"__name__", b"up") for ev in got)
    own_time = sum(1 for ev in got if ev["secs"] != 1700000000)
    assert (own_time > 400) if honor else (own_time == 0)
    c, d = p.counters(), double.counters()
    assert (c["discarded_events_total"], c["out_failed_events_total"], c["out_successful_events_total"]) == (d[pp.DISCARDED], d[pp.OUT_FAILED], d[pp.OUT_SUCCESSFUL])
    assert c["discarded_events_total"] == events.count(None) and p.deferred_tokens() == double.deferred_tokens() > 20
    assert p.mop_up_lines() == 1 and not alarms
    # the second trip through the knob: the same events with two labels kept by the first trip
    narrow = prom.PromProcessor(config)
    narrow.set_first_trip_labels(2)
    group = prom.RawGroup(events, 1700000000123)
    narrow.process(group)
    assert [_metric(ev) for ev in group.events()] == [_metric(ev) for ev in want] and narrow.mop_up_lines() > 300


def test_processor_without_scrape_timestamp_warns_and_uses_zero():
    from loongcollector_amd import prom
    _torch()
    p = prom.PromProcessor({"job_name": "j"})
    alarms = p.collect_alarms()
    group = prom.RawGroup([b"m 1", b"m 2 1715829785083"], "garbled")
    p.process(group)
    assert [(ev["secs"], ev["nanos"]) for ev in group.events()] == [(0, 0), (1715829785, 83000000)] and [k for k, _ in alarms] == [1]
