"""The SLS encoder on the device (include/sls/lc_sls.h): sls_size_kernel, the scan and sls_write_kernel against the bytes of
tests/helpers/sls_wire.py, the Python model that tests/test_sls_model.py holds to the reference's writer; the processor level against the
reference's bytes of tests/golden/sls_wire_vectors.json.  In the engine tests the capture rows and status bytes are written by the test:
no regex is in the way.  64 sentinel bytes stand on both sides of d_out[0 .. total), sentinel rows around d_rec_off."""
import ctypes
import json
import threading

import numpy as np
import pytest

from helpers import sls_cases as sc
from helpers import sls_wire
from loongcollector_amd import binding, sls

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
ROW_SENTINEL = -0x5A5A5A5A5A5A5A5B


def _device():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _layout(rows, form, residues):
    """-> data bytes, off (n or n + 1 entries), len or None, sep_bytes.  form "len": d_off + d_len, line i at a 4-byte boundary + residues[i]
    (bytes of another value between the lines); form "off": d_off[n + 1] with one separator byte behind every line"""
    if form == "off":
        data = b"".join(r[0] + b"\n" for r in rows)
        off = np.zeros(len(rows) + 1, np.uint32)
        off[1:] = np.cumsum([len(r[0]) + 1 for r in rows], dtype=np.uint64)
        return data, off, None, 1
    data, off = bytearray(), []
    for i, r in enumerate(rows):
        if residues is not None:
            while len(data) % 4 != residues[i]:
                data.append(0x7E)
        off.append(len(data))
        data += r[0]
    return bytes(data), np.array(off, np.uint32), np.array([len(r[0]) for r in rows], np.uint32), 0


class Batch:
    """rows = [(line, status, caps, time, ns or -1)] on the device, ready for lc_sls_encode_device"""

    def __init__(self, rows, form="len", residues=None, ns_null=False, ngroups=None):
        import torch
        dev = _device()
        self.rows, self.n = rows, len(rows)
        self.G = ngroups if ngroups is not None else (len(rows[0][2]) // 2 if rows else 1)
        data, off, length, self.sep = _layout(rows, form, residues)
        pad = (-len(data)) % 16 + 16
        self.d_data = torch.from_numpy(np.frombuffer(data + b"\0" * pad, np.uint8).copy()).to(dev)
        self.d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev) if self.n else torch.zeros(1, dtype=torch.int32, device=dev)
        self.d_len = torch.from_numpy(length.view(np.int32).copy()).to(dev) if length is not None and self.n else None
        caps = np.array([r[2] for r in rows], np.int32).reshape(self.n, 2 * self.G) if self.n else np.zeros((1, 2 * self.G), np.int32)
        self.d_caps = torch.from_numpy(caps).to(dev)
        self.d_status = torch.from_numpy(np.array([r[1] for r in rows] or [0], np.uint8)).to(dev)
        self.d_time = torch.from_numpy(np.array([r[3] for r in rows] or [0], np.uint32).view(np.int32).copy()).to(dev)
        self.d_ns = None if ns_null else torch.from_numpy(np.array([r[4] for r in rows] or [0], np.int32)).to(dev)
        self.d_scratch = torch.empty(sls.scratch_bytes(self.n), dtype=torch.uint8, device=dev)

    def encode(self, plan, enable_ns, d_out, out_cap, d_rec_off):
        import torch
        sls.encode_device(plan, self.d_data, self.d_off, self.d_len, self.sep, self.n, self.G, self.d_caps, self.d_status, self.d_time, self.d_ns,
                          enable_ns, d_out, out_cap, d_rec_off, self.d_scratch, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()


def _rec_rows(n):
    import torch
    return torch.full((n + 3,), ROW_SENTINEL, dtype=torch.int64, device=_device())


def _check_rec_rows(rec, n, offsets):
    got = rec.cpu().numpy()
    assert got[0] == ROW_SENTINEL and got[n + 2] == ROW_SENTINEL, "a row beside d_rec_off was written"
    assert np.array_equal(got[1:n + 2], offsets), "d_rec_off"


def run(spec, rows, enable_ns, form="len", residues=None, ns_null=False, ngroups=None, model_rows=None):
    """the batch through lc_sls_encode_device -- first without room (out_cap 0: d_rec_off must be complete and right), then with exactly
    total bytes between two runs of 64 sentinel bytes -- against the model.  -> (bytes, offsets)"""
    import torch
    keys, matched, unmatched = spec
    plan = sls.Plan(keys, matched, unmatched)
    sizes, want = sc.model_batch(keys, matched, unmatched, model_rows or rows, enable_ns and not ns_null)
    offsets = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
    b = Batch(rows, form, residues, ns_null, ngroups)
    rec = _rec_rows(b.n)
    b.encode(plan, enable_ns, None, 0, rec[1:])
    _check_rec_rows(rec, b.n, offsets)
    total = len(want)
    buf = torch.full((64 + total + 64,), SENTINEL, dtype=torch.uint8, device=_device())
    rec = _rec_rows(b.n)
    b.encode(plan, enable_ns, buf[64:], total, rec[1:])
    _check_rec_rows(rec, b.n, offsets)
    got = buf.cpu().numpy()
    assert (got[:64] == SENTINEL).all() and (got[64 + total:] == SENTINEL).all(), "a byte outside d_out[0 .. total) was written"
    data = got[64:64 + total].tobytes()
    if data != want:
        at = next(i for i in range(total) if data[i] != want[i])
        event = int(np.searchsorted(offsets, at, side="right")) - 1
        raise AssertionError("byte %d of %d differs (event %d, record bytes %d..%d): got %s, want %s" % (
            at, total, event, offsets[event], offsets[event + 1], data[at:at + 8].hex(), want[at:at + 8].hex()))
    return data, offsets


def _value(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ---------------------------------------------------------------------------------------------- 1. copy edges
COPY_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 65537]
COPY_PLANS = {
    "one_item_key_1": ([b"k"], [(0, 1)], [(0, 0)]),
    "one_item_key_130": ([b"K" * 130], [(0, 1)], [(0, 0)]),
    "three_items_keys_3_4_5": ([b"abc", b"abcd", b"abcde"], [(0, 1), (1, 0), (2, 2)], [(1, 0)]),
}


@pytest.mark.parametrize("name", sorted(COPY_PLANS))
def test_copy_edges_every_length_at_every_source_and_destination_residue(name):
    """per value length: 4 source residues x 16 destination residues.  A leading event of chosen length (an unmatched line, whose record is
    the line under the first key) sets the residue at which the record under test begins."""
    spec = COPY_PLANS[name]
    keys, matched, unmatched = spec
    rng = np.random.default_rng(17)
    rows, residues, at, seen = [], [], 0, set()
    for vlen in COPY_LENGTHS:
        for src in range(4):
            for dst in range(16):
                # the filler: the shortest unmatched line after which the offset has residue dst
                for fill in range(64):
                    filler = (b"f" * fill, 0, [-1, -1, -1, -1], 7, -1)
                    size = sc.model_batch(keys, matched, unmatched, [filler], 1)[0][0]
                    if (at + size) % 16 == dst:
                        break
                else:
                    raise AssertionError("no filler")
                rows.append(filler)
                residues.append(fill % 4)
                at += size
                seen.add((vlen, src, at % 16))
                # the value under test: group 1 of a line that begins one byte before it, so that the VALUE has source residue src
                line = b"<" + _value(rng, vlen) + b">"
                row = (line, 1, [1, 1 + vlen, 0, 1], 1700000000 + vlen, -1)
                rows.append(row)
                residues.append((src - 1) % 4)
                at += sc.model_batch(keys, matched, unmatched, [row], 1)[0][0]
    assert len(seen) == len(COPY_LENGTHS) * 64
    run(spec, rows, 1, form="len", residues=residues)


# ---------------------------------------------------------------------------------------------- 2. varint edges
def test_varint_edges_of_value_content_and_record_sizes():
    """one item under a one-byte key: vlen, the content size (vlen + 4 + its varints) and logSZ (+ 6, + 5 with ns) each pass 2^7 and 2^14
    inside the windows; with and without the nanosecond part, which moves logSZ's crossing"""
    spec = ([b"k"], [(0, 1)], [])
    rng = np.random.default_rng(2)
    rows = []
    for vlen in list(range(100, 140)) + list(range(16360, 16400)):
        line = _value(rng, vlen)
        rows.append((line, 1, [0, vlen], 1700000000, 5))
        rows.append((line, 1, [0, vlen], 1700000000, -1))
    sizes = sc.model_batch(*spec, rows, 1)[0]
    for border in (1 << 7, 1 << 14):   # (record size = logSZ + 1 + its varint: both sides of each border are there)
        assert min(sizes) < border < max(sizes)
    run(spec, rows, 1)
    run(spec, rows, 0)


def test_a_record_whose_size_crosses_2_to_the_21():
    spec = ([b"k"], [(0, 1)], [])
    rng = np.random.default_rng(3)
    rows = []
    for vlen in ((1 << 21) - 20, (1 << 21) - 19, (1 << 21) - 18, (1 << 21) - 17, (1 << 21) - 12, 1 << 21):
        rows.append((_value(rng, vlen), 1, [0, vlen], 1700000000, -1))
    log_sizes = [len(sls_wire.decode(sls_wire.record(t, None, [(b"k", line)], 0))[0][2]) for line, _, _, t, _ in rows]
    assert min(log_sizes) < 1 << 21 <= max(log_sizes)
    run(spec, rows, 0)


@pytest.mark.parametrize("enable_ns,ns_null", [(0, False), (1, False), (1, True), (0, True)])
def test_times_and_nanoseconds(enable_ns, ns_null):
    spec = ([b"time"], [(0, 1)], [(0, 0)])
    rows = []
    for t in (0, (1 << 28) - 1, 1 << 28, (1 << 32) - 1, 1700000000):
        for ns in (0, 999999999, -1, 1, -7):
            rows.append((b"abcdef", 1 if len(rows) % 3 else 0, [1, 4], t, ns))
    model_rows = [(l, s, c, t, ns if ns >= 0 else -1) for l, s, c, t, ns in rows]
    data, _ = run(spec, rows, enable_ns, ns_null=ns_null, model_rows=model_rows)
    assert (b"\x25" in data) == bool(enable_ns and not ns_null)


# ---------------------------------------------------------------------------------------------- 3. rows
ROW_KEYS = [b"whole", b"g1", b"g2", b"g3", b"g4", b"raw"]


def _row_cases():
    line = b"0123456789abcdefghijklmnopqrstuvwxyz"
    n = len(line)
    return [
        (line, 1, [-1, -1, -1, -1, -1, -1, -1, -1], 10, -1),          # no group took part
        (line, 1, [0, n, 0, n, 0, n, 0, n], 11, 3),                    # every group is the whole line: the values outweigh the line
        (line, 1, [2, 30, 5, 25, 10, 20, 15, 16], 12, -1),             # nested
        (line, 1, [0, 20, 10, 30, 15, n, 5, 6], 13, 4),                # overlapping; group 3 ends at the line's last byte
        (line, 1, [n - 1, n, n, n, 0, 0, -1, -1], 14, -1),             # the last byte, empty groups at both ends
        (b"", 1, [0, 0, -1, -1, 0, 0, -1, -1], 15, 5),                 # an empty line that matched
        (b"x", 1, [0, 1, 0, 1, -1, -1, 0, 0], 16, -1),
    ]


@pytest.mark.parametrize("form", ["len", "off"])
@pytest.mark.parametrize("unmatched", [[], [(5, 0)], [(5, 0), (0, 0)]])
def test_rows_groups_status_bytes_and_both_offset_forms(form, unmatched):
    """every status byte 0..5 next to its neighbours (only LC_MATCH = 1 takes the matched list); with an empty unmatched list records vanish
    from the middle of a wavefront and rec_off repeats"""
    spec = (ROW_KEYS, [(1, 1), (0, 0), (2, 2), (3, 3), (4, 4)], unmatched)
    cases = _row_cases()
    rows = []
    for k in range(300):
        line, _, caps, t, ns = cases[k % len(cases)]
        rows.append((line, (k * 7 + k // 6) % 6, caps, t + k, ns))
    assert {r[1] for r in rows} == set(range(6))
    data, offsets = run(spec, rows, 1, form=form)
    repeats = int((np.diff(offsets) == 0).sum())
    assert (repeats > 100) == (not unmatched) and len(data) > 5000


def test_a_row_outside_its_line_is_cut_to_it():
    """what lc_regex_match_device never writes: the header defines it (cut to the line, or the empty value)"""
    spec = ([b"a", b"b", b"c"], [(0, 1), (1, 2), (2, 3)], [])
    line = b"0123456789"
    rows = [(line, 1, [5, 50, 12, 20, 7, 3], 9, -1)]
    model_rows = [(line, 1, [5, 10, -1, -1, -1, -1], 9, -1)]
    run(spec, rows, 0, model_rows=model_rows)


# ---------------------------------------------------------------------------------------------- 4. counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1022, 1023, 1024, 1025, 2047, 2048, 4095])
def test_counts_around_the_wavefront_the_block_and_the_scan_s_tile(n):
    """the scan works on n + 1 entries in tiles of 1024: n = 1023 fills one tile exactly"""
    spec = ([b"k", b"u"], [(0, 1), (1, 0)], [(1, 0)])
    rows = [(b"line %d %s" % (i, b"x" * (i % 13)), 0 if i % 5 == 2 else 1, [5, 6 + len(str(i)) - 1], 1700000000 + i, i if i % 2 else -1) for i in range(n)]
    run(spec, rows, 1, form="off" if n % 2 else "len", ngroups=1)


def test_a_batch_that_needs_more_than_one_pass_over_the_tile_sums():
    """more than 1024 tiles of 1024 entries: 1 Mi + 5 lines of one byte, every third without a record; the expected bytes are built with
    numpy from the model's record of one line"""
    import torch
    n = (1 << 20) + 5
    dev = _device()
    spec = ([b"k"], [(0, 0)], [])
    plan = sls.Plan(*spec)
    record = sls_wire.record(1700000000, None, [(b"k", b"z")], 0)
    status = (np.arange(n) % 3 != 1).astype(np.uint8)
    offsets = np.concatenate([[0], np.cumsum(status.astype(np.int64) * len(record))])
    total = int(offsets[-1])
    d_data = torch.full((n + 32,), ord("z"), dtype=torch.uint8, device=dev)
    d_off = torch.arange(n, dtype=torch.int32, device=dev)
    d_len = torch.ones(n, dtype=torch.int32, device=dev)
    d_status = torch.from_numpy(status).to(dev)
    d_time = torch.full((n,), 1700000000, dtype=torch.int32, device=dev)
    d_scratch = torch.empty(sls.scratch_bytes(n), dtype=torch.uint8, device=dev)
    assert sls.scratch_bytes(n) >= 1025 * 8
    rec = _rec_rows(n)
    buf = torch.full((64 + total + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    sls.encode_device(plan, d_data, d_off, d_len, 0, n, 0, None, d_status, d_time, None, 0, buf[64:], total, rec[1:], d_scratch,
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check_rec_rows(rec, n, offsets)
    got = buf.cpu().numpy()
    assert (got[:64] == SENTINEL).all() and (got[64 + total:] == SENTINEL).all()
    want = np.tile(np.frombuffer(record, np.uint8), int(status.sum()))
    assert np.array_equal(got[64:64 + total], want)


# ---------------------------------------------------------------------------------------------- 5. out_cap
def test_out_cap_too_small_stores_nothing_and_two_runs_give_the_same_bytes():
    import torch
    spec = COPY_PLANS["three_items_keys_3_4_5"]
    rng = np.random.default_rng(5)
    rows = []
    for i in range(700):
        vlen = int(rng.integers(0, 90))
        rows.append((b"<" + _value(rng, vlen) + b">", int(i % 4 != 3), [1, 1 + vlen, 0, 1], 1700000000 + i, int(rng.integers(0, 10 ** 9)) if i % 2 else -1))
    data, offsets = run(spec, rows, 1)
    total = len(data)
    plan = sls.Plan(*spec)
    b = Batch(rows)
    for cap in (total - 1, 0, 1):
        buf = torch.full((64 + total + 64,), SENTINEL, dtype=torch.uint8, device=_device())
        rec = _rec_rows(b.n)
        b.encode(plan, 1, buf[64:], cap, rec[1:])
        _check_rec_rows(rec, b.n, offsets)
        assert (buf.cpu().numpy() == SENTINEL).all(), "out_cap %d of %d: a byte was stored" % (cap, total)
    for cap in (total, total + 1000):
        buf = torch.full((64 + total + 64,), SENTINEL, dtype=torch.uint8, device=_device())
        rec = _rec_rows(b.n)
        b.encode(plan, 1, buf[64:], cap, rec[1:])
        got = buf.cpu().numpy()
        assert got[64:64 + total].tobytes() == data and (got[64 + total:] == SENTINEL).all()


def test_refused_arguments():
    import torch
    plan = sls.Plan([b"k"], [(0, 2)], [])
    b = Batch([(b"abc", 1, [0, 1, 1, 2], 5, -1)])
    out = torch.zeros(256, dtype=torch.uint8, device=_device())
    rec = torch.zeros(8, dtype=torch.int64, device=_device())

    def rc(d_out=None, d_rec=None, ngroups=2, scratch=None, n=1):
        return sls.encode_device_rc(plan, b.d_data.data_ptr(), b.d_off.data_ptr(), b.d_len.data_ptr(), 0, n, ngroups, b.d_caps.data_ptr(),
                                    b.d_status.data_ptr(), b.d_time.data_ptr(), None, 0, d_out if d_out is not None else out.data_ptr(), 128,
                                    d_rec if d_rec is not None else rec.data_ptr(), b.d_scratch.data_ptr(),
                                    b.d_scratch.numel() if scratch is None else scratch)
    assert rc(d_out=out.data_ptr() + 8) == binding.LC_ERR_ARG          # d_out: 16 bytes
    assert rc(d_rec=rec.data_ptr() + 4) == binding.LC_ERR_ARG          # d_rec_off: 8 bytes
    assert rc(ngroups=1) == binding.LC_ERR_ARG                         # the plan names group 2
    assert rc(scratch=0) == binding.LC_ERR_ARG
    assert rc(n=1 << 31) == binding.LC_ERR_ARG
    assert rc() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 6. the processor level
def _real_serialize(L, proc, fixture, enable_ns):
    g = sc.group_handle(L, fixture)
    before = sc.group_json(L, g)
    data, fused = proc.serialize(g, enable_ns)
    assert sc.group_json(L, g) == before
    L.lc_group_free(g)
    return data, fused


def test_every_golden_vector_through_the_processor_gives_the_reference_s_bytes_and_the_twin_s_counters():
    L = binding.load()
    sls.load()
    procs, twins, fused_groups = {}, {}, 0
    binding.launched_kernels()
    for v in sc.load_golden():
        name = json.dumps(v["config"], sort_keys=True)
        if name not in procs:
            procs[name], twins[name] = sls.Processor(v["config"]), sc.Twin(L, v["config"])
        data, fused = _real_serialize(L, procs[name], v["group"], v["enable_ns"])
        assert data == bytes.fromhex(v["bytes"]), (v["config"], v["group"])
        assert fused == (1 if all(len(e["contents"]) == 1 for e in v["group"]["events"]) else 0)   # (the two-content group: the host path)
        fused_groups += fused
        g = sc.group_handle(L, v["group"])
        twins[name].process(g)
        L.lc_group_free(g)
    kernels = binding.launched_kernels()
    assert fused_groups == 52 and "sls_size_kernel" in kernels and "sls_write_kernel" in kernels
    for name, p in procs.items():
        c = p.counters()
        assert {k: c[k] for k in sls.PARSE_COUNTERS} == twins[name].counters(), name
        assert c["failed_trips"] == 0


def test_match_encode_host_with_rows_that_outgrow_the_first_download():
    """a plan that writes the line beside nested groups: the payload exceeds the bound the first download takes, the second brings all"""
    rx = binding.GpuRegex(rb"((\w+) (\w+)) (.*)")
    spec = ([b"both", b"first", b"second", b"rest", b"line"], [(0, 1)] * 6 + [(1, 2), (2, 3), (3, 4), (4, 0), (4, 0)], [(4, 0)])
    plan = sls.Plan(*spec)
    lines = [b"a" * 20 + b" " + b"b" * 21 + b" " + b"r" * (i % 90) if i % 7 else b"-" for i in range(500)]
    times = [1700000000 + i for i in range(500)]
    ns = [i if i % 3 else -1 for i in range(500)]
    data, rec_off, status = sls.match_encode_host(plan, rx, lines, times, ns, 1)
    rows = []
    for line, st, t, n in zip(lines, status, times, ns):
        rows.append((line, int(st), [0, 42, 0, 20, 21, 42, 43, len(line)] if st == 1 else [-1] * 8, t, n))
    assert int(status.sum()) == 500 - len(range(0, 500, 7))
    sizes, want = sc.model_batch(*spec, rows, 1)
    assert data == want and list(rec_off) == list(np.concatenate([[0], np.cumsum(sizes)]))
    again, none, _ = sls.match_encode_host(plan, rx, lines, times, None, 1, want_rec_off=False)
    assert none is None and again == sc.model_batch(*spec, [(l, s, c, t, -1) for l, s, c, t, _ in rows], 0)[1]


def test_eight_runner_threads_share_one_processor_on_groups_of_different_sizes():
    L = binding.load()
    config = sc.configs()[7]
    proc = sls.Processor(config)
    keys, matched, unmatched = sc.plan_of(config)
    jobs = {}
    for t in range(8):
        for k in range(5):
            group = sc.group(100 * t + k, n=1 + 61 * t + k)
            rows, _ = sc.engine_rows(config, group)
            jobs[(t, k)] = (group, sc.model_batch(keys, matched, unmatched, rows, 1)[1])
    errors = []

    def runner(t):
        try:
            held = None
            for k in range(5):
                group, want = jobs[(t, k)]
                g = sc.group_handle(L, group)
                if held is not None:          # the view of this thread's call before, while the other threads made theirs
                    assert ctypes.string_at(held[0], held[1]) == held[2]
                out, n, fused = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
                assert sls.load().lc_sls_processor_serialize(proc._h, g, 1, ctypes.byref(out), ctypes.byref(n), ctypes.byref(fused)) == 0
                L.lc_group_free(g)
                assert fused.value == 1 and ctypes.string_at(out, n.value) == want
                held = (out, n.value, want)
            sls.load().lc_sls_thread_release()
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=runner, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
    assert proc.counters()["groups_device"] == 40


def test_append_tags_equals_the_model():
    pairs = [(b"__topic__", b"topic-1"), (b"__source__", b"10.1.2.3"), (b"__machine_uuid__", b"uuid"), (b"host", b"h" * 300), (b"", b""),
             (b"__tag__:__path__", b"/var/log/" + b"x" * 16384)]
    got = sls.append_tags(pairs)
    assert got == sls_wire.tags(pairs)
    assert [(f, w) for f, w, _ in sls_wire.decode(got)] == [(3, 2), (4, 2), (5, 2), (6, 2), (6, 2), (6, 2)]
    with pytest.raises(OverflowError):
        sls.append_tags(pairs, cap=len(got) - 1)
