"""The JSON-lines encoder on the device (include/jsonl/lc_jsonl.h): jsonl_size_kernel, the scan and jsonl_write_kernel against the bytes of
tests/helpers/jsonl_model.py, the Python model that tests/test_jsonl_model.py holds to its witness; the processor level against the
model's bytes of tests/golden/jsonl_vectors.json.  In the engine tests the capture rows and status bytes are written by the test: no
regex is in the way.  64 sentinel bytes stand on both sides of d_out[0 .. total), sentinel rows around d_rec_off.

First-run durations on the MI355X: docs/NEXT.md section 14."""
import ctypes
import threading

import numpy as np
import pytest

import test_jsonl_host as host
from helpers import jsonl_cases as jc
from helpers import jsonl_model as jm
from helpers import sls_cases as sc
from loongcollector_amd import binding, jsonl

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
ROW_SENTINEL = -0x5A5A5A5A5A5A5A5B
LANES = 8                 # lanes per event in jsonl_write_kernel (csrc/jsonl_device.hip); jsonl_size_kernel has 4: its stride is 64 bytes
W = LANES * 16            # the bytes a sub-group of the write kernel takes per round
ONE = ([b"v"], [(0, 0)], [(0, 0)])


def _device():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _layout(rows, form, residues):
    """-> data bytes, off (n or n + 1 entries), len or None, sep_bytes.  form "len": d_off + d_len, line i at a 16-byte boundary +
    residues[i] (bytes of another value between the lines, reactive ones among them); form "off": d_off[n + 1] with one separator byte
    behind every line"""
    if form == "off":
        data = b"".join(r[0] + b"\n" for r in rows)
        off = np.zeros(len(rows) + 1, np.uint32)
        off[1:] = np.cumsum([len(r[0]) + 1 for r in rows], dtype=np.uint64)
        return data, off, None, 1
    data, off = bytearray(), []
    for i, r in enumerate(rows):
        if residues is not None:
            while len(data) % 16 != residues[i % len(residues)]:
                data += b'"\x00\x01\\'[len(data) % 4:len(data) % 4 + 1]
        off.append(len(data))
        data += r[0]
    return bytes(data), np.array(off, np.uint32), np.array([len(r[0]) for r in rows], np.uint32), 0


class Batch:
    """rows = [(line, status, caps, time)] on the device, ready for lc_jsonl_encode_device"""

    def __init__(self, plan, rows, head, form="len", residues=None, ngroups=None):
        import torch
        dev = _device()
        self.plan, self.rows, self.n = plan, rows, len(rows)
        self.G = ngroups if ngroups is not None else (len(rows[0][2]) // 2 if rows else 1)
        data, off, length, self.sep = _layout(rows, form, residues)
        pad = (-len(data)) % 16 + 16
        self.d_data = torch.from_numpy(np.frombuffer(data + b'"' * pad, np.uint8).copy()).to(dev)
        self.d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev) if self.n else torch.zeros(1, dtype=torch.int32, device=dev)
        self.d_len = torch.from_numpy(length.view(np.int32).copy()).to(dev) if length is not None and self.n else None
        caps = np.array([r[2] for r in rows], np.int32).reshape(self.n, 2 * self.G) if self.n else np.zeros((1, max(1, 2 * self.G)), np.int32)
        self.d_caps = torch.from_numpy(caps).to(dev) if self.G else None
        self.d_status = torch.from_numpy(np.array([r[1] for r in rows] or [0], np.uint8)).to(dev)
        self.d_time = torch.from_numpy(np.array([r[3] for r in rows] or [0], np.uint32).view(np.int32).copy()).to(dev)
        self.head_len = len(head)
        self.d_head = torch.from_numpy(np.frombuffer(head + b"\0" * ((-len(head)) % 4), np.uint8).copy()).to(dev)
        self.d_scratch = torch.empty(max(8, jsonl.scratch_bytes(plan, self.n)), dtype=torch.uint8, device=dev)

    def encode(self, d_out, out_cap, d_rec_off):
        import torch
        jsonl.encode_device(self.plan, self.d_data, self.d_off, self.d_len, self.sep, self.n, self.G, self.d_caps, self.d_status, self.d_time,
                            self.d_head, self.head_len, d_out, out_cap, d_rec_off, self.d_scratch, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()


def _rec_rows(n):
    import torch
    return torch.full((n + 3,), ROW_SENTINEL, dtype=torch.int64, device=_device())


def _check_rec_rows(rec, n, offsets):
    got = rec.cpu().numpy()
    assert got[0] == ROW_SENTINEL and got[n + 2] == ROW_SENTINEL, "a row beside d_rec_off was written"
    assert np.array_equal(got[1:n + 2], offsets), "d_rec_off"


def run(spec, rows, tags=(), form="len", residues=None, ngroups=None, model_rows=None):
    """the batch through lc_jsonl_encode_device -- first without room (out_cap 0: d_rec_off must be complete and right), then with exactly
    total bytes between two runs of 64 sentinel bytes -- against the model.  The head is the model's.  -> (bytes, offsets)"""
    import torch
    keys, matched, unmatched = spec
    plan = jsonl.Plan(keys, matched, unmatched)
    sizes, want = jc.model_batch(keys, matched, unmatched, model_rows or rows, tags)
    offsets = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
    b = Batch(plan, rows, jm.head(tags), form, residues, ngroups)
    rec = _rec_rows(b.n)
    b.encode(None, 0, rec[1:])
    _check_rec_rows(rec, b.n, offsets)
    total = len(want)
    buf = torch.full((64 + total + 64,), SENTINEL, dtype=torch.uint8, device=_device())
    rec = _rec_rows(b.n)
    b.encode(buf[64:], total, rec[1:])
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


# ---------------------------------------------------------------------------------------------- 1. every byte value
def test_every_byte_value_and_each_reactive_byte_at_every_position_at_every_residue():
    """one-byte values 0x00 .. 0xFF; each reactive byte at positions 0 .. 17 of an 18-byte value; every line start residue 0 .. 15; the
    records' sizes vary, so that every destination residue 0 .. 3 is met by a record's first byte and by a value's"""
    plain = b"abcdefghijklmnopqr"
    values = [bytes([c]) for c in range(256)]
    for r in host.REACTIVE:
        values += [plain[:at] + r + plain[at + 1:] for at in range(18)]
    rows, residues = [], []
    for res in range(16):
        for k, v in enumerate(values):
            rows.append((v, (k + res) % 2, [], 10 ** (k % 10)))
            residues.append(res)
    _, offsets = run(ONE, rows, residues=residues)
    assert {int(o) % 4 for o in offsets} == {0, 1, 2, 3}


@pytest.mark.parametrize("kind", ["reactive", "nul"])
def test_unit_and_round_borders(kind):
    """a reactive byte, and separately a NUL, on positions 15 / 16 / 17, 63 / 64 / 65, W - 1 / W / W + 1 and the same around 2 W of a value
    of 2 W + 40 bytes, W = lanes per event x 16, for every line residue; the value is group 1, behind 3 bytes of the line"""
    spec = ([b"g", b"l"], [(0, 1), (1, 0)], [])
    rows, residues = [], []
    base = bytes(97 + i % 26 for i in range(2 * W + 43))
    for res in range(16):
        for at in (15, 16, 17, 63, 64, 65, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1):
            for byte in ((b'"', b"\x01", b"\n") if kind == "reactive" else (b"\0",)):
                line = bytearray(base)
                line[3 + at] = byte[0]
                if kind == "nul":
                    line[3 + at + 5] = 0x22           # behind the NUL: must not count or appear
                rows.append((bytes(line), 1, [3, len(line)], 1700000000))
                residues.append(res)
    run(spec, rows, residues=residues)


# ---------------------------------------------------------------------------------------------- 2. the host test's edge batches
def _edges():
    return host.edge_batches()


@pytest.mark.parametrize("part", range(4))
def test_edge_batches_nul_lengths_clean_dirty_and_six_fold_time_digits_and_heads(part):
    """tests/test_jsonl_host.py::edge_batches on the device: NULs (at 0, 1, 15, 16, 17, last, two, reactive bytes behind one, in a key and
    in a tag), every length of LENGTHS clean / with one reactive byte / all 0x01, a clean item behind a dirty one and the reverse, times
    of 1 to 10 digits under heads of 12 bytes to 4 KiB.  Line residues 0 .. 15 in turn."""
    batches = _edges()
    assert len(batches) == 3 + 3 * len(host.LENGTHS) + 1 + 5
    for k, (keys, matched, unmatched, rows, tags) in enumerate(batches):
        if k % 4 != part:
            continue
        G = max([len(r[2]) // 2 for r in rows] + [0])
        rows = [(line, st, list(caps) + [-1] * (2 * G - len(caps)), t) for line, st, caps, t in rows]
        run((keys, matched, unmatched), rows, tags, residues=[(k + 5 * i) % 16 for i in range(16)], ngroups=G,
            model_rows=[(line, st, _cut(caps, len(line)), t) for line, st, caps, t in rows])


def _cut(caps, n):
    """the header's rule for a row outside its line, for the model"""
    out = []
    for b, e in zip(caps[0::2], caps[1::2]):
        out += [-1, -1] if (b < 0 or e <= b or b >= n) else [b, min(e, n)]
    return out


def test_heads_of_every_residue():
    """heads of 12, 13, 14, 15 ... 27 bytes and one of 4 KiB: every residue of the position where the time and the first item begin.  A tag
    adds six bytes or more, so the lengths between are made with blanks behind the brace, which the entry copies like any head"""
    import json
    import torch
    plan = jsonl.Plan(*ONE)
    rows = [(b"value %d" % i, 1, [], 10 ** (i % 10) - (i % 2)) for i in range(40)]
    for blanks in list(range(16)) + [4084]:
        head = b"{" + b" " * blanks + b'"__time__":'
        want = b"".join(head + b"%d" % t + b',"v":"' + line + b'"}\n' for line, _, _, t in rows)
        b = Batch(plan, rows, head, residues=[3], ngroups=0)
        buf = torch.full((64 + len(want) + 64,), SENTINEL, dtype=torch.uint8, device=_device())
        rec = _rec_rows(b.n)
        b.encode(buf[64:], len(want), rec[1:])
        got = buf.cpu().numpy()
        assert got[64:64 + len(want)].tobytes() == want, len(head)
        assert (got[:64] == SENTINEL).all() and (got[64 + len(want):] == SENTINEL).all()
        assert [json.loads(x)["__time__"] for x in want.split(b"\n")[:-1]] == [r[3] for r in rows]


# ---------------------------------------------------------------------------------------------- 3. rows
ROW_KEYS = [b"whole", b"g1", b"g2", b"g3", b"g4", b"raw"]


def _row_cases():
    line = b'01234"6789ab\\defghijklm\x01opqrstuvwxy"'
    n = len(line)
    return [
        (line, 1, [-1, -1, -1, -1, -1, -1, -1, -1], 10),          # no group took part
        (line, 1, [0, n, 0, n, 0, n, 0, n], 11),                    # every group is the whole line: the values outweigh the line
        (line, 1, [2, 30, 5, 25, 10, 20, 15, 16], 12),             # nested
        (line, 1, [0, 20, 10, 30, 15, n, 5, 6], 13),                # overlapping; group 3 ends at the line's last byte
        (line, 1, [n - 1, n, n, n, 0, 0, -1, -1], 14),             # the last byte, empty groups at both ends
        (b"", 1, [0, 0, -1, -1, 0, 0, -1, -1], 15),                 # an empty line that matched
        (b"x", 1, [0, 1, 0, 1, -1, -1, 0, 0], 16),
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
        line, _, caps, t = cases[k % len(cases)]
        rows.append((line, (k * 7 + k // 6) % 6, caps, t + k))
    assert {r[1] for r in rows} == set(range(6))
    data, offsets = run(spec, rows, [(b"t", b"v")], form=form)
    repeats = int((np.diff(offsets) == 0).sum())
    assert (repeats > 100) == (not unmatched) and len(data) > 5000


def test_a_row_outside_its_line_is_cut_to_it():
    """what lc_regex_match_device never writes: the header defines it (cut to the line, or the empty value)"""
    spec = ([b"a", b"b", b"c"], [(0, 1), (1, 2), (2, 3)], [])
    line = b'01234"6789'
    run(spec, [(line, 1, [5, 50, 12, 20, 7, 3], 9)], model_rows=[(line, 1, [5, 10, -1, -1, -1, -1], 9)])


# ---------------------------------------------------------------------------------------------- 4. counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 4095])
def test_counts_around_the_wavefront_the_block_and_the_scan_s_tile(n):
    """the scan works on n + 1 entries in tiles of 1024: n = 1023 fills one tile exactly"""
    spec = ([b"k", b"u"], [(0, 1), (1, 0)], [(1, 0)])
    rows = [(b'line %d "%s' % (i, b"x" * (i % 13)), 0 if i % 5 == 2 else 1, [5, 6 + len(str(i)) - 1], 1700000000 + i) for i in range(n)]
    run(spec, rows, form="off" if n % 2 else "len", ngroups=1)


def test_a_batch_that_needs_more_than_one_pass_over_the_tile_sums():
    """more than 1024 tiles of 1024 entries: 1 Mi + 5 empty lines, every third without a record; the expected bytes are built with numpy
    from the model's record of one line"""
    import torch
    n = (1 << 20) + 5
    dev = _device()
    plan = jsonl.Plan([b"k"], [(0, 0)], [])
    record = jm.record(1700000000, [(b"k", b"")])
    status = (np.arange(n) % 3 != 1).astype(np.uint8)
    offsets = np.concatenate([[0], np.cumsum(status.astype(np.int64) * len(record))])
    total = int(offsets[-1])
    d_data = torch.full((32,), 0x22, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n, dtype=torch.int32, device=dev)
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    d_status = torch.from_numpy(status).to(dev)
    d_time = torch.full((n,), 1700000000, dtype=torch.int32, device=dev)
    d_head = torch.from_numpy(np.frombuffer(jm.head(), np.uint8).copy()).to(dev)
    assert jsonl.scratch_bytes(plan, n) >= 1025 * 8 + n * 8
    d_scratch = torch.empty(jsonl.scratch_bytes(plan, n), dtype=torch.uint8, device=dev)
    rec = _rec_rows(n)
    buf = torch.full((64 + total + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    jsonl.encode_device(plan, d_data, d_off, d_len, 0, n, 0, None, d_status, d_time, d_head, 12, buf[64:], total, rec[1:], d_scratch,
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
    spec = ([b"abc", b"abcd", b"abcde"], [(0, 1), (1, 0), (2, 2)], [(1, 0)])
    rng = np.random.default_rng(5)
    rows = []
    for i in range(700):
        vlen = int(rng.integers(0, 90))
        value = rng.integers(0, 256 if i % 3 else 64, vlen, dtype=np.uint8).tobytes()
        rows.append((b"<" + value + b">", int(i % 4 != 3), [1, 1 + vlen, 0, 1], 1700000000 + i))
    tags = [(b"t", b"v")]
    data, offsets = run(spec, rows, tags)
    total = len(data)
    plan = jsonl.Plan(*spec)
    b = Batch(plan, rows, jm.head(tags))
    for cap in (total - 1, 0, 1):
        buf = torch.full((64 + total + 64,), SENTINEL, dtype=torch.uint8, device=_device())
        rec = _rec_rows(b.n)
        b.encode(buf[64:], cap, rec[1:])
        _check_rec_rows(rec, b.n, offsets)
        assert (buf.cpu().numpy() == SENTINEL).all(), "out_cap %d of %d: a byte was stored" % (cap, total)
    for cap in (total, total + 1000):
        buf = torch.full((64 + total + 64,), SENTINEL, dtype=torch.uint8, device=_device())
        rec = _rec_rows(b.n)
        b.encode(buf[64:], cap, rec[1:])
        got = buf.cpu().numpy()
        assert got[64:64 + total].tobytes() == data and (got[64 + total:] == SENTINEL).all()


def test_refused_arguments():
    import torch
    plan = jsonl.Plan([b"k"], [(0, 2)], [])
    b = Batch(plan, [(b"abc", 1, [0, 1, 1, 2], 5)], jm.head())
    out = torch.zeros(256, dtype=torch.uint8, device=_device())
    rec = torch.zeros(8, dtype=torch.int64, device=_device())

    def rc(d_out=None, d_rec=None, ngroups=2, scratch=None, n=1, d_head=None, head_len=12, d_time=None, d_scratch=None):
        return jsonl.encode_device_rc(plan, b.d_data.data_ptr(), b.d_off.data_ptr(), b.d_len.data_ptr(), 0, n, ngroups, b.d_caps.data_ptr(),
                                      b.d_status.data_ptr(), d_time if d_time is not None else b.d_time.data_ptr(),
                                      d_head if d_head is not None else b.d_head.data_ptr(), head_len,
                                      d_out if d_out is not None else out.data_ptr(), 128, d_rec if d_rec is not None else rec.data_ptr(),
                                      d_scratch if d_scratch is not None else b.d_scratch.data_ptr(),
                                      b.d_scratch.numel() if scratch is None else scratch)
    assert rc(d_out=out.data_ptr() + 8) == binding.LC_ERR_ARG          # d_out: 16 bytes
    assert rc(d_rec=rec.data_ptr() + 4) == binding.LC_ERR_ARG          # d_rec_off: 8 bytes
    assert rc(d_scratch=b.d_scratch.data_ptr() + 4) == binding.LC_ERR_ARG
    assert rc(d_time=b.d_time.data_ptr() + 2) == binding.LC_ERR_ARG
    assert rc(d_head=b.d_head.data_ptr() + 2) == binding.LC_ERR_ARG    # d_head: 4 bytes
    assert rc(head_len=11) == binding.LC_ERR_ARG
    assert rc(head_len=65537) == binding.LC_ERR_ARG
    assert rc(ngroups=1) == binding.LC_ERR_ARG                         # the plan names group 2
    assert rc(scratch=0) == binding.LC_ERR_ARG
    assert rc(n=1 << 31) == binding.LC_ERR_ARG
    assert rc() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 6. the host entry and the processor level
def _real_serialize(L, proc, fixture):
    g = sc.group_handle(L, fixture)
    before = sc.group_json(L, g)
    data, fused = proc.serialize(g)
    assert sc.group_json(L, g) == before
    L.lc_group_free(g)
    return data, fused


def test_match_encode_host_with_escapes_that_outgrow_the_first_block():
    """all-control values: six bytes for one, beyond the bound the first write gets; the write kernel is queued once more"""
    rx = binding.GpuRegex(rb"(\w+) (.*)")
    spec = ([b"first", b"rest", b"line"], [(0, 1), (1, 2)], [(2, 0)])
    plan = jsonl.Plan(*spec)
    lines = [b"a" * 20 + b" " + b"\x01" * (i % 90) + b'"\0zz' if i % 7 else b"\x02-" for i in range(500)]
    times = [1700000000 + i for i in range(500)]
    tags = [(b"t", b'v"')]
    jsonl.load().lc_jsonl_thread_release()        # a fresh block: the first write cannot have room by chance
    binding.launched_kernels()
    data, rec_off, status = jsonl.match_encode_host(plan, rx, lines, times, jm.head(tags))
    assert "jsonl_write_kernel" in binding.launched_kernels()
    rows = [(line, int(st), [0, 20, 21, len(line)] if st == 1 else [-1] * 4, t) for line, st, t in zip(lines, status, times)]
    assert int(status.sum()) == 500 - len(range(0, 500, 7))
    sizes, want = jc.model_batch(*spec, rows, tags)
    # the room of the first write: per line the head, ten digits, }\n and the matched list's prefixes and quotes, plus the lines' bytes
    bound = 500 * (len(jm.head(tags)) + 12 + len(b',"first":""') + len(b',"rest":""')) + sum(len(x) for x in lines)
    assert len(want) > bound + 4096
    assert data == want and list(rec_off) == list(np.concatenate([[0], np.cumsum(sizes)]))
    again, none, _ = jsonl.match_encode_host(plan, rx, lines, times, jm.head(tags), want_rec_off=False)
    assert none is None and again == want


def test_eight_runner_threads_share_one_processor_on_groups_of_different_sizes():
    L = binding.load()
    config = sc.configs()[7]
    proc = jsonl.Processor(config)
    jobs = {}
    for t in range(8):
        for k in range(5):
            group = jc.group(100 * t + k, jc.TAG_SETS[(t + k) % 3])
            group["events"] = (group["events"] * (1 + 8 * t))[:1 + 61 * t + k]
            jobs[(t, k)] = (group, jc.model_batch(*jc.engine_batch(config, group))[1])
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
                assert jsonl.load().lc_jsonl_processor_serialize(proc._h, g, ctypes.byref(out), ctypes.byref(n), ctypes.byref(fused)) == 0
                L.lc_group_free(g)
                assert fused.value == 1 and ctypes.string_at(out, n.value) == want
                held = (out, n.value, want)
            jsonl.load().lc_jsonl_thread_release()
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=runner, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
    assert proc.counters()["groups_device"] == 40


def test_every_golden_vector_through_the_processor_gives_the_model_s_bytes_and_the_twin_s_counters():
    """fused = 1 for every golden group (events that hold the source content alone); the same group with a second content, with a non-log
    event and with a head beyond the bound is served on the host path with the same bytes"""
    L = binding.load()
    jsonl.load()
    binding.launched_kernels()
    fused_groups = 0
    for v in jc.load_golden():
        if v["kind"] != "group":
            continue
        proc, twin = jsonl.Processor(v["config"]), sc.Twin(L, v["config"])
        data, fused = _real_serialize(L, proc, v["group"])
        assert data == bytes.fromhex(v["bytes"]), (v["config"], v["group"])
        fused_groups += fused
        mixed = dict(v["group"], events=v["group"]["events"][:2] + [{"type": 3, "content": "raw"}] + v["group"]["events"][2:])
        assert _real_serialize(L, proc, mixed) == (data, 0)
        big = dict(v["group"], tags=dict(v["group"].get("tags", {}), zzbig="v" * 65536))
        assert _real_serialize(L, proc, big) == (jc.model_batch(*jc.engine_batch(v["config"], big))[1], 0)
        for fixture in (v["group"], mixed, big):
            g = sc.group_handle(L, fixture)
            twin.process(g)
            L.lc_group_free(g)
        c = proc.counters()
        assert {k: c[k] for k in jsonl.PARSE_COUNTERS} == twin.counters(), v["config"]
        assert (c["groups_device"], c["groups_host"], c["failed_trips"]) == (1, 2, 0)
    kernels = binding.launched_kernels()
    assert fused_groups == 26 and "jsonl_size_kernel" in kernels and "jsonl_write_kernel" in kernels


def test_a_second_content_takes_the_host_path():
    L = binding.load()
    v = jc.load_golden()[3]
    proc, twin = jsonl.Processor(v["config"]), sc.Twin(L, v["config"])
    two = dict(v["group"], events=[dict(e, contents={"content": e["contents"]["content"], "zz": 'ex"tra'}) for e in v["group"]["events"]])
    data, fused = _real_serialize(L, proc, two)
    assert fused == 0 and data == jm.records(jc.left_events(L, twin, two), jc.tags_of(two))
    c = proc.counters()
    assert {k: c[k] for k in jsonl.PARSE_COUNTERS} == twin.counters() and (c["groups_device"], c["groups_host"]) == (0, 1)
