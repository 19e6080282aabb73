"""The LZ4 block writer on the device (include/lz4/lc_lz4.h): lz4_match_kernel, the scans, lz4_size_kernel and lz4_emit_kernel against the
host routine of csrc/lz4_vm.hpp (tests/native/lz4_host_check.cpp, built here as a plain program) -- bit for bit -- and against the strict
Python decoder of tests/helpers/lz4_block.py.  64 sentinel bytes stand on both sides of d_out[0 .. total), sentinel rows around
d_out_off.  The shapes are the ones at which these kernels can go wrong (tests/helpers/lz4_cases.py), not the workload's."""
import ctypes
import random
import threading

import numpy as np
import pytest

from helpers import lz4_block
from helpers import lz4_cases as lc
from loongcollector_amd import binding, corpus, lz4_block as lz4, sls

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
ROW_SENTINEL = -0x5A5A5A5A5A5A5A5B


def _device():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host routine: [(chunk, data)] -> [block]"""
    exe = lc.build_host_check(tmp_path_factory.mktemp("lz4"))
    return lambda items: [b for _, b in lc.run_host_check(exe, items)[0]]


@pytest.fixture(scope="module")
def cases():
    return lc.cases()


class Batch:
    """segments on the device: segment s begins at a 16-byte boundary + residues[s], in the order `order`, `gap` foreign bytes between"""

    def __init__(self, segs, residues=None, order=None, gap=0):
        import torch
        dev = _device()
        self.segs, self.n = segs, len(segs)
        order = list(order) if order is not None else list(range(self.n))
        data, begin = bytearray(b"\x7e" * gap), [0] * self.n
        for s in order:
            if residues is not None:
                while len(data) % 16 != residues[s]:
                    data.append(0x7E)
            begin[s] = len(data)
            data += segs[s] + b"\x7e" * gap
        self.d_in = torch.from_numpy(np.frombuffer(bytes(data) or b"\0", np.uint8).copy()).to(dev)
        self.d_begin = torch.from_numpy(np.array(begin or [0], np.int64)).to(dev)
        self.d_len = torch.from_numpy(np.array([len(s) for s in segs] or [0], np.uint32).view(np.int32).copy()).to(dev)
        self.total_in = sum(len(s) for s in segs)

    def compress(self, ctx, d_out, out_cap, d_off, scratch=None):
        import torch
        if scratch is None:
            scratch = torch.empty(max(8, ctx.scratch_bytes(self.total_in, self.n)), dtype=torch.uint8, device=_device())
        ctx.compress_device(self.d_in, self.d_begin, self.d_len, self.n, d_out, out_cap, d_off, scratch, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()


def _off_rows(n):
    import torch
    return torch.full((n + 3,), ROW_SENTINEL, dtype=torch.int64, device=_device())


def _check_off_rows(rows, n, offsets):
    got = rows.cpu().numpy()
    assert got[0] == ROW_SENTINEL and got[n + 2] == ROW_SENTINEL, "a row beside d_out_off was written"
    assert np.array_equal(got[1:n + 2], offsets), "d_out_off"


def run(ctx, segs, want, **layout):
    """the segments through lc_lz4_compress_device -- without room (out_cap 0, d_out NULL: d_out_off must be complete), one byte short
    (d_out keeps its sentinel), and twice with exactly total bytes between two runs of 64 sentinel bytes -- against the host routine's
    blocks `want`, bit for bit"""
    import torch
    b = Batch(segs, **layout)
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in want], dtype=np.int64)]).astype(np.int64)
    total = int(offsets[-1])
    rows = _off_rows(b.n)
    b.compress(ctx, None, 0, rows[1:])
    _check_off_rows(rows, b.n, offsets)
    runs = []
    for cap in ([total - 1] if total else []) + [total, total]:
        buf = torch.full((64 + total + 64,), SENTINEL, dtype=torch.uint8, device=_device())
        rows = _off_rows(b.n)
        b.compress(ctx, buf[64:], cap, rows[1:])
        _check_off_rows(rows, b.n, offsets)
        got = buf.cpu().numpy()
        if cap < total:
            assert (got == SENTINEL).all(), "out_cap one byte short: a byte of d_out was stored"
            continue
        assert (got[:64] == SENTINEL).all() and (got[64 + total:] == SENTINEL).all(), "a byte outside d_out[0 .. total) was written"
        runs.append(got[64:64 + total].tobytes())
    assert runs[0] == runs[1], "two runs give different bytes"
    for s, w in enumerate(want):
        got = runs[0][offsets[s]:offsets[s + 1]]
        if got != w:
            at = next((i for i in range(min(len(got), len(w))) if got[i] != w[i]), min(len(got), len(w)))
            raise AssertionError("segment %d (%d bytes): block byte %d of %d differs: got %s, want %s" % (
                s, len(segs[s]), at, len(w), got[at:at + 8].hex(), w[at:at + 8].hex()))
    return runs[0], offsets


# ---------------------------------------------------------------------------------------------- 1. the constructed cases
@pytest.mark.parametrize("chunk", lc.CHUNKS)
def test_every_case_equals_the_host_routine_and_decodes(chunk, cases, host):
    """end rules, length bytes, windows (periods, one byte: 64 lanes on one slot) and chunk borders: every case of lz4_cases.py with this
    chunk size, each alone at its own residue and all of them as one batch"""
    mine = [c for c in cases if c["chunk"] == chunk]
    assert len(mine) >= 15
    want = host([(chunk, c["data"]) for c in mine])
    ctx = lz4.Lz4(chunk)
    for c, w in zip(mine, want):
        lc.check_block(w, c["data"], chunk, lz4_block.decode)
    for k, (c, w) in enumerate(zip(mine, want)):
        if len(c["data"]) <= 1200 or k % 5 == 0:
            run(ctx, [c["data"]], [w], residues=[k % 16], gap=3)
    run(ctx, [c["data"] for c in mine], want)


def test_the_end_rules_on_the_device(host):
    """no match in a segment below 13 bytes; a match that would run to the segment's end is cut at n - 5"""
    ctx = lz4.Lz4(65536)
    segs = [b"a" * n for n in lc.END_LENGTHS] + [b"ab" * 100, b"a" * 1000]
    data, off = run(ctx, segs, host([(65536, s) for s in segs]))
    for s, seg in enumerate(segs):
        _, seqs = lz4_block.decode(data[off[s]:off[s + 1]], len(seg))
        m = lz4_block.matches(seqs)
        # (one repeated byte meets itself in the second step at the earliest: position 64, which takes part from n = 76 on)
        assert (m == []) if len(seg) < 76 else (m[-1][0] + m[-1][1] == len(seg) - 5 and m[-1][0] <= len(seg) - 12)
    assert lz4_block.matches(lz4_block.decode(data[off[-2]:off[-1]], 1000)[1])[-1][:2] == (64, 1000 - 5 - 64)


# ---------------------------------------------------------------------------------------------- 2. segments
def _mixed_segments(n_seg, seed):
    rng = random.Random(seed)
    lengths = lc.END_LENGTHS + lc.LITERAL_RUNS + [255, 256, 300, 1000, 4095, 4097]
    segs = []
    for s in range(n_seg):
        n = 0 if s % 9 == 4 else rng.choice(lengths)
        segs.append(rng.choice([lc.text, lc.rnd, lambda n, seed: lc.periodic(1 + seed % 70, n, seed)])(n, 1000 * seed + s))
    return segs


@pytest.mark.parametrize("n_seg", [0, 1, 2, 63, 64, 65, 257])
def test_segment_counts_at_every_residue_in_permuted_order_with_gaps(n_seg, host):
    ctx = lz4.Lz4(4096)
    segs = _mixed_segments(n_seg, n_seg + 1)
    want = host([(4096, s) for s in segs]) if segs else []
    order = list(range(n_seg))
    random.Random(n_seg).shuffle(order)
    run(ctx, segs, want, residues=[(5 * s + 3) % 16 for s in range(n_seg)], order=order, gap=7)
    assert n_seg < 16 or {(5 * s + 3) % 16 for s in range(n_seg)} == set(range(16))


def test_one_segment_of_1_mib_among_short_ones(host):
    big = lc.text(300000, 1) + lc.rnd(200000, 2) + lc.periodic(300, (1 << 20) - 500000, 3)
    segs = [b"short one", big, b"", lc.text(700, 4)]
    for chunk in (4096, 65536):
        data, off = run(lz4.Lz4(chunk), segs, host([(chunk, s) for s in segs]), residues=[1, 2, 3, 4], order=[2, 1, 3, 0])
        lc.check_block(data[off[1]:off[2]], big, chunk, lz4_block.decode)


def test_the_default_chunk_and_the_bound():
    ctx = lz4.Lz4()
    assert ctx.chunk_bytes % 64 == 0 and 64 <= ctx.chunk_bytes <= 65536
    assert [lz4.bound(n) for n in (0, 1, 255, 1000)] == [16, 17, 272, 1019]
    for bad in (1, 32, 100, 65536 + 64):
        with pytest.raises(ValueError, match="rc=5"):
            lz4.Lz4(bad)


# ---------------------------------------------------------------------------------------------- 3. arguments
def test_refused_arguments():
    import torch
    ctx = lz4.Lz4(4096)
    b = Batch([b"hello hello hello hello"])
    out = torch.zeros(256, dtype=torch.uint8, device=_device())
    off = torch.zeros(8, dtype=torch.int64, device=_device())
    scratch = torch.zeros(ctx.scratch_bytes(b.total_in, 1) + 8, dtype=torch.uint8, device=_device())

    def rc(d_off=None, d_scratch=None, scratch_len=None, d_len=None):
        return ctx.compress_device_rc(b.d_in.data_ptr(), b.d_begin.data_ptr(), d_len or b.d_len.data_ptr(), 1, out.data_ptr(), 256,
                                      d_off or off.data_ptr(), d_scratch or scratch.data_ptr(), scratch.numel() - 8 if scratch_len is None else scratch_len)
    assert rc(d_off=off.data_ptr() + 4) == binding.LC_ERR_ARG          # d_out_off: 8 bytes
    assert rc(d_scratch=scratch.data_ptr() + 4) == binding.LC_ERR_ARG  # d_scratch: 8 bytes
    assert rc(d_len=b.d_len.data_ptr() + 2) == binding.LC_ERR_ARG
    assert rc(scratch_len=0) == binding.LC_ERR_ARG
    assert rc() == 0
    torch.cuda.synchronize()
    # a segment at or above the limit: the lengths live on the device, so the device refuses -- every offset is UINT64_MAX, no byte stored
    out.fill_(SENTINEL)
    big = torch.from_numpy(np.array([lz4.LC_LZ4_MAX_SEGMENT], np.uint32).view(np.int32).copy()).to(_device())
    assert rc(d_len=big.data_ptr()) == 0
    torch.cuda.synchronize()
    assert list(off.cpu().numpy()[:2]) == [-1, -1] and (out.cpu().numpy() == SENTINEL).all()
    # ... and a scratch that holds the segment table but not the lengths' sum
    long_one = Batch([lc.text(100000, 1)])
    off.fill_(0)
    assert ctx.compress_device_rc(long_one.d_in.data_ptr(), long_one.d_begin.data_ptr(), long_one.d_len.data_ptr(), 1, out.data_ptr(), 256,
                                  off.data_ptr(), scratch.data_ptr(), ctx.scratch_bytes(0, 1)) == 0
    torch.cuda.synchronize()
    assert list(off.cpu().numpy()[:2]) == [-1, -1] and (out.cpu().numpy() == SENTINEL).all()
    # lc_lz4_compress_host knows the lengths: LC_ERR_ARG before anything is queued
    seg_len =np.array([lz4.LC_LZ4_MAX_SEGMENT], np.uint32)
    ptrs = np.array([out.data_ptr()], np.uint64)
    view, o = ctypes.c_void_p(), np.zeros(2, np.uint64)
    assert ctx._L.lc_lz4_compress_host(ctx.handle, ptrs.ctypes.data, seg_len.ctypes.data, 1, ctypes.byref(view), o.ctypes.data) == binding.LC_ERR_ARG


def test_a_tensor_on_another_device_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    ctx = lz4.Lz4(4096)
    other = torch.device("cuda:1")
    d_in = torch.zeros(64, dtype=torch.uint8, device=other)
    d_begin = torch.zeros(1, dtype=torch.int64, device=other)
    d_len = torch.full((1,), 64, dtype=torch.int32, device=other)
    out = torch.zeros(256, dtype=torch.uint8, device=other)
    off = torch.zeros(2, dtype=torch.int64, device=other)
    scratch = torch.zeros(ctx.scratch_bytes(64, 1), dtype=torch.uint8, device=other)
    torch.cuda.set_device(0)
    assert ctx.compress_device_rc(d_in.data_ptr(), d_begin.data_ptr(), d_len.data_ptr(), 1, out.data_ptr(), 256, off.data_ptr(), scratch.data_ptr(),
                                  scratch.numel()) == binding.LC_ERR_ARG


# ---------------------------------------------------------------------------------------------- 4. the host entries
def test_compress_host_from_eight_threads_each_holding_its_view_until_its_next_call(host):
    ctx = lz4.Lz4(4096)
    jobs = {(t, k): [lc.text(1 + 977 * t + 131 * k, 10 * t + k), b"", lc.rnd(40 + t, t), lc.periodic(3 + k, 5000, k)] for t in range(8) for k in range(4)}
    flat = [(key, s) for key, segs in jobs.items() for s in segs]
    blocks = host([(4096, s) for _, s in flat])
    want = {key: [b for (k2, _), b in zip(flat, blocks) if k2 == key] for key in jobs}
    errors = []

    def runner(t):
        try:
            held = None
            for k in range(4):
                if held is not None:          # the view of this thread's call before, while the other threads made theirs
                    assert ctypes.string_at(held[0], len(held[1])) == held[1]
                at, off = ctx.compress_host_view(jobs[(t, k)])
                joined = b"".join(want[(t, k)])
                assert int(off[-1]) == len(joined) and ctypes.string_at(at, len(joined)) == joined
                held = (at, joined)
            lz4.thread_release()
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=runner, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
    assert ctx.compress_host([]) == []


TAGS = [(b"__topic__", b"topic-1"), (b"__source__", b"10.1.2.3"), (b"__machine_uuid__", b"uuid"), (b"host", b"h" * 40), (b"__tag__:__path__", b"/var/log/app.log")]


@pytest.mark.parametrize("enable_ns", [0, 1])
def test_match_encode_compress_on_600_headline_lines(enable_ns):
    """the block decodes to exactly lc_sls_match_encode_host's bytes followed by the tag bytes; raw_len, status and rec_off are that entry's"""
    n = 600
    data, off, length = corpus.apache_batch(n, "A", poison_every=17)
    lines = [data[off[i]:off[i] + length[i]].tobytes() for i in range(n)]
    rx = binding.GpuRegex(corpus.REGEX_A)
    G = rx.groups
    keys = [b"g%d" % g for g in range(1, G + 1)] + [b"__raw__"]
    plan = sls.Plan(keys, [(g - 1, g) for g in range(1, G + 1)], [(G, 0)])
    times, ns = [1700000000 + i for i in range(n)], [i if i % 2 else -1 for i in range(n)]
    tags = sls.append_tags(TAGS)
    records, rec_off, status = sls.match_encode_host(plan, rx, lines, times, ns, enable_ns)
    ctx = lz4.Lz4()
    binding.launched_kernels()
    block, raw_len, rec_off2, status2 = ctx.match_encode_compress_host(plan, rx, lines, times, ns, enable_ns, tags)
    kernels = binding.launched_kernels()
    for name in ("lz4_plan_kernel", "lz4_match_kernel", "lz4_scan_kernel", "lz4_size_kernel", "lz4_emit_kernel", "lz4_tags_kernel", "sls_write_kernel"):
        assert name in kernels, "the kernel %s was not launched" % name
    assert raw_len == len(records) + len(tags)
    got, _ = lz4_block.decode(block, raw_len)
    assert got == records + tags
    assert np.array_equal(status2, status) and np.array_equal(rec_off2, rec_off)
    assert len(block) < raw_len
    L = lc.system_lz4()
    if L is not None:
        assert lc.system_decode(L, block, raw_len) == records + tags
    # no tags, no offsets asked for; no lines at all
    block, raw_len, none, _ = ctx.match_encode_compress_host(plan, rx, lines, times, ns, enable_ns, b"", want_rec_off=False)
    assert none is None and lz4_block.decode(block, raw_len)[0] == records
    block, raw_len, rec, _ = ctx.match_encode_compress_host(plan, rx, [], [], None, 0, tags)
    assert raw_len == len(tags) and list(rec) == [0] and lz4_block.decode(block, raw_len)[0] == tags


def test_match_encode_compress_with_rows_that_outgrow_the_first_buffer():
    """a plan that writes the line beside nested groups: the records exceed the bound the first attempt takes, the second makes them all"""
    rx = binding.GpuRegex(rb"((\w+) (\w+)) (.*)")
    plan = sls.Plan([b"both", b"first", b"second", b"rest", b"line"], [(0, 1)] * 6 + [(1, 2), (2, 3), (3, 4), (4, 0), (4, 0)], [(4, 0)])
    lines = [b"a" * 20 + b" " + b"b" * 21 + b" " + b"r" * (i % 90) if i % 7 else b"-" for i in range(500)]
    times = [1700000000 + i for i in range(500)]
    ns = [i if i % 3 else -1 for i in range(500)]
    tags = sls.append_tags(TAGS)
    records, rec_off, status = sls.match_encode_host(plan, rx, lines, times, ns, 1)
    assert len(records) > 3 * sum(len(v) for v in lines)          # (what makes it outgrow the bound)
    block, raw_len, rec_off2, status2 = lz4.Lz4().match_encode_compress_host(plan, rx, lines, times, ns, 1, tags)
    assert raw_len == len(records) + len(tags) and lz4_block.decode(block, raw_len)[0] == records + tags
    assert np.array_equal(status2, status) and np.array_equal(rec_off2, rec_off)
