"""The small kernels every batch passes through -- line split (split_kernel.hpp), length scheduler (sched_kernel.hpp), span filter
and pinned upload (pipeline_kernel.hpp) -- at the edges of their own geometry: behind the split scan's first carry (16 MiB), at
piece / sub-tile / tile boundaries, from unaligned base pointers, with truncated tables, above 2^31 bytes, in the grid-stride
loops of the capped grids, and with every capacity guard exercised.

Everything is bit-exact against the plain models of tests/helpers/edge_models.py.  Every output tensor is larger than what the
library is told about and pre-filled with a sentinel that must survive behind the handed-over extent."""
import numpy as np
import pytest

from helpers.edge_models import sched_bucket, span_filter_model, split_table_from_hits, split_table_np
from helpers.pipeline_corpus import access_log_buffer
from loongcollector_amd import binding as B
from loongcollector_amd import corpus
from oracle.oracle import OracleRegex

pytestmark = pytest.mark.gpu

MIB = 1 << 20
TILE = 16384                       # split_kernel.hpp kSplitBytesPerBlock
OFF_SENTINEL = -559038737          # 0xDEADBEEF as int32; no table entry of these tests has that value
GUARD = 64                         # bytes / entries kept behind every extent handed to the library


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert B.device_count() >= 1
    torch.cuda.set_device(0)
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------ split
def _upload_padded(torch, arr, split_char, lead=0):
    """arr on the device, behind `lead` bytes and in front of GUARD bytes that all hold the split char (a read outside
    [0, nbytes) then shows as extra lines); -> the view that starts at arr[0]"""
    host = np.full(lead + len(arr) + GUARD, split_char, dtype=np.uint8)
    host[lead:lead + len(arr)] = arr
    return torch.from_numpy(host).to("cuda:0")[lead:]


def _run_split(torch, d_data, nbytes, split_char, table_entries, off_capacity=None, scratch_words=None, check=True):
    """-> (status code, *d_nlines, the WHOLE allocated table as uint32: table_entries handed over + GUARD sentinels)"""
    d_off = torch.full((table_entries + GUARD,), OFF_SENTINEL, dtype=torch.int32, device="cuda:0")
    d_n = torch.full((1 + GUARD,), -1, dtype=torch.int32, device="cuda:0")
    words = B.split_scratch_bytes(nbytes) // 4 + 1 if scratch_words is None else scratch_words
    d_scratch = torch.empty((words,), dtype=torch.int32, device="cuda:0")
    rc = B.split_lines_device(d_data, nbytes, d_off[:table_entries], d_n, d_scratch, split_char=split_char, stream=_stream(torch),
                              off_capacity=off_capacity, check=check)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()
    assert (n[1:] == -1).all()
    return rc, int(n.view(np.uint32)[0]), d_off.cpu().numpy().view(np.uint32)


def _assert_whole_table(torch, d_data, nbytes, split_char, exp, what):
    rc, n, got = _run_split(torch, d_data, nbytes, split_char, len(exp) + 8)
    assert rc == B.LC_OK
    assert n == len(exp) - 1, (what, n, len(exp) - 1)
    bad = np.flatnonzero(got[:len(exp)] != exp)
    assert bad.size == 0, (what, "first wrong entry", int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
    assert (got[len(exp):] == np.uint32(OFF_SENTINEL & 0xFFFFFFFF)).all(), what


@pytest.fixture(scope="module")
def slab_corpus():
    """mixed nginx / JSON lines of 128-2048 bytes, as bench.py builds its 64 MiB slabs"""
    data, off, length = corpus.mixed_batch(int((64 * MIB) / 600))
    assert len(data) >= 64 * MIB + 4096
    return data


@pytest.mark.parametrize("nbytes,start", [(16 * MIB - 1, 0), (16 * MIB, 1), (16 * MIB + 1, 777), (16 * MIB + TILE + 1, 1234),
                                           (32 * MIB + 5, 4001), (64 * MIB, 0)])
def test_split_table_is_whole_behind_the_scan_carry(torch_dev, slab_corpus, nbytes, start):
    """one scan round covers 1024 tiles = 16 MiB: 1, 2, 3 and 4 rounds, and the whole table is compared"""
    arr = slab_corpus[start:start + nbytes]
    exp = split_table_np(arr, 10)
    assert len(exp) > nbytes // 2100
    _assert_whole_table(torch_dev, _upload_padded(torch_dev, arr, 10), nbytes, 10, exp, nbytes)


def test_split_dense_buffer_carries_sixteen_million_hits(torch_dev):
    nbytes = 16 * MIB + 3
    d_data = torch_dev.full((nbytes + GUARD,), 10, dtype=torch_dev.uint8, device="cuda:0")
    exp = np.arange(nbytes + 1, dtype=np.uint32)          # every byte closes a line: off[i] = i
    _assert_whole_table(torch_dev, d_data, nbytes, 10, exp, "dense")
    del d_data
    torch_dev.cuda.empty_cache()


def test_split_sparse_buffer_with_hits_only_around_the_round_boundaries(torch_dev):
    nbytes = 40 * MIB
    last = nbytes // TILE - 1
    hits = []
    for tile in (1023, 1024, 2047, 2048, last):
        hits += [tile * TILE + p for p in (0, 1, 15, 16, 4095, 4096, 9000, TILE - 2, TILE - 1)]
    hits = sorted(h for h in hits if h < nbytes - 1)      # (the buffer stays unterminated)
    arr = np.full(nbytes, 0x61, dtype=np.uint8)
    arr[hits] = 10
    exp = split_table_from_hits(hits, nbytes, terminated=False)
    assert np.array_equal(exp, split_table_np(arr, 10))
    _assert_whole_table(torch_dev, _upload_padded(torch_dev, arr, 10), nbytes, 10, exp, "sparse")


@pytest.mark.parametrize("nbytes", [4095, 4097, 16383, 16384, 16385, 5 * TILE + 1])
@pytest.mark.parametrize("split_char", [10, 0])
def test_split_separators_on_piece_subtile_and_tile_boundaries(torch_dev, nbytes, split_char):
    pos = {0, nbytes - 1}
    for k in (1, 2, 3, 255, 256, 257, 1023, 1024, 1025):
        pos |= {k * 16 - 1, k * 16}
    for k in range(1, 21):
        pos |= {k * 4096 - 1, k * 4096}
    for k in range(1, 6):
        pos |= {k * TILE - 1, k * TILE}
    pos = sorted(p for p in pos if 0 <= p < nbytes)
    for terminated in (True, False):
        hits = [p for p in pos if terminated or p != nbytes - 1]
        arr = np.full(nbytes, 0x41, dtype=np.uint8)
        arr[hits] = split_char
        exp = split_table_from_hits(hits, nbytes, terminated)
        assert np.array_equal(exp, split_table_np(arr, split_char))
        _assert_whole_table(torch_dev, _upload_padded(torch_dev, arr, split_char), nbytes, split_char, exp, (nbytes, terminated))


@pytest.mark.parametrize("lead", [1, 5, 15])
@pytest.mark.parametrize("split_char", [10, 0, 0x80, 0xFF])
def test_split_from_an_unaligned_base_pointer(torch_dev, lead, split_char):
    """d_data[k:] takes the byte-load path of splitLaneMask; the bytes behind nbytes hold the split char"""
    rng = np.random.default_rng(100 * lead + split_char)
    alphabet = np.array([split_char, 0x00, 0x0A, 0x61, 0x7F, 0x80, 0xFF, 0x20, 0x62, 0x63], dtype=np.uint8)
    for nbytes in (1, 15, 17, 16385, 70001):
        for ends_with_hit in (False, True):
            arr = rng.choice(alphabet, size=nbytes)
            arr[-1] = split_char if ends_with_hit else (0x61 if split_char != 0x61 else 0x62)
            d_data = _upload_padded(torch_dev, arr, split_char, lead=lead)
            assert d_data.data_ptr() % 16 == lead
            _assert_whole_table(torch_dev, d_data, nbytes, split_char, split_table_np(arr, split_char), (lead, split_char, nbytes))


@pytest.mark.parametrize("terminated", [True, False])
def test_split_truncates_at_off_capacity(torch_dev, terminated):
    rng = np.random.default_rng(31)
    arr = rng.choice(np.frombuffer(b"abcdefghij\n", dtype=np.uint8), size=50000)
    arr[-1] = 10 if terminated else 0x61
    exp = split_table_np(arr, 10)
    L = len(exp) - 1
    assert L > 3000
    d_data = _upload_padded(torch_dev, arr, 10)
    sentinel = np.uint32(OFF_SENTINEL & 0xFFFFFFFF)
    for capacity in (2, L, L + 1):
        rc, n, got = _run_split(torch_dev, d_data, len(arr), 10, L + 9, off_capacity=capacity)
        assert rc == B.LC_OK and n == L, (capacity, n, L)      # *d_nlines >= off_capacity says "truncated"
        assert np.array_equal(got[:capacity], exp[:capacity]), capacity
        assert (got[capacity:] == sentinel).all(), capacity   # nothing behind the table, whatever the allocation holds


def test_split_offsets_above_two_to_the_31(torch_dev):
    """2 GiB + 1 MiB + 7 bytes built on the device; the expected table follows from where the separators were put"""
    torch = torch_dev
    nbytes = (1 << 31) + MIB + 7
    rng = np.random.default_rng(2031)
    pos = {0, 15, 16, TILE - 1, TILE, (1 << 31) - TILE - 1, (1 << 31) - 17, (1 << 31) - 2, (1 << 31) - 1, 1 << 31, (1 << 31) + 1,
           (1 << 31) + 15, (1 << 31) + 16, (1 << 31) + TILE - 1, (1 << 31) + TILE, nbytes - 9, nbytes - 2}
    pos |= {int(p) for p in rng.integers(0, nbytes - 1, size=260)}
    pos |= {int(p) for p in rng.integers((1 << 31) - 4 * TILE, (1 << 31) + 4 * TILE, size=60)}
    pos |= {int(p) for p in rng.integers(1 << 31, nbytes - 1, size=150)}
    pos = sorted(pos)                                      # byte nbytes - 1 is no separator: an unterminated tail
    assert pos[-1] == nbytes - 2 and len(pos) > 300
    d_data = torch.full((nbytes + GUARD,), 0x61, dtype=torch.uint8, device="cuda:0")
    d_data[nbytes:].fill_(10)
    for p in pos:
        d_data[p:p + 1].fill_(10)
    exp = split_table_from_hits(pos, nbytes, terminated=False)
    assert exp.dtype == np.uint32 and int(exp[-1]) == nbytes + 1 and (exp > np.uint32(1 << 31)).sum() > 100
    try:
        _assert_whole_table(torch, d_data, nbytes, 10, exp, "above 2^31")
    finally:
        del d_data
        torch.cuda.empty_cache()
    assert torch.cuda.memory_allocated() < 256 * MIB


def test_split_argument_errors_and_the_empty_buffer(torch_dev):
    torch = torch_dev
    arr = np.frombuffer(b"one\ntwo\nthree", dtype=np.uint8)
    d_data = _upload_padded(torch, arr, 10)
    sentinel = np.uint32(OFF_SENTINEL & 0xFFFFFFFF)
    for capacity in (0, 1):
        rc, n, got = _run_split(torch, d_data, len(arr), 10, 8, off_capacity=capacity, check=False)
        assert rc == B.LC_ERR_ARG and n == 0xFFFFFFFF and (got == sentinel).all()
    big = np.full(100000, 0x61, dtype=np.uint8)
    rc, n, got = _run_split(torch, _upload_padded(torch, big, 10), len(big), 10, 8, scratch_words=B.split_scratch_bytes(len(big)) // 4 - 1,
                            check=False)
    assert rc == B.LC_ERR_ARG and n == 0xFFFFFFFF and (got == sentinel).all()
    # 2^32 - 1 bytes cannot be described by a 32-bit table: refused before any launch (the tensor has 16 bytes)
    d_small = torch.full((16,), 10, dtype=torch.uint8, device="cuda:0")
    rc, n, got = _run_split(torch, d_small, (1 << 32) - 1, 10, 8, scratch_words=B.split_scratch_bytes((1 << 32) - 1) // 4 + 1, check=False)
    assert rc == B.LC_ERR_ARG and n == 0xFFFFFFFF and (got == sentinel).all()
    with pytest.raises(RuntimeError):
        B.split_lines_device(d_small, (1 << 32) - 1, torch.zeros(8, dtype=torch.int32, device="cuda:0"),
                             torch.zeros(1, dtype=torch.int32, device="cuda:0"), torch.zeros(8, dtype=torch.int32, device="cuda:0"))
    rc, n, got = _run_split(torch, d_data, 0, 10, 8)
    assert rc == B.LC_OK and n == 0 and (got == sentinel).all()      # an empty buffer has no lines


# -------------------------------------------------------------------------------------------------------- length scheduler
def _run_ragged(torch, rx, data, off, length, n, sep_bytes, n_dyn=None):
    """lc_regex_match_device_ragged, engine TDFA.  off: n (+1) entries; length None: sizes from the table.
    -> (caps, status, order) with every array GUARD lines longer than n"""
    G = rx.groups
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(GUARD, np.uint8)])).to("cuda:0")
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")
    d_len = None if length is None else torch.from_numpy(np.ascontiguousarray(length, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")
    d_caps = torch.full((n + GUARD, 2 * G), -7, dtype=torch.int32, device="cuda:0")
    d_status = torch.full((n + GUARD,), 9, dtype=torch.uint8, device="cuda:0")
    words = B.sched_scratch_bytes(n) // 4
    assert words == n + 512
    d_scratch = torch.full((words + GUARD,), -1, dtype=torch.int32, device="cuda:0")
    d_nlines = None if n_dyn is None else torch.tensor([n_dyn], dtype=torch.int32, device="cuda:0")
    rx.match_device_ragged(d_data, d_off, d_len, n, d_caps, d_status, d_scratch[:words], sep_bytes=sep_bytes, d_nlines=d_nlines,
                           stream=_stream(torch), engine=B.LC_ENGINE_TDFA)
    torch.cuda.synchronize()
    return d_caps.cpu().numpy(), d_status.cpu().numpy(), d_scratch.cpu().numpy().view(np.uint32)[512:]


def _assert_ragged(got, exp_caps, exp_status, length, n, n_dyn=None):
    caps, status, order = got
    live = n if n_dyn is None else min(n, n_dyn)
    assert np.array_equal(status[:live], exp_status[:live])               # at the ORIGINAL indices
    assert np.array_equal(caps[:live], exp_caps[:live])
    assert (status[live:] == 9).all() and (caps[live:] == -7).all()       # lines at or beyond *d_nlines are not touched
    assert np.array_equal(np.sort(order[:live]), np.arange(live, dtype=np.uint32))          # a permutation
    assert (order[live:] == 0xFFFFFFFF).all()
    buckets = sched_bucket(np.asarray(length[:live])[order[:live].astype(np.int64)])
    assert (np.diff(buckets) >= 0).all()                                  # longest length class first


@pytest.fixture(scope="module")
def big_ragged_batch():
    n = 600_001                         # above 2048 workgroups x 256 lines: both kernels loop
    data, off, length = corpus.mixed_batch(n, min_len=1, max_len=300)
    zeroed = length.copy()
    zeroed[::97] = 0                    # empty lines in the mix (views of zero length)
    oracle = OracleRegex(corpus.REGEX_B)
    return {"n": n, "data": data, "off": off, "length": length, "zeroed": zeroed,
            "exp_zeroed": oracle.fullmatch_batch(data, off[:-1], zeroed), "exp_table": oracle.fullmatch_batch(data, off[:-1], length)}


@pytest.mark.parametrize("n_dyn", [None, 524_289, 0])
def test_scheduler_grid_stride_loop_and_runtime_line_count(torch_dev, big_ragged_batch, n_dyn):
    b = big_ragged_batch
    rx = B.GpuRegex(corpus.REGEX_B)
    got = _run_ragged(torch_dev, rx, b["data"], b["off"][:-1], b["zeroed"], b["n"], 0, n_dyn=n_dyn)
    _assert_ragged(got, b["exp_zeroed"][0], b["exp_zeroed"][1], b["zeroed"], b["n"], n_dyn=n_dyn)
    if n_dyn != 0:
        assert 0 < int((got[1][:b["n"]] == B.LC_MATCH).sum()) < (n_dyn or b["n"])


@pytest.mark.parametrize("n_dyn", [None, 524_289])
def test_scheduler_takes_sizes_from_a_split_table(torch_dev, big_ragged_batch, n_dyn):
    """d_len = NULL, sep_bytes = 1 on an off[n+1] table"""
    b = big_ragged_batch
    rx = B.GpuRegex(corpus.REGEX_B)
    got = _run_ragged(torch_dev, rx, b["data"], b["off"], None, b["n"], 1, n_dyn=n_dyn)
    _assert_ragged(got, b["exp_table"][0], b["exp_table"][1], b["length"], b["n"], n_dyn=n_dyn)


def test_scheduler_clamped_bucket_of_very_long_lines(torch_dev):
    rng = np.random.Generator(np.random.MT19937(77))
    long_ones = [8159, 8160, 8191, 8192, 70000, 8160, 8159, 70000]
    chunks = []
    for i in range(3000):
        if i % 373 == 5:
            chunks.append(corpus._one_line(rng, "B", long_ones[(i // 373) % len(long_ones)]))
        elif i % 5 == 0:
            chunks.append(b'{"msg":"' + bytes(rng.integers(97, 123, size=int(rng.integers(1, 400)), dtype=np.uint8)) + b'"}')
        else:
            chunks.append(corpus._one_line(rng, "B", int(rng.integers(160, 700))))
    length = np.array([len(c) for c in chunks], dtype=np.uint32)
    assert set(long_ones) <= set(length.tolist())
    off = np.zeros(len(chunks) + 1, dtype=np.uint32)
    off[1:] = np.cumsum(length + 1)
    data = np.frombuffer(b"\n".join(chunks) + b"\n", dtype=np.uint8)
    exp_caps, exp_status = OracleRegex(corpus.REGEX_B).fullmatch_batch(data, off[:-1], length)
    assert (exp_status[length >= 8159] == B.LC_MATCH).all()
    rx = B.GpuRegex(corpus.REGEX_B)
    for form in ("len", "table"):
        got = _run_ragged(torch_dev, rx, data, off[:-1] if form == "len" else off, length if form == "len" else None, len(chunks),
                          0 if form == "len" else 1)
        _assert_ragged(got, exp_caps, exp_status, length, len(chunks))
        clamped = sorted(l for l in length.tolist() if l >= 8160)                           # bucket 0 = everything from 8160 up
        assert len(clamped) == 6 and sorted(length[got[2][:6].astype(np.int64)].tolist()) == clamped


def test_scheduler_constant_length_batch_lands_in_one_bucket(torch_dev):
    n = 70_003
    data, off, length = corpus.apache_batch(n, "B", line_bytes=200, poison_every=19)
    exp_caps, exp_status = OracleRegex(corpus.REGEX_B).fullmatch_batch(data, off[:-1], length)
    rx = B.GpuRegex(corpus.REGEX_B)
    got = _run_ragged(torch_dev, rx, data, off, None, n, 1)
    _assert_ragged(got, exp_caps, exp_status, length, n)
    assert len(set(sched_bucket(length).tolist())) == 1


# ------------------------------------------------------------------------------------------------------------- span filter
PACK_SENTINEL = -77
KEY_GROUP = {k: i + 1 for i, k in enumerate(corpus.KEYS_B)}
RULES_USER_AGENT = [("^no-agent$", KEY_GROUP["user_agent"])]                                       # tests/test_gpu_pipeline.py FILTERS[0]
RULES_METHOD_CODE = [("GET|POST", KEY_GROUP["method"]), (r"2\d\d", KEY_GROUP["response_code"])]    # FILTERS[1]
RULES_REFERRER = [(".*", KEY_GROUP["referrer"])]                                                   # FILTERS[2]
RULES_EIGHT = RULES_METHOD_CODE + RULES_REFERRER + [(r"[\d.]+", KEY_GROUP["ip"]), ("-", KEY_GROUP["ident"]),
                                                    (r".* \+0000", KEY_GROUP["timestamp"]), (r"HTTP/1\.[01]", KEY_GROUP["http_version"]),
                                                    (r"\d+", KEY_GROUP["bytes"])]
RULE_SETS = {"none": [], "user_agent": RULES_USER_AGENT, "method_code": RULES_METHOD_CODE, "referrer": RULES_REFERRER, "eight": RULES_EIGHT}


class _Parsed:
    """a read buffer split (model) and parsed on the device; the parse result is first held to the oracle"""

    def __init__(self, torch, buf, pattern, extra_lines=0):
        self.torch = torch
        arr = np.frombuffer(buf, dtype=np.uint8)
        self.off = split_table_np(arr, 10)
        self.n = len(self.off) - 1
        self.max_lines = self.n + extra_lines
        self.lines = [(int(self.off[i]), buf[int(self.off[i]):int(self.off[i + 1]) - 1]) for i in range(self.n)]
        self.rx = B.GpuRegex(pattern)
        self.G = self.rx.groups
        self.exp_caps, self.exp_status = OracleRegex(pattern).fullmatch_batch(
            arr, self.off[:-1], np.array([len(l) for _, l in self.lines], dtype=np.uint32))
        self.d_data = _upload_padded(torch, arr, 10)
        d_off = np.zeros(self.max_lines + 1 + GUARD, dtype=np.uint32)
        d_off[:self.n + 1] = self.off
        self.d_off = torch.from_numpy(d_off.view(np.int32)).to("cuda:0")
        self.d_n = torch.tensor([self.n], dtype=torch.int32, device="cuda:0")
        self.d_caps = torch.full((self.max_lines + GUARD, 2 * self.G), -7, dtype=torch.int32, device="cuda:0")
        self.d_status = torch.full((self.max_lines + GUARD,), 9, dtype=torch.uint8, device="cuda:0")
        self.rx.match_device_dyn(self.d_data, self.d_off, self.d_n, self.max_lines, self.d_caps, self.d_status, stream=_stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(self.d_status.cpu().numpy()[:self.n], self.exp_status)
        assert np.array_equal(self.d_caps.cpu().numpy()[:self.n], self.exp_caps)
        assert (self.d_status.cpu().numpy()[self.n:] == 9).all()
        self.status = self.exp_status.copy()
        self._rules = {}

    def compiled(self, rules):
        out = []
        for pattern, group in rules:
            if pattern not in self._rules:
                self._rules[pattern] = B.GpuRegex(pattern)
                assert self._rules[pattern].prepare_span_filter() == B.LC_OK
            out.append((self._rules[pattern], group))
        return out

    def check(self, rules, cap_rows=None, cap_delta=None, n_dyn=None, null_table=False):
        """one lc_span_filter_device call against the model; cap_rows / cap_delta (relative to the survivors) pick packed_cap_rows"""
        torch = self.torch
        live = self.n if n_dyn is None else n_dyn
        counts, rows = span_filter_model(self.lines[:live], self.status[:live], self.exp_caps[:live], rules)
        cap = cap_rows if cap_rows is not None else max(0, counts[1] + (8 if cap_delta is None else cap_delta))
        width = 3 + 2 * self.G
        d_packed = torch.full((cap + GUARD, width), PACK_SENTINEL, dtype=torch.int32, device="cuda:0")
        d_counts = torch.full((4 + GUARD,), -5, dtype=torch.int32, device="cuda:0")
        d_n = self.d_n if n_dyn is None else torch.tensor([n_dyn], dtype=torch.int32, device="cuda:0")
        rc = B.span_filter_device(self.compiled(rules), self.d_data, self.d_off, 1, d_n, self.max_lines, self.G, self.d_caps, self.d_status,
                                  None if null_table else d_packed[:cap], cap, d_counts, stream=_stream(torch))
        torch.cuda.synchronize()
        assert rc == B.LC_OK
        got_counts = d_counts.cpu().numpy()
        what = (rules, cap, live)
        assert got_counts[:4].tolist() == counts, what
        assert (got_counts[4:] == -5).all()
        packed = d_packed.cpu().numpy()
        written = min(counts[1], cap)
        assert (packed[written:] == PACK_SENTINEL).all(), what             # nothing behind the rows that fit
        seen = packed[:written, 0].tolist()
        assert len(set(seen)) == written, what                             # distinct lines ...
        for r in range(written):
            assert seen[r] in rows and packed[r].tolist() == rows[seen[r]], (what, r)   # ... each a true survivor with its own row
        return counts


@pytest.mark.parametrize("n_lines", [1, 63, 64, 65, 257, 50_000])
def test_span_filter_rule_counts_and_line_counts(torch_dev, n_lines):
    buf, _ = access_log_buffer(n_lines, seed=5)
    p = _Parsed(torch_dev, buf, corpus.REGEX_B, extra_lines=37)            # *d_nlines < max_lines throughout
    assert p.n == n_lines
    matched = int((p.exp_status == B.LC_MATCH).sum())
    for name, rules in RULE_SETS.items():
        counts = p.check(rules)
        if name in ("none", "referrer"):
            assert counts[1] == matched                                    # zero rules: every matched line survives
        assert counts[0] == n_lines and counts[2] == n_lines - matched and counts[3] == 0
        if n_lines >= 257:
            assert 0 < counts[1] <= matched and counts[2] > 0, name


@pytest.mark.parametrize("n_lines", [257, 50_000])
def test_span_filter_packed_capacity_and_runtime_line_count(torch_dev, n_lines):
    buf, _ = access_log_buffer(n_lines, seed=6, trailing_newline=False)
    p = _Parsed(torch_dev, buf, corpus.REGEX_B)
    for rules in (RULES_USER_AGENT, RULES_METHOD_CODE, []):
        survivors = p.check(rules, cap_delta=8)[1]
        assert survivors > 8
        p.check(rules, cap_delta=0)
        p.check(rules, cap_delta=-1)
        p.check(rules, cap_rows=1)
        p.check(rules, cap_rows=0)
        p.check(rules, cap_rows=0, null_table=True)
        for n_dyn in (0, 1, n_lines // 2, n_lines - 1):
            p.check(rules, n_dyn=n_dyn)
            p.check(rules, n_dyn=n_dyn, cap_rows=3)


def test_span_filter_counts_undecided_lines(torch_dev):
    """LC_OVERFLOW / LC_GAVE_UP status bytes, put there after the match, go to counts[3] and never survive"""
    torch = torch_dev
    buf, _ = access_log_buffer(50_000, seed=8)
    p = _Parsed(torch, buf, corpus.REGEX_B)
    rng = np.random.default_rng(8)
    idx = rng.choice(p.n, size=400, replace=False)
    p.status[idx[:230]] = B.LC_OVERFLOW
    p.status[idx[230:]] = B.LC_GAVE_UP
    p.d_status[:p.n].copy_(torch.from_numpy(p.status).to("cuda:0"))
    torch.cuda.synchronize()
    for rules in ([], RULES_USER_AGENT, RULES_EIGHT):
        counts = p.check(rules)
        assert counts[3] == 400
        p.check(rules, cap_delta=-1)
        p.check(rules, n_dyn=p.n // 3)


@pytest.mark.parametrize("n_copies", [1, 21, 5000])
def test_span_filter_gives_a_group_that_did_not_take_part_the_empty_value(torch_dev, n_copies):
    texts = [b"alpha 12 rest of line", b"beta rest without number", b"nospace", b"gamma 7 x", b"delta  y", b"", b"eps 0 ", b"zeta tail"]
    buf = b"\n".join(texts[i % len(texts)] + (b" %d" % i if i % len(texts) in (0, 1) else b"") for i in range(n_copies * len(texts))) + b"\n"
    p = _Parsed(torch_dev, buf, r"(\S+)(?: (\d+))? (.*)")
    absent = int(((p.exp_status == B.LC_MATCH) & (p.exp_caps[:, 2] < 0)).sum())
    present = int(((p.exp_status == B.LC_MATCH) & (p.exp_caps[:, 2] >= 0)).sum())
    assert absent >= 3 * n_copies and present >= 3 * n_copies
    assert p.check([(r"\d*", 2)])[1] == absent + present          # the empty value matches \d*: absent groups are kept
    assert p.check([(r"\d+", 2)])[1] == present                   # ... and dropped by \d+
    assert p.check([(r"\d*", 2), (r"\S+", 1), (r".*", 3)], cap_delta=-1)[1] == absent + present
    assert p.check([(r"", 2)])[1] == absent


def test_span_filter_argument_errors(torch_dev):
    torch = torch_dev
    buf, _ = access_log_buffer(257, seed=5)
    p = _Parsed(torch, buf, corpus.REGEX_B)
    d_packed = torch.full((p.n + GUARD, 3 + 2 * p.G), PACK_SENTINEL, dtype=torch.int32, device="cuda:0")
    d_counts = torch.full((4 + GUARD,), -5, dtype=torch.int32, device="cuda:0")

    def call(rules):
        rc = B.span_filter_device(rules, p.d_data, p.d_off, 1, p.d_n, p.max_lines, p.G, p.d_caps, p.d_status, d_packed[:p.n], p.n, d_counts,
                                  stream=_stream(torch), check=False)
        torch.cuda.synchronize()
        return rc

    rule = p.compiled([(".*", 1)])[0][0]
    assert call([(rule, 1)] * 9) == B.LC_ERR_ARG                           # at most eight rules
    assert call([(rule, 0)]) == B.LC_ERR_ARG                               # groups are 1-based
    assert call([(rule, p.G + 1)]) == B.LC_ERR_ARG
    assert call([(rule, 1), (rule, p.G + 1)]) == B.LC_ERR_ARG
    fresh = B.GpuRegex("GET")
    assert call([(fresh, 5)]) == B.LC_ERR_UNSUPPORTED                      # no prepare_span_filter
    assert (d_packed.cpu().numpy() == PACK_SENTINEL).all() and (d_counts.cpu().numpy() == -5).all()   # nothing was launched
    with pytest.raises(RuntimeError):
        B.span_filter_device([(fresh, 5)], p.d_data, p.d_off, 1, p.d_n, p.max_lines, p.G, p.d_caps, p.d_status, d_packed[:p.n], p.n, d_counts,
                             stream=_stream(torch))
    assert call([(rule, p.G)] * 8) == B.LC_OK
    assert int(d_counts[0].item()) == p.n


# ----------------------------------------------------------------------------------------------------------- pinned upload
@pytest.mark.parametrize("nbytes", [1, 15, 16, 17, 4 * MIB - 16, 4 * MIB, 4 * MIB + 16, 64 * MIB])
def test_pinned_upload_copies_whole_sixteen_byte_pieces_and_nothing_more(torch_dev, nbytes):
    """1024 workgroups x 256 lanes x 16 bytes = 4 MiB per pass of the kernel's loop"""
    torch = torch_dev
    whole = (nbytes + 15) // 16 * 16
    rng = np.random.default_rng(nbytes)
    h_src = torch.empty(whole + 16, dtype=torch.uint8).pin_memory()
    assert h_src.is_pinned() and h_src.data_ptr() % 16 == 0
    h_src.copy_(torch.from_numpy(rng.integers(0, 256, size=whole + 16, dtype=np.uint8)))
    d_dst = torch.full((whole + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert B.upload_pinned(h_src, d_dst, nbytes, stream=_stream(torch)) == B.LC_OK
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got[:whole], h_src.numpy()[:whole])
    assert (got[whole:] == 0xA5).all()


def test_pinned_upload_refuses_unaligned_pointers(torch_dev):
    torch = torch_dev
    h_src = torch.zeros(4096, dtype=torch.uint8).pin_memory()
    d_dst = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert B.upload_pinned(h_src[1:], d_dst, 1024, stream=_stream(torch), check=False) == B.LC_ERR_ARG
    assert B.upload_pinned(h_src, d_dst[1:], 1024, stream=_stream(torch), check=False) == B.LC_ERR_ARG
    with pytest.raises(RuntimeError):
        B.upload_pinned(h_src[1:], d_dst, 1024, stream=_stream(torch))
    torch.cuda.synchronize()
    assert (d_dst.cpu().numpy() == 0xA5).all()                             # nothing was launched
    assert B.upload_pinned(h_src, d_dst, 0, stream=_stream(torch)) == B.LC_OK
    assert B.upload_pinned(h_src[16:], d_dst[32:], 1024, stream=_stream(torch)) == B.LC_OK
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert (got[:32] == 0xA5).all() and (got[32:32 + 1024] == 0).all() and (got[32 + 1024:] == 0xA5).all()
