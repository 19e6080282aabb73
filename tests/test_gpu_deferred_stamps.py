"""The compact one-stamp pair kernel with its capture stamps deferred (tdfa_stream_kernel.hpp kLabDeferStamps, LC_TDFA_DEFER_STAMPS=1) and with a
stamp per pair (=0, the default), and the result epilogue that builds a row from registers read once (tdfa_kernel.hpp
tdfaWriteResults): one workgroup's worth of lines and a bit more, against the oracle.  The walk is pinned store for store on the
CPU in tests/test_deferred_stamps.py."""
import numpy as np
import pytest

from loongcollector_amd import binding as B
from loongcollector_amd import corpus
from oracle.oracle import OracleRegex
from tests.helpers.table_interp import TdfaPair1Interp

pytestmark = pytest.mark.gpu

# adjacent one-byte and empty fields: DOUBLE entries, folded set registers, a stamp on nearly every byte
FIELDS = rb"(\w)(\w)(\w?)(\w*),(\d?)(\d*);(.)(.)(.*)"
# nine one-byte fields in a row: every start register is derived from the one before it (a chain of derive words, resolved by the
# epilogue on the slot map), four real stamps of a lane in one chunk
CHAIN = rb"(\w)(\w)(\w)(\w)(\w)(\w)(\w)(\w)(\w) (\d*)(.*)"
COUNTS = [1, 63, 64, 65, 511, 513]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return torch


def _run(torch, rx, data, off, length, scratch=False):
    """-> (caps, status, kernel names); off has one entry per line.  scratch: through the length-scheduled entry (a permuted order)"""
    dev = torch.device("cuda:0")
    n, G = len(off), rx.groups
    pad = np.zeros(max(1, len(data)) + 1, dtype=np.uint8)
    pad[1:1 + len(data)] = data                                   # (every line starts one byte off: nothing is 16-byte aligned by luck)
    d_data = torch.from_numpy(pad).to(dev)
    d_off = torch.from_numpy((np.ascontiguousarray(off, dtype=np.uint32) + np.uint32(1)).view(np.int32)).to(dev)
    d_len = torch.from_numpy(np.ascontiguousarray(length, dtype=np.uint32).view(np.int32)).to(dev)
    d_caps = torch.full((n, 2 * G), -7, dtype=torch.int32, device=dev)
    d_status = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    B.launched_kernels()
    if scratch:
        d_scratch = torch.empty((B.sched_scratch_bytes(n) // 4 + 1,), dtype=torch.int32, device=dev)
        rx.match_device_ragged(d_data, d_off, d_len, n, d_caps, d_status, d_scratch, engine=B.LC_ENGINE_TDFA,
                               stream=torch.cuda.current_stream().cuda_stream)
    else:
        rx.match_device(d_data, d_off, d_len, n, d_caps, d_status, ngroups=G, sep_bytes=0,
                        stream=torch.cuda.current_stream().cuda_stream, engine=B.LC_ENGINE_TDFA)
    torch.cuda.synchronize()
    return d_caps.cpu().numpy(), d_status.cpu().numpy(), B.launched_kernels()


def _pack(subs):
    length = np.array([len(s) for s in subs], np.uint32)
    off = np.zeros(len(subs), np.uint32)
    off[1:] = np.cumsum(length)[:-1]
    data = np.frombuffer(b"".join(subs), np.uint8) if int(length.sum()) else np.zeros(0, np.uint8)
    return data, off, length


# One wave of every corpus from 128 lines on (lines 64..127) is ALL LONG: 200..260 bytes, no short line in it, so that its shortest span
# lets whole stages run the copy of the chunk loop that does not ask (ALLFULL) and the deferred-stamp queue is walked by that copy too.
LONG_WAVE = range(64, 128)


def _long_a_lines():
    out = []
    for w in (200, 213, 231, 248, 260):
        data, off, length = corpus.apache_batch(13, "A", line_bytes=w, pool_lines=64)
        out += [bytes(data[off[i]:off[i] + length[i]]) for i in range(13)]
    return out


def _regex_a_lines(n, rng):
    data, off, length = corpus.apache_batch(n, "A", empty_every=5)
    subs = [bytes(data[off[i]:off[i] + length[i]]) for i in range(n)]
    long_lines = _long_a_lines() if n > LONG_WAVE[0] else []
    for i in range(n):
        if i in LONG_WAVE:
            subs[i] = long_lines[i - LONG_WAVE[0]]
        elif i % 64 == 7:
            subs[i] = b"no match " + subs[i][:40]                  # a line that fails in every wave
        elif i % 3 == 1:                                          # ragged: the free last field cut or stretched, 0..600 bytes
            want = int(rng.integers(0, 601))
            subs[i] = subs[i][:want] if want < len(subs[i]) else subs[i][:-1] + b"y" * (want - len(subs[i])) + b'"'
    if n > 2:
        subs[2] = subs[2][:-1] + b"z" * 66000 + b'"'              # 64 KiB and more: left to the launch behind the compact one
    return subs


def _field_lines(n, rng):
    alphabet = list(b"ab1 ,;_9")
    subs = []
    for i in range(n):
        if i in LONG_WAVE:
            subs.append(b"ab" + b"c" * (i % 3) + b"," + b"7" * (i % 4) + b";xy" + bytes(rng.choice(alphabet, size=194 + (i * 7) % 50).astype(np.uint8)))
        elif i % 64 == 9:
            subs.append(b";;no comma")
        elif i % 4 == 0:
            subs.append(b"ab" + b"c" * (i % 3) + b"," + b"7" * (i % 4) + b";xy" + bytes(rng.choice(alphabet, size=int(rng.integers(0, 600))).astype(np.uint8)))
        elif i % 4 == 1:
            subs.append(b"xy,;..")
        else:
            subs.append(bytes(rng.choice(alphabet, size=int(rng.integers(0, 40))).astype(np.uint8)))
    if n > 1:
        subs[1] = b"abcd,12;pq" + b"w" * 65600
    return subs


def _chain_lines(n, rng):
    subs = []
    for i in range(n):
        if i in LONG_WAVE:
            subs.append(b"abcdefghi " + b"7" * (i % 5) + b" " + b"r" * (189 + (i * 11) % 46))
        elif i % 64 == 11:
            subs.append(b"abcdefgh 1")
        else:
            subs.append(b"abcdefghi " + b"7" * (i % 5) + (b" " + b"r" * int(rng.integers(0, 590)) if i % 2 else b""))
    return subs


@pytest.fixture(scope="module")
def cases():
    """(pattern, lines, oracle captures, oracle status) per pattern and line count, computed once"""
    out = {}
    for name, pattern, make in (("A", corpus.REGEX_A, _regex_a_lines), ("fields", FIELDS, _field_lines), ("chain", CHAIN, _chain_lines)):
        for n in COUNTS:
            subs = make(n, np.random.default_rng(n))
            data, off, length = _pack(subs)
            caps, status = OracleRegex(pattern).fullmatch_batch(data, off, length)
            out[name, n] = (pattern, data, off, length, caps, status)
    return out


@pytest.mark.parametrize("defer", ["1", "0"])
@pytest.mark.parametrize("name", ["A", "fields", "chain"])
def test_one_workgroup_and_a_bit_more_against_the_oracle(torch_dev, monkeypatch, cases, name, defer):
    monkeypatch.setenv("LC_TDFA_PAIR", "2")
    monkeypatch.setenv("LC_TDFA_COMPACT", "512")
    monkeypatch.setenv("LC_TDFA_DEFER_STAMPS", defer)
    rx = None
    for n in COUNTS:
        pattern, data, off, length, exp_caps, exp_status = cases[name, n]
        rx = rx or B.GpuRegex(pattern)
        blob = rx.table(B.LC_TABLE_TDFA_WIDE_BLOB, np.uint32)
        assert blob is not None and int(blob[7]) and int(blob[int(blob[7]) // 4 + 4]) == 1, "no one-stamp pair table"
        if name == "chain":                                       # (a derived register that is the source of another one: the epilogue's back-chase)
            derive = TdfaPair1Interp(rx).derive
            assert {a for _, a, _ in derive} & {b for b, _, _ in derive}, derive
        caps, status, names = _run(torch_dev, rx, data, off, length)
        assert "pair1" in names and "compact" in names, names
        assert ("pair1,dma,defer>" in names) == (defer == "1"), (defer, names)   # (the instantiation the knob asks for is what ran)
        bad = np.nonzero((status != exp_status) | (caps != exp_caps).any(axis=1))[0]
        assert bad.size == 0, (name, n, defer, bad[:8].tolist(), caps[bad[0]].tolist(), exp_caps[bad[0]].tolist(), int(length[bad[0]]))
        if n >= 64:
            assert 0 < int(exp_status.sum()) < n


@pytest.mark.parametrize("defer", ["1", "0"])
def test_epilogue_with_more_than_one_slot_trip_and_a_permuted_order(torch_dev, monkeypatch, defer):
    """40 groups (80 slots: the row does not fit the registers, two trips of 64 slots) and 12 groups (the row in registers), in
    line order and through the length-scheduled entry, whose order is a permutation (rows leave lane by lane)"""
    monkeypatch.setenv("LC_TDFA_PAIR", "2")
    monkeypatch.setenv("LC_TDFA_COMPACT", "512")
    monkeypatch.setenv("LC_TDFA_DEFER_STAMPS", defer)
    rng = np.random.default_rng(3)
    for groups in (40, 12):
        pattern = b" ".join([rb"(\w+)"] * (groups - 1)) + rb" ?(.*)"
        subs = []
        for i in range(130):
            words = [b"w" * int(rng.integers(1, 6)) for _ in range(groups - 1)]
            s = b" ".join(words) + (b" tail %d" % i if i % 3 else b"")
            subs.append(s[:17] if i % 64 == 5 else s)               # (a line that fails in every wave)
        data, off, length = _pack(subs)
        exp_caps, exp_status = OracleRegex(pattern).fullmatch_batch(data, off, length)
        assert 0 < int(exp_status.sum()) < len(subs)
        rx = B.GpuRegex(pattern)
        assert rx.groups == groups and rx.info()["engine"] == B.LC_ENGINE_TDFA
        for scratch in (False, True):
            caps, status, names = _run(torch_dev, rx, data, off, length, scratch=scratch)
            assert "tdfa_stream_kernel" in names, names
            assert np.array_equal(status, exp_status) and np.array_equal(caps, exp_caps), (groups, scratch, defer)
