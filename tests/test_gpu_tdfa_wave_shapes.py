"""tdfa_stream_kernel (csrc/tdfa_stream_kernel.hpp) and its epilogue tdfaWriteResults (csrc/tdfa_kernel.hpp) at wave-uniform line
shapes and result edges: the corpus of tests/helpers/wave_shapes.py -- waves whose 64 lines all have a boundary length, or all but
one, or all fail -- through every instantiation the launcher can pick, against the oracle, bit for bit.  The thresholds of the chunk
loop (allNextInside, nextInsideButLast, waveFull, __all(fullNext)) and the epilogue's paths (viaTile, sameMap, rowInRegs, the 16-byte
copy or the dword loop) are decisions of a whole wavefront: a slip in one of them misparses the waves of particular lengths only.
tests/test_tdfa_wave_shapes.py says on the CPU that the corpus holds those waves and that the tables are right.

Every launch starts its lines one byte off (nothing is 16-byte aligned by luck), keeps four sentinel rows in front of and behind the
capture table and the status bytes, and runs in both forms: (off, len) and off[n + 1] with a separator byte."""
import numpy as np
import pytest

from loongcollector_amd import binding as B
from oracle.oracle import OracleRegex
from tests.helpers import wave_shapes as ws
from tests.helpers.guarded_launch import GuardedResults      # (the sentinel rows around the results: shared with tests/test_gpu_chunk_edges.py)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def batches(torch_dev):
    """family -> the corpus on the device and the oracle's rows for it: computed once, shared by every test, left unchanged"""
    torch = torch_dev
    dev = torch.device("cuda:0")
    made = {}

    def get(name):
        if name not in made:
            c = ws.generate(name)
            data, off, length = c.pack()
            caps, status = OracleRegex(c.family.pattern).fullmatch_batch(data, off[:-1], length)
            pad = np.zeros((len(data) + 1 + 31) // 16 * 16, dtype=np.uint8)
            pad[1:1 + len(data)] = data                               # every line starts one byte off
            made[name] = dict(corpus=c, caps=caps, status=status, n=len(c.lines), d_data=torch.from_numpy(pad).to(dev),
                              d_off=torch.from_numpy((off + np.uint32(1)).view(np.int32)).to(dev),
                              d_len=torch.from_numpy(length.view(np.int32)).to(dev))
        return made[name]
    return get


def _launch(torch, rx, batch, n, ngroups, form, caps_shift=0):
    """One launch over the first n lines -> (caps[n, 2 * ngroups], status[n], kernel names).  form: "len" = (off, len), "sep" = off[n + 1]
    and a separator byte, "ragged" = the length-scheduled entry (a permuted order).  caps_shift: the capture table starts that many
    dwords into a 16-byte aligned allocation.  Asserts that the sentinel rows around the results are untouched."""
    res = GuardedResults(torch, n, ngroups, caps_shift)
    d_caps, d_status = res.d_caps, res.d_status
    stream = torch.cuda.current_stream().cuda_stream
    B.launched_kernels()
    if form == "ragged":
        d_scratch = torch.empty((B.sched_scratch_bytes(n) // 4 + 1,), dtype=torch.int32, device=torch.device("cuda:0"))
        rx.match_device_ragged(batch["d_data"], batch["d_off"], batch["d_len"], n, d_caps, d_status, d_scratch, ngroups=ngroups,
                               engine=B.LC_ENGINE_TDFA, stream=stream)
    elif form == "len":
        rx.match_device(batch["d_data"], batch["d_off"], batch["d_len"], n, d_caps, d_status, ngroups=ngroups, sep_bytes=0, stream=stream,
                        engine=B.LC_ENGINE_TDFA)
    else:
        rx.match_device(batch["d_data"], batch["d_off"], None, n, d_caps, d_status, ngroups=ngroups, sep_bytes=1, stream=stream,
                        engine=B.LC_ENGINE_TDFA)
    torch.cuda.synchronize()
    names = B.launched_kernels().split(", ")
    caps, status = res.read((form, n, ngroups, caps_shift))
    return caps, status, names


def _expected(batch, n, ngroups):
    """the oracle's rows for the first n lines at ngroups output groups: fewer groups cut the row, further ones read -1"""
    caps, status = batch["caps"][:n], batch["status"][:n]
    G = caps.shape[1] // 2
    if ngroups <= G:
        return caps[:, :2 * ngroups], status
    return np.concatenate([caps, np.full((n, 2 * (ngroups - G)), -1, np.int32)], axis=1), status


def _compare(batch, got_caps, got_status, n, ngroups, where):
    exp_caps, exp_status = _expected(batch, n, ngroups)
    bad = np.nonzero((got_status != exp_status) | (got_caps != exp_caps).any(axis=1))[0]
    if bad.size:
        c, i = batch["corpus"], int(bad[0])
        waves = sorted({int(c.wave_of[k]) for k in bad})
        pytest.fail("%s: %d lines differ, in %d waves %s; first: %s\n  expected status %d row %s\n  actual   status %d row %s" % (
            where, bad.size, len(waves), [(c.waves[w].kind, c.waves[w].L) for w in waves[:12]], c.label(i),
            int(exp_status[i]), exp_caps[i].tolist(), int(got_status[i]), got_caps[i].tolist()))


def _compile(inst, monkeypatch):
    """the pattern of an instantiation compiled under its environment, and that its tables have the format the kernel name stands for"""
    ws.set_env(monkeypatch, inst)
    rx = B.GpuRegex(ws.FAMILIES[inst.family].pattern)
    assert rx.info()["engine"] == B.LC_ENGINE_TDFA
    blob = rx.table(B.LC_TABLE_TDFA_WIDE_BLOB if inst.compact else B.LC_TABLE_TDFA_BLOB, np.uint32)
    assert blob is not None and ws.table_format(blob) == (inst.block, inst.pair, inst.nogen), (inst.id, ws.table_format(blob))
    return rx


@pytest.mark.parametrize("inst", ws.INSTANTIATIONS, ids=[i.id for i in ws.INSTANTIATIONS])
def test_whole_corpus_through_each_instantiation(torch_dev, monkeypatch, batches, inst):
    rx = _compile(inst, monkeypatch)
    batch = batches(inst.family)
    n, G = batch["n"], rx.groups
    assert n % 64 == ws.TAIL_R[1]                                     # (the last wave has lanes without a line)
    for form in ("len", "sep"):
        caps, status, names = _launch(torch_dev, rx, batch, n, G, form)
        assert inst.kernel in names, (inst.id, form, names)           # (the instantiation the row names is what ran)
        _compare(batch, caps, status, n, G, "%s, %s form" % (inst.id, form))


EDGE_INSTS = [i for i in ws.INSTANTIATIONS if i.id in ("pair1-256-sweep", "compact-pair1-512-fields")]


@pytest.mark.parametrize("inst", EDGE_INSTS, ids=[i.id for i in EDGE_INSTS])
def test_epilogue_edges(torch_dev, monkeypatch, batches, inst):
    """The capture table 4, 8 and 12 bytes into an aligned allocation (the dword copy out of the tile instead of the 16-byte one); 0 groups
    (status only), 1, the pattern's own count and 3 more (the extra slots read -1); n = 64k + r (the last wave has lanes without a line,
    and writes its rows lane by lane); the length-scheduled entry (a permuted order).  All against the same oracle rows."""
    rx = _compile(inst, monkeypatch)
    batch = batches(inst.family)
    n, G = batch["n"], rx.groups
    for shift in (0, 1, 2, 3):
        for ngroups in (0, 1, G, G + 3):
            caps, status, names = _launch(torch_dev, rx, batch, n, ngroups, "len" if shift % 2 else "sep", caps_shift=shift)
            assert inst.kernel in names, names
            _compare(batch, caps, status, n, ngroups, "%s, table %d bytes off, %d groups" % (inst.id, 4 * shift, ngroups))
    for cut in batch["corpus"].cut_counts():
        assert cut % 64 in ws.TAIL_R and cut < n
        for shift in (0, 1):
            caps, status, _ = _launch(torch_dev, rx, batch, cut, G, "len", caps_shift=shift)
            _compare(batch, caps, status, cut, G, "%s, %d lines, table %d bytes off" % (inst.id, cut, 4 * shift))
    for shift in (0, 2):
        caps, status, names = _launch(torch_dev, rx, batch, n, G, "ragged", caps_shift=shift)
        assert inst.kernel in names, names
        _compare(batch, caps, status, n, G, "%s, length-scheduled, table %d bytes off" % (inst.id, 4 * shift))
