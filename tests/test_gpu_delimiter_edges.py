"""delim_split_kernel (csrc/delim_kernel.hpp, delim_vm.hpp, wave_tile_source.hpp) at its edges: the deterministic corpus of
tests/helpers/delimiter_edges.py -- every decision byte on the last byte of a quad or stage, the first of the next and one beyond, for
all 16 heads -- through lc_delim_split_device, with sentinel rows around every output array, batch sizes that leave lanes and whole
wavefronts without a line, wavefronts whose stage count comes from one lane or is zero behind the trim, the host entry and the argument
checks.  Every expectation comes from helpers/delimiter_model.Engine (tests/test_delimiter_model.py holds it to the reference's recorded
output), never from the routine compiled for the host; every comparison is bit-exact."""
import random

import numpy as np
import pytest

from helpers import delimiter_edges as de
from helpers.delimiter_model import OK, Engine

pytestmark = pytest.mark.gpu
GUARD = 4      # sentinel rows in front of and behind status, ncols and spans
CONFIG_IDS = ["%s-%s-%s-%d" % (s.decode().replace("\t", "TAB"), q.decode().replace("\t", "TAB"), m, k) for s, q, m, k in de.CONFIGS]


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _engine(cfg):
    from loongcollector_amd import delimiter
    return delimiter.GpuDelimiter(*cfg)


def launch(torch, dl, cfg, lines, W, pad_front=0, what=""):
    """one lc_delim_split_device over the packed lines; the three output arrays lie between GUARD sentinel rows on both sides, everything
    painted with the sentinel byte -> (status u8[n], ncols i64[n], spans i32[n, W, 2]) once the guard rows are seen untouched.
    W = 0 passes d_spans = NULL."""
    dev = torch.device("cuda:0")
    n = len(lines)
    data, off = de.pack(cfg, lines, pad_front)
    row = {"status": 1, "ncols": 4, "spans": 8 * W}
    full = {k: torch.full(((n + 2 * GUARD) * b + 16,), de.SENT, dtype=torch.uint8, device=dev) for k, b in row.items()}
    view = {k: full[k][GUARD * b:] for k, b in row.items()}
    assert view["ncols"].data_ptr() % 4 == 0 and view["spans"].data_ptr() % 8 == 0
    dl.split_device(torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev), n, W, view["status"], view["ncols"], view["spans"] if W else None,
                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw = {k: full[k].cpu().numpy() for k in row}
    for k, b in row.items():
        assert (raw[k][:GUARD * b] == de.SENT).all(), "%s: a guard row in front of %s was written" % (what, k)
        assert (raw[k][(GUARD + n) * b:] == de.SENT).all(), "%s: a guard row behind %s was written" % (what, k)
    body = {k: raw[k][GUARD * b:(GUARD + n) * b] for k, b in row.items()}
    return body["status"], body["ncols"].view(np.uint32).astype(np.int64), body["spans"].view(np.int32).reshape(n, W, 2)


def same(got, want, lines, W, what):
    """status and the TRUE count of every line; for an OK line every span of the first min(count, W) columns with bit 31, and the sentinel
    in the columns behind them; a FAIL or BLANK line reports 0 columns (its row is not looked at: the kernel stores columns as it
    finds them)"""
    status, ncols, spans = got
    want_status, want_count, want_spans = de.expected_arrays(want, W)
    bad = np.nonzero((status != want_status) | (ncols != want_count))[0]
    assert not len(bad), (what, [(i, lines[i][:160], int(status[i]), int(ncols[i]), want[i][:2]) for i in bad[:4]])
    assert (ncols[want_status != OK] == 0).all()
    bad = np.nonzero((want_status == OK) & (spans != want_spans).any(axis=(1, 2)))[0]
    assert not len(bad), (what, [(i, lines[i][:160], spans[i].tolist(), want[i]) for i in bad[:4]])


@pytest.mark.parametrize("k", range(len(de.CONFIGS)), ids=CONFIG_IDS)
def test_the_corpus_on_the_device_at_w_6_and_w_2_between_guard_rows(k):
    from loongcollector_amd import binding
    torch = _torch()
    cp = de.corpus(k)
    dl = _engine(cp.cfg)
    binding.launched_kernels()
    got = launch(torch, dl, cp.cfg, cp.lines, 6, what="W = 6")
    assert "delim_split_kernel" in binding.launched_kernels()
    same(got, cp.want, cp.lines, 6, "W = 6")
    narrow = launch(torch, dl, cp.cfg, cp.lines, 2, what="W = 2")
    same(narrow, cp.want, cp.lines, 2, "W = 2")
    above = sum(w[1] > 2 for w in cp.want)      # the TRUE count above W (one key and the early stop: "abc" never has a third column)
    assert (narrow[1] > 2).sum() == above and (above > 100 or k == 6)


@pytest.mark.parametrize("k", [0, 3])
def test_w_0_with_null_spans_gives_status_and_the_true_count(k):
    torch = _torch()
    cp = de.corpus(k)
    got = launch(torch, _engine(cp.cfg), cp.cfg, cp.lines, 0, what="W = 0")
    same(got, cp.want, cp.lines, 0, "W = 0")
    assert got[1].max() >= 3


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_leave_lanes_and_wavefronts_without_a_line(n):
    """lanes (and, at 1, 63, 64, 65 and 257, whole wavefronts) without a line walk the cooperative stage loop with length 0"""
    torch = _torch()
    for k in (0, 4):
        cp = de.corpus(k)
        pick = [(i * 37) % len(cp.lines) for i in range(n)]
        lines, want = [cp.lines[i] for i in pick], [cp.want[i] for i in pick]
        same(launch(torch, _engine(cp.cfg), cp.cfg, lines, 3, pad_front=5, what="n = %d" % n), want, lines, 3, "n = %d, configuration %d" % (n, k))


def _line(rng, cfg, length):
    """`length` bytes of fields, separators, quoted fields and blanks"""
    sep, quote = cfg[0], cfg[1]
    parts, size = [], 0
    while size < length:
        r = rng.random()
        part = (quote + b"q" * rng.randrange(0, 5) + sep[:1] + quote + sep) if r < 0.15 else (b"v" * rng.randrange(0, 9) + sep) if r < 0.9 else b" "
        parts.append(part)
        size += len(part)
    return b"".join(parts)[:length]


@pytest.mark.parametrize("k", [0, 3], ids=["quote_path", "plain_path"])
def test_wavefronts_whose_stage_count_comes_from_one_lane_or_is_zero_behind_the_trim(k):
    torch = _torch()
    cfg = de.CONFIGS[k]
    model, dl = Engine(*cfg), _engine(cfg)
    rng = random.Random(20261021 + k)
    short = [_line(rng, cfg, rng.choice([0, 1, 2, 15, 16, 17, 63, 64, 65, 200])) for _ in range(256)]
    long_line = ((b"v" + cfg[0]) * 4096)[:4095] + b"w"
    assert len(long_line) == 4096 and model.split_line(long_line)[0] == OK
    for where in (0, 63, 200):          # lane 0, lane 63, and only in wave 3 of the workgroup
        lines = list(short)
        lines[where] = long_line
        want = [model.split_line(ln) for ln in lines]
        same(launch(torch, dl, cfg, lines, 6, pad_front=where % 16, what="long line at %d" % where), want, lines, 6, "long line at %d" % where)
    # a wavefront of 64 all-blank lines of 130 bytes: no stage to walk for the whole wave behind the trim; a normal one follows it
    for first_wave in (0, 1):
        lines = list(short)
        for j in range(64):
            lines[64 * first_wave + j] = de.blanks(130, j)
        want = [model.split_line(ln) for ln in lines]
        assert all(w[0] == 2 for w in want[64 * first_wave:64 * first_wave + 64])
        same(launch(torch, dl, cfg, lines, 6, what="blank wave %d" % first_wave), want, lines, 6, "blank wave %d" % first_wave)


def test_the_host_entry_equals_the_device_entry_over_a_corpus():
    torch = _torch()
    cp = de.corpus(3)
    dl = _engine(cp.cfg)
    W = 6
    status, ncols, spans = launch(torch, dl, cp.cfg, cp.lines, W, what="device")
    data, off = de.pack(cp.cfg, cp.lines)
    hst, hnc, hsp = dl.split_host(data, off, W)
    assert np.array_equal(hst, status) and np.array_equal(hnc.astype(np.int64), ncols)
    live = np.arange(W)[None, :] < np.minimum(ncols, W)[:, None]      # (entries at and behind the count are unspecified: lc_delimiter.h)
    assert np.array_equal(hsp[live], spans[live]) and live.sum() > len(cp.lines)
    same((hst, hnc.astype(np.int64), np.where(live[:, :, None], hsp, de.SENT32)), cp.want, cp.lines, W, "host entry")


def test_argument_errors():
    from loongcollector_amd import binding
    torch = _torch()
    dev = torch.device("cuda:0")
    cfg = de.CONFIGS[0]
    dl = _engine(cfg)
    data, off = de.pack(cfg, [b"a,b", b"c"])
    d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)
    d_st, d_nc = torch.zeros(2, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    L = dl._L
    assert L.lc_delim_split_device(dl.handle, d_data.data_ptr(), d_off.data_ptr(), 2, 4, d_st.data_ptr(), d_nc.data_ptr(), None, None) == binding.LC_ERR_ARG
    assert L.lc_delim_split_device(dl.handle, None, None, 0, 4, None, None, None, None) == binding.LC_OK
    assert L.lc_delim_split_host(dl.handle, None, None, 0, 4, None, None, None) == binding.LC_OK
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [0, 0]


def test_a_tensor_of_another_device_is_refused():
    from loongcollector_amd import binding
    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: nothing lives on another one")
    cfg = de.CONFIGS[0]
    dl = _engine(cfg)
    other = torch.device("cuda:1")
    data, off = de.pack(cfg, [b"a,b"] * 4)
    torch.cuda.set_device(0)
    with pytest.raises(RuntimeError) as e:
        dl.split_device(torch.from_numpy(data).to(other), torch.from_numpy(off).to(other), 4, 2, torch.zeros(4, dtype=torch.uint8, device=other),
                        torch.zeros(4, dtype=torch.int32, device=other), torch.zeros((4, 2, 2), dtype=torch.int32, device=other))
    assert "rc=%d " % binding.LC_ERR_ARG in str(e.value)
