"""dfa_screen_kernel (csrc/screen_kernel.hpp, lc_regex_screen_device) at its edges: one value per lane, 16-byte pieces read from
`address & ~15`, bytes taken with `bi >= head && bi < total`, the walk left on the sink, and a list of accepted values that is
APPENDED to (the count is incremented, not set).  The corpus is tests/helpers/chunk_edges.py screen_corpus: every decision on offsets
0..33 for every residue mod 16, packed in the (off, len) form with filler between the values and the `after` byte behind each -- a
NEEDY value is accepted only if the byte behind it is read.  What is expected is TdfaInterp(screen).fullmatch over the same tables;
tests/test_chunk_edges.py says on the CPU that this is the oracle's answer on every case and that values end, and the sink is reached,
on both sides of the first two piece borders for all 16 residues.

Every launch has sentinel words in front of the list, behind its last possible entry and around the count word; entries of the list
the launch did not fill keep the sentinel."""
import numpy as np
import pytest

from loongcollector_amd import binding as B
from tests.helpers import chunk_edges as ce
from tests.helpers.table_interp import TdfaInterp

pytestmark = pytest.mark.gpu

PAD = 8                        # sentinel words on each side
SENTINEL = -7
SIZES = (1, 255, 256, 257, 513)                # around one and two workgroups of 256 lanes


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def batches(torch_dev):
    """family -> the screen, the corpus on the device with values of length 0 and 1 behind it, and what the tables say of each
    value: computed once per family, left unchanged"""
    torch = torch_dev
    dev = torch.device("cuda:0")
    made = {}

    def get(name):
        if name not in made:
            c = ce.screen_corpus(name)
            scr = ce.compile_screen(name)
            it = TdfaInterp(scr)
            data, off, length, residue = c.pack("len")
            assert [int(r) for r in residue] == [k.head for k in c.cases]
            # values of length 0 and of length 1 at every residue: views into the packed data (the bytes are whatever lies there)
            at = np.array([int(off[i]) + j for i in range(40, 44) for j in range(16)], np.uint32)
            assert set(int(a) % 16 for a in at) == set(range(16)) and int(at.max()) + 1 < len(data) - ce.GUARD_BYTES
            off = np.concatenate([off, at, at]).astype(np.uint32)
            length = np.concatenate([length, np.zeros(len(at), np.uint32), np.ones(len(at), np.uint32)]).astype(np.uint32)
            values = [bytes(data[int(o):int(o) + int(n)]) for o, n in zip(off, length)]
            assert values[:len(c.cases)] == c.lines
            want = np.array([it.fullmatch(v) is not None for v in values])
            short = np.arange(len(c.cases), len(values))
            assert not want[short[:len(at)]].any()                                                      # a value of length 0 is never accepted
            d_data = torch.from_numpy(data.copy()).to(dev)
            assert d_data.data_ptr() % 16 == 0                                                          # a value's residue is its offset's
            made[name] = dict(scr=scr, n=len(values), want=want, short=short, corpus=c,
                              d_data=d_data, d_off=torch.from_numpy(off.view(np.int32).copy()).to(dev),
                              d_len=torch.from_numpy(length.view(np.int32).copy()).to(dev))
        return made[name]
    return get


def _screen(torch, b, n, lines=None, count0=0, where=""):
    """one launch over the first n values (or over the n values `lines` lists) with the count word at count0 -> the entries the launch
    appended, in the order found.  Asserts the sentinels, the count and that nothing else of the list was written."""
    dev = torch.device("cuda:0")
    room = count0 + n                                                                                   # the list cannot grow beyond this
    out = torch.full((PAD + room + PAD,), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((PAD + 1 + PAD,), SENTINEL, dtype=torch.int32, device=dev)
    cnt[PAD] = count0
    d_lines = None if lines is None else torch.from_numpy(np.asarray(lines, np.uint32).view(np.int32).copy()).to(dev)
    B.launched_kernels()
    b["scr"].screen_device(b["d_data"], b["d_off"], b["d_len"], n, out[PAD:], cnt[PAD:], d_lines=d_lines,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    names = B.launched_kernels().split(", ")
    assert ("dfa_screen_kernel" in names) == (n > 0), (where, names)                                    # (no values: no launch)
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    assert (cnt[:PAD] == SENTINEL).all() and (cnt[PAD + 1:] == SENTINEL).all(), ("words around the count were written", where)
    k = int(cnt[PAD]) - count0
    assert 0 <= k <= n, (where, k, n)
    assert (out[:PAD + count0] == SENTINEL).all(), ("words in front of the appended entries were written", where)
    assert (out[PAD + count0 + k:] == SENTINEL).all(), ("words behind the appended entries were written", where)
    return out[PAD + count0:PAD + count0 + k]


def _check(b, got, listed, where):
    """the appended entries, sorted, are the accepted ones of the `listed` values: each occurrence counts"""
    listed = np.asarray(listed, np.int64)
    exp = np.sort(listed[b["want"][listed]])
    got = np.sort(got.astype(np.int64))
    if not np.array_equal(got, exp):
        c = b["corpus"]
        g, e = np.bincount(got[(got >= 0) & (got < b["n"])], minlength=b["n"]), np.bincount(exp, minlength=b["n"])
        bad = np.nonzero(g != e)[0]
        first = int(bad[0]) if bad.size else -1
        label = c.label(first) if 0 <= first < len(c.cases) else "value %d (length 0 or 1)" % first
        pytest.fail("%s: %d entries for %d expected, %d values differ, by kind %s; first: %s, listed %d times, expected %d entries, got %d" % (
            where, len(got), len(exp), bad.size, c.kinds_of([i for i in bad if i < len(c.cases)]), label, int((listed == first).sum()),
            int(e[first]) if bad.size else 0, int(g[first]) if bad.size else 0))


@pytest.mark.parametrize("name", ce.SCREEN_FAMILIES)
def test_screen_lists_exactly_the_values_its_tables_accept(torch_dev, batches, name):
    torch = torch_dev
    b = batches(name)
    N = b["n"]
    rng = np.random.default_rng(16)
    # every value
    _check(b, _screen(torch, b, N, where="all"), np.arange(N), "%s, all %d values" % (name, N))
    # a permuted subset of 4k + 3 values
    subset = rng.permutation(N)[:1027]
    assert len(subset) % 4 == 3
    _check(b, _screen(torch, b, len(subset), lines=subset, where="subset"), subset, "%s, a permuted subset of %d" % (name, len(subset)))
    # a list that names values twice: each occurrence is looked at, an accepted value that is named twice is listed twice
    twice = np.concatenate([subset[:300], subset[100:400][::-1], subset[:5]])
    assert int(b["want"][subset[100:300]].sum()) >= 20
    _check(b, _screen(torch, b, len(twice), lines=twice, where="twice"), twice, "%s, a list that names values twice" % name)
    # the first n values, and n listed ones, around one and two workgroups
    for n in SIZES:
        _check(b, _screen(torch, b, n, where="n=%d" % n), np.arange(n), "%s, the first %d values" % (name, n))
        _check(b, _screen(torch, b, n, lines=subset[:n], where="n=%d listed" % n), subset[:n], "%s, %d listed values" % (name, n))
    # no values: nothing is written and the count stays what it was
    for count0 in (0, 5):
        assert len(_screen(torch, b, 0, count0=count0, where="n=0")) == 0
        assert len(_screen(torch, b, 0, lines=subset[:1], count0=count0, where="n=0 listed")) == 0
    # the count is incremented, not set: a list that already holds 5 entries keeps them (_screen asserts out[0:5] and count = 5 + k)
    _check(b, _screen(torch, b, 257, count0=5, where="count 5"), np.arange(257), "%s, 257 values behind 5 entries" % name)
    _check(b, _screen(torch, b, len(subset), lines=subset, count0=5, where="count 5, subset"), subset, "%s, the subset behind 5 entries" % name)
    # values of length 0 (never accepted) and of length 1, at every residue
    short = b["short"]
    assert len(short) == 128
    _check(b, _screen(torch, b, len(short), lines=short, where="short"), short, "%s, values of length 0 and 1" % name)
    _check(b, _screen(torch, b, 1, lines=short[:1], where="one empty value"), short[:1], "%s, one value of length 0" % name)
