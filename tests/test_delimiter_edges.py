"""The delimiter split's deterministic edge corpus (tests/helpers/delimiter_edges.py) on a machine without a GPU: first that the corpus
is what it says -- every decision byte on its tile offset, every head for every kind, every status, the doubled flag both ways, counts
on both sides of the key count --, then the product's PER-LINE ROUTINE (delimSplitLine of csrc/delim_vm.hpp through HostLineSource, junk
outside the line) over every line at its head against helpers/delimiter_model.Engine, which tests/test_delimiter_model.py holds to the
reference's recorded output.  tests/test_gpu_delimiter_edges.py runs the same corpus through delim_split_kernel.

Teeth, each mutation of csrc/delim_vm.hpp applied to a scratch copy and the corpus run through it:
  * delimStepPlain without `i + 1 - w.fs < c.sepLen`: caught by separator/doubled and separator/leftmost of the "||" and "@@@@"
    configurations (a separator found overlapping the one before it; "abc" repeats no byte and cannot show it);
  * the trim stopping after its first quad: caught in every configuration by trailing/data, trailing/separator, trailing/close and
    leading/then_trailing wherever the run reaches beyond the line's last quad, and by the all-blank lengths;
  * DOUBLEQUOTE-then-separator without `--w.dq`: caught in every quote-path configuration by quote/close_sep, quote/open,
    quote/sep_inside, quote/qsqsk_sep, quote/qsqsk_close and leading/quoted (bit 31 set on a column without doubled quotes)."""
import ctypes

import numpy as np
import pytest

from helpers import delimiter_edges as de
from helpers.delimiter_model import BLANK, FAIL, OK
from test_delimiter_host import _double

W = 6
KINDS = {"separator", "trailing", "leading", "length"}
CONFIG_IDS = ["%s-%s-%s-%d" % (s.decode().replace("\t", "TAB"), q.decode().replace("\t", "TAB"), m, k) for s, q, m, k in de.CONFIGS]


@pytest.mark.parametrize("k", range(len(de.CONFIGS)), ids=CONFIG_IDS)
def test_the_corpus_is_what_it_says(k):
    cp = de.corpus(k)
    sep, quote, mode, nk = cp.cfg
    use_quote = len(sep) == 1 and quote != sep
    assert len(cp.cases) == len(cp.index) and len(cp.lines) > 3000
    data, off = de.pack(cp.cfg, cp.lines)
    assert len(data) % 16 == 0 and len(data) >= int(off[-1]) + 16 and not (data[int(off[-1]):] == 0).any()
    heads = {}
    for c, i in zip(cp.cases, cp.index):
        assert cp.lines[i] == c.line and int(off[i]) % 16 == c.head, (c.kind, c.variant, c.p, c.head)
        heads.setdefault(c.kind, set()).add(c.head)
        if c.p is not None:   # the decision byte stands on tile offset p: at p - head of the line, at off + p - head of the data
            assert c.pos == c.p - c.head >= de.MIN_POS and c.line[c.pos] == c.byte == data[int(off[i]) + c.p - c.head], (c.kind, c.variant, c.p, c.head)
    assert set(heads) == KINDS | ({"quote"} if use_quote else set())
    assert all(h == set(range(16)) for h in heads.values()), heads
    assert {c.p for c in cp.cases} == set(de.OFFSETS) | {None}
    # the shapes the random tests never make
    trimmed = [len(ln) - len(ln.rstrip(b" \r")) for ln in cp.lines if ln.strip(b" \r")]
    assert {r for r in trimmed if r > 3} >= set(de.RUNS) - {1}
    assert max(len(ln) - len(ln.lstrip(b" ")) for ln in cp.lines if ln.strip(b" \r")) > 120
    if len(sep) > 1:      # every byte of the separator on a stage border
        assert {(c.p, c.variant) for c in cp.cases if c.kind == "separator" and c.p in (63, 64)} >= {(p, "column/%d" % b) for p in (63, 64) for b in range(len(sep))}
    # what the model says about it
    status = [w[0] for w in cp.want]
    assert status.count(OK) > 2000 and status.count(BLANK) > 200
    assert (status.count(FAIL) > 500) if use_quote else (status.count(FAIL) == 0)      # the plain path cannot fail
    case_status = {}
    for c, i in zip(cp.cases, cp.index):
        case_status.setdefault(c.kind, set()).add(cp.want[i][0])
    assert case_status["leading"] >= {OK, BLANK} and case_status["length"] >= {OK, BLANK} and case_status["trailing"] == {OK}
    if use_quote:
        assert case_status["quote"] == {OK, FAIL} and case_status["leading"] >= {FAIL}
        doubled = {d for w in cp.want for _, _, d in w[2]}
        assert doubled == {True, False}
    else:
        assert not any(d for w in cp.want for _, _, d in w[2])
    counts = {w[1] for w in cp.want}
    if mode != "extend":
        assert {nk, nk + 1} <= counts
        if not use_quote:     # the early stop: no line has more, and the remainder column begins AT the separator
            assert max(counts) == nk + 1
            remainders = [(ln, w[2][nk]) for ln, w in zip(cp.lines, cp.want) if w[1] == nk + 1]
            assert len(remainders) > 500 and all(ln[b:b + len(sep)] == sep for ln, (b, e, _) in remainders)


@pytest.mark.parametrize("k", range(len(de.CONFIGS)), ids=CONFIG_IDS)
def test_the_per_line_routine_equals_the_model_on_every_line_at_its_head(k):
    L = _double()
    cp = de.corpus(k)
    sep, quote, mode, nk = cp.cfg
    h = ctypes.c_void_p()
    assert L.lc_delim_create(sep, len(sep), quote[0], {"extend": 0, "keep": 1, "discard": 2}[mode], nk, ctypes.byref(h)) == 0
    _, off = de.pack(cp.cfg, cp.lines)
    n = len(cp.lines)
    status = np.full(n, de.SENT, np.uint8)
    ncols = np.full(n, 0xA5A5A5A5, np.uint32)
    spans = np.full((n, W, 2), de.SENT32, np.int32)
    sp, nc, sa = spans.ctypes.data, ncols.ctypes.data, status.ctypes.data
    for i, ln in enumerate(cp.lines):
        L.dd_split_line(h, ln, len(ln), int(off[i]) % 16, W, sa + i, nc + 4 * i, sp + 8 * W * i)
    L.lc_delim_destroy(h)
    want_status, want_count, want_spans = de.expected_arrays(cp.want, W)
    bad = np.nonzero((status != want_status) | (ncols.astype(np.int64) != want_count))[0]
    assert not len(bad), [(cp.lines[i], int(status[i]), int(ncols[i]), cp.want[i][:2]) for i in bad[:5]]
    ok = want_status == OK
    # every span of the first min(count, W) columns, bit 31 included -- and nothing written behind them
    bad = np.nonzero(ok & (spans != want_spans).any(axis=(1, 2)))[0]
    assert not len(bad), [(cp.lines[i], spans[i].tolist(), cp.want[i]) for i in bad[:5]]
