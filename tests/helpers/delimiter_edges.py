"""Test-only: the deterministic edge corpus of the delimiter split (delimSplitLine of csrc/delim_vm.hpp, delim_split_kernel of
csrc/delim_kernel.hpp through csrc/wave_tile_source.hpp).  One author for tests/test_delimiter_edges.py (the per-line routine on the
host) and tests/test_gpu_delimiter_edges.py (the kernel).

The kernel walks a line in 16-byte quads and 64-byte stages counted from the 16-byte boundary at or below the line's first byte ("tile
coordinates": the line's first byte stands at `head`, 0..15).  Every case puts its DECISION BYTE on a chosen tile offset p -- the last
byte of a quad or stage, the first byte of the next, and one beyond -- for every head; in the line the byte stands at p - head.  Each
kind brings its failing and near-miss siblings behind the same filler.  What a line must give always comes from
helpers/delimiter_model.Engine, never from the routine under test.  Not part of the product."""
import functools
from collections import namedtuple

import numpy as np

from helpers.delimiter_model import Engine

# (separator, quote, mode, keys)
CONFIGS = [(b",", b'"', "extend", 3), (b"|", b"'", "keep", 2), (b"\t", b"\t", "discard", 2), (b"||", b'"', "keep", 3),
           (b"@@@@", b'"', "extend", 2), (b",", b'"', "discard", 1), (b"abc", b'"', "keep", 1)]
OFFSETS = (15, 16, 17, 63, 64, 65, 127, 128, 129)
RUNS = (1, 15, 16, 17, 63, 64, 65, 130)          # trailing blanks: the backward walk over 1 to 9 quads
LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65)
MIN_POS = 2                                      # decision bytes below this line position are skipped
SENT = 0xA5                                      # what the GPU test paints its output arrays with
SENT32 = int(np.frombuffer(bytes([SENT] * 4), np.int32)[0])

# pos: the decision byte's position in the line; byte: what stands there; p = head + pos (None: the case has no decision byte)
Case = namedtuple("Case", "kind variant p head pos byte line")


def fill(n):
    assert n >= 0
    return b"f" * n


def blanks(n, salt=0):
    """n bytes of ' ' and '\\r', mixed (both occur from two bytes on)"""
    return bytes(b" \r\r  \r \r"[(i + salt) % 8] for i in range(n))


def _separator_cases(cfg, pos):
    S, Q, mode, nk = cfg
    L = len(S)
    near = S[:-1] + b"f"
    left = S[:1] + S
    for k in range(L):  # byte k of the separator on p
        a = pos - k
        if a < 0:
            continue
        F = fill(a)
        yield "separator", "column/%d" % k, F + S + b"gh", S[k]
        yield "separator", "ends_line/%d" % k, F + S, S[k]
        yield "separator", "doubled/%d" % k, F + S + S + b"g", S[k]
        yield "separator", "leftmost/%d" % k, F + left + b"b", left[k]
        if L > 1:
            yield "separator", "near_miss/%d" % k, F + near + b"g", near[k]
            if k < L - 1:
                yield "separator", "one_short/%d" % k, F + S[:-1], S[k]
        earlier = (S + b"f") * (nk - 1)  # the separator on p is the n_keys-th one
        if a >= len(earlier):
            yield "separator", "nth_key/%d" % k, fill(a - len(earlier)) + earlier + S + b"gh" + S + b"i", S[k]


def _open_prefixes(cfg, n):
    """n bytes after which the walk stands inside a quoted field"""
    S, Q = cfg[0], cfg[1]
    if n >= 1:
        yield "long", Q + fill(n - 1)
    if n >= 5:
        yield "short", fill(n - 4) + S + Q + b"ab"


def _quote_cases(cfg, pos):
    S, Q = cfg[0], cfg[1]
    q = Q[0]
    # the opening quote on p (behind a separator: a quote behind data fails)
    pre = fill(pos - 1) + S
    yield "quote", "open", pre + Q + b"ab" + Q + S + b"c", q
    yield "quote", "open_unterminated", pre + Q + b"ab", q
    yield "quote", "open_close_last", pre + Q + Q, q
    yield "quote", "in_data", fill(pos) + Q + b"a", q
    yield "quote", "in_data_last", fill(pos) + Q, q
    for form, P in _open_prefixes(cfg, pos):
        yield "quote", "close_sep/" + form, P + Q + S + b"c", q
        yield "quote", "close_last/" + form, P + Q, q
        yield "quote", "close_then_data/" + form, P + Q + b"x", q
        yield "quote", "doubled_first_more/" + form, P + Q + Q + b"cd" + Q, q
        yield "quote", "doubled_first_end3/" + form, P + Q + Q + Q, q
        yield "quote", "doubled_first_end2/" + form, P + Q + Q, q
        yield "quote", "doubled_first_sep/" + form, P + Q + Q + b"c" + Q + S + b"d", q
        yield "quote", "sep_inside/" + form, P + S + b"a" + Q + S + b"b", S[0]
        yield "quote", "unterminated_last/" + form, P + b"x", ord("x")
        yield "quote", "qsqsk_sep/" + form, P + S + Q + S + b"k", S[0]
    for form, P in _open_prefixes(cfg, pos - 1):
        yield "quote", "doubled_second_more/" + form, P + Q + Q + b"cd" + Q, q
        yield "quote", "doubled_second_end3/" + form, P + Q + Q + Q, q
        yield "quote", "doubled_second_end2/" + form, P + Q + Q, q
        yield "quote", "doubled_second_sep/" + form, P + Q + Q + Q + S + b"d", q
        yield "quote", "data_behind_close/" + form, P + Q + b"x" + S + b"y", ord("x")
        yield "quote", "qsqsk_close/" + form, P + S + Q + S + b"k", q


def _trim_cases(cfg, pos, use_quote):
    S, Q = cfg[0], cfg[1]
    L = len(S)
    for r in RUNS:
        B = blanks(r, pos + r)
        yield "trailing", "data/%d" % r, fill(pos) + b"g" + B, ord("g")
        yield "trailing", "not_trailing/%d" % r, fill(pos) + b"g" + B + b"h", ord("g")
        if pos >= L - 1:
            yield "trailing", "separator/%d" % r, fill(pos - L + 1) + S + B, S[-1]
        if use_quote:
            yield "trailing", "close/%d" % r, Q + fill(pos - 1) + Q + B, Q[0]


def _leading_cases(cfg, pos, use_quote):
    S, Q = cfg[0], cfg[1]
    run = b" " * pos
    yield "leading", "column", run + b"g" + S + b"h", ord("g")
    yield "leading", "alone", run + b" ", 0x20
    yield "leading", "then_cr", run + b"\r", 0x0D
    yield "leading", "cr_is_data", run + b"\rg", 0x0D
    yield "leading", "then_trailing", run + b"g" + blanks(17, pos), ord("g")
    yield "leading", "separator_first", run + S + b"h", S[0]
    if use_quote:
        yield "leading", "quoted", run + Q + b"a" + S + b"b" + Q + S + b"c", Q[0]
        yield "leading", "quoted_unterminated", run + Q + b"a" + S, Q[0]


def edge_cases(cfg):
    """-> [Case]: every kind at every offset of OFFSETS for every head, and the short lengths for every head"""
    S, Q, mode, nk = cfg
    use_quote = Engine(S, Q, mode, nk).use_quote
    out = []
    for p in OFFSETS:
        for head in range(16):
            pos = p - head
            if pos < MIN_POS:
                continue
            found = list(_separator_cases(cfg, pos)) + list(_trim_cases(cfg, pos, use_quote)) + list(_leading_cases(cfg, pos, use_quote))
            if use_quote:
                found += list(_quote_cases(cfg, pos))
            out += [Case(kind, variant, p, head, pos, byte, line) for kind, variant, line, byte in found]
    for n in LENGTHS:
        for head in range(16):
            out.append(Case("length", "filler/%d" % n, None, head, None, None, fill(n)))
            out.append(Case("length", "blank/%d" % n, None, head, None, None, blanks(n, head)))
            if n >= len(S):
                out.append(Case("length", "separator_last/%d" % n, None, head, None, None, fill(n - len(S)) + S))
    return out


def with_heads(cfg, cases, start=0):
    """filler lines between the cases so that every case line starts at its head (the packed data begins at a 16-byte boundary, `start`
    bytes in front).  -> (lines, indices of the case lines).  The fillers are lines of their own, made of the bytes the routine reacts
    to; they are checked against the model like every other line."""
    S, Q = cfg[0], cfg[1]
    cycle = (Q + S + b" \r" + S[:1] + Q + b"\r " + S) * 3
    lines, index, at = [], [], start
    for c in cases:
        gap = (c.head - at) % 16
        if gap:
            rot = len(lines) % 7
            lines.append(cycle[rot:rot + gap])
            at += gap
        index.append(len(lines))
        lines.append(c.line)
        at += len(c.line)
    return lines, index


def pack(cfg, lines, pad_front=0):
    """lines back to back behind pad_front bytes -> (data u8, padded to a whole 16-byte unit plus one more with bytes the routine reacts
    to, never zeros; off i32[n + 1])"""
    S, Q = cfg[0], cfg[1]
    react = S + Q + b" \r"
    blob = (react * (pad_front // len(react) + 1))[:pad_front] + b"".join(lines)
    size = (len(blob) + 15) // 16 * 16 + 16
    data = np.frombuffer(blob + react * ((size - len(blob)) // len(react) + 1), np.uint8)[:size].copy()
    off = np.zeros(len(lines) + 1, np.int64)
    off[1:] = np.cumsum([len(ln) for ln in lines])
    return data, (off + pad_front).astype(np.int32)


Corpus = namedtuple("Corpus", "cfg cases lines index want")


@functools.lru_cache(maxsize=None)
def corpus(k):
    """configuration k: the cases, the placed lines (fillers included), the case lines' indices, and the MODEL's answer for every line
    (computed once per process; callers leave it unchanged)"""
    cfg = CONFIGS[k]
    cases = edge_cases(cfg)
    lines, index = with_heads(cfg, cases)
    model = Engine(*cfg)
    return Corpus(cfg, cases, lines, index, [model.split_line(ln) for ln in lines])


def expected_arrays(want, W, fill_value=SENT32):
    """the model's answers as the arrays the device writes: status u8[n], the TRUE count i64[n], spans i32[n, W, 2] with bit 31 of begin
    for a doubled column and fill_value in every column from min(count, W) on"""
    n = len(want)
    status = np.array([w[0] for w in want], np.uint8).reshape(n)
    count = np.array([w[1] for w in want], np.int64).reshape(n)
    spans = np.full((n, W, 2), fill_value, np.int64)
    for i, (_, _, cols) in enumerate(want):
        for c, (b, e, doubled) in enumerate(cols[:W]):
            spans[i, c, 0] = (b | 0x80000000) - (1 << 32) if doubled else b
            spans[i, c, 1] = e
    return status, count, spans.astype(np.int32)
