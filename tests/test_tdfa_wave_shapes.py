"""The wave-shape corpus of tests/helpers/wave_shapes.py, without a GPU: that it is what it says (conditions on the INPUTS of
tests/test_gpu_tdfa_wave_shapes.py, so that test cannot pass on a degenerate corpus), that every instantiation the GPU test names
gets the table format it needs, and that the packed tables themselves -- walked by the interpreters of tests/helpers/table_interp.py
-- give the oracle's answer on every line.  A mismatch on the GPU is then the kernel's, not the tables'."""
import numpy as np
import pytest

from loongcollector_amd import binding as B
from oracle.oracle import OracleRegex
from tests.helpers import wave_shapes as ws
from tests.helpers.table_interp import TdfaBlobInterp, TdfaPair1Interp

NAMES = list(ws.FAMILIES)
_cache = {}


def _case(name):
    """(corpus, lengths, oracle captures, oracle status) of a family, computed once"""
    if name not in _cache:
        c = ws.generate(name)
        data, off, length = c.pack()
        caps, status = OracleRegex(c.family.pattern).fullmatch_batch(data, off[:-1], length)
        _cache[name] = (c, length, caps, status)
    return _cache[name]


def _rows(c, w, caps, status):
    """the capture rows of the matched lines of wave w: (begins, ends), one row per line"""
    sl = slice(w.first, w.first + w.count)
    cp = caps[sl][status[sl] == 1]
    return cp[:, 0::2], cp[:, 1::2]


@pytest.mark.parametrize("name", NAMES)
def test_every_wave_kind_and_length_is_there(name):
    c, length, caps, status = _case(name)
    fam = c.family
    uni = c.waves_of("uniform")
    assert [w.L for w in uni] == ws.UNIFORM_L and all(w.count == 64 for w in uni)
    for w in uni:
        assert (length[w.first:w.first + 64] == w.L).all(), w
    edge = [fam.edge_len(L) for L in ws.EDGE_L]
    assert all(e % 64 == L % 64 and e >= L for e, L in zip(edge, ws.EDGE_L))          # (moved by whole stages, if at all)
    short = c.waves_of("one_short")
    assert [w.L for w in short] == [L for L in edge for _ in range(5)]
    seen_lanes = set()
    for k, w in enumerate(short):
        lens = length[w.first:w.first + 64]
        want = ws.short_lengths(w.L)[k % 5]
        odd = np.nonzero(lens != w.L)[0]
        assert odd.tolist() == [ws.SHORT_LANES[k % 4]] and int(lens[odd[0]]) == want, (w, odd, want)
        seen_lanes.add(int(odd[0]))
    assert seen_lanes == set(ws.SHORT_LANES)
    long_ = c.waves_of("one_long")
    assert [w.L for w in long_] == edge
    for w in long_:
        lens = length[w.first:w.first + 64]
        assert sorted(lens.tolist()) == [10] * 63 + [w.L], w
    assert [w.L for w in c.waves_of("two_formats")] == [fam.edge_len(L) for L in ws.TWO_FORMAT_L]
    if fam.can_fail:
        assert [w.L for w in c.waves_of("all_dead")] == list(fam.dead_at) and len(fam.dead_at) == 3
        assert [w.L for w in c.waves_of("half_dead")] == edge
        assert 0 < int(status.sum()) < len(status)                                    # matches and failures
    else:
        # SWEEP: every part of the pattern is optional and the dot takes every byte -- no byte string fails, so there is no dead wave
        assert name == "sweep" and not c.waves_of("all_dead") and not c.waves_of("half_dead") and status.all()
    assert c.waves[-1].kind == "tail" and c.waves[-1].count == ws.TAIL_R[1] and len(c.lines) % 64 == ws.TAIL_R[1]
    assert [n % 64 for n in c.cut_counts()] == list(ws.TAIL_R) and len({int(c.wave_of[n]) for n in c.cut_counts()}) == 3
    assert all(w.first % 64 == 0 for w in c.waves)                                    # a wave of the corpus is a wavefront of the launch
    assert 6000 <= len(c.lines) <= 12000


@pytest.mark.parametrize("name", NAMES)
def test_lines_match_where_they_are_meant_to(name):
    c, length, caps, status = _case(name)
    fam = c.family
    for w in c.waves:
        st, lens = status[w.first:w.first + w.count], length[w.first:w.first + w.count]
        meant = c.meant[w.first:w.first + w.count]
        assert (st == meant).all(), (w, np.nonzero(st != meant)[0][:4])
        able = lens >= fam.min_len                                                    # (the pattern has a match that long)
        if w.kind == "all_dead":
            assert not meant.any(), w
        elif w.kind == "half_dead":
            assert not meant[0::2].any() and meant[1::2].all(), w
        elif w.kind == "uniform":                                                     # all but the needy lanes
            assert not (meant & ~able).any() and int((able & ~meant).sum()) <= ws.NEEDY_LANES, w
        else:
            assert (meant == able).all(), w
        if w.kind in ("two_formats", "tail", "half_dead") or (w.kind == "one_short" and w.L >= fam.min_len):
            assert st.any(), w
    assert not (caps[status == 0] != -1).any()
    # the needy lines: they fail as they are and match with the byte that lies behind them in the packed data
    needy = [i for i in range(len(c.lines)) if c.after[i] != b"\n"]
    assert all(c.waves[int(c.wave_of[i])].kind == "uniform" and c.meant[i] == fam.needy_matches for i in needy)
    lengths = {len(c.lines[i]) for i in needy}
    if name == "sweep":                                                               # (no line fails: the byte behind moves a capture)
        assert lengths == {L for L in ws.UNIFORM_L if L >= 1}
    elif name == "alt":                                                               # (what follows the first five bytes is (d*)(.*))
        assert lengths == {1, 2, 4}
    else:                                                                             # every length the pattern can nearly match at
        assert lengths == {L for L in ws.UNIFORM_L if L >= fam.min_len - 1} and {L % 8 for L in lengths} == set(range(8))
    if needy:
        more = [c.lines[i] + c.after[i] for i in needy]
        ln = np.array([len(s) for s in more], np.uint32)
        of = np.concatenate(([0], np.cumsum(ln)[:-1])).astype(np.uint32)
        cp, st = OracleRegex(fam.pattern).fullmatch_batch(np.frombuffer(b"".join(more), np.uint8), of, ln)
        assert st.all() and all(len(c.lines[i]) + 1 in cp[k] and len(c.lines[i]) + 1 not in caps[i] for k, i in enumerate(needy))


@pytest.mark.parametrize("name", NAMES)
def test_offsets_the_uniform_waves_cover(name):
    """Over the batch every offset 0..L is a capture begin and a capture end (from the first offset the pattern leaves free), and
    inside a wave every offset of the last 18 is (from the length at which the pattern leaves the line room for it); lanes differ;
    one-byte fields at even and odd offsets; empty fields at 0, at L and at the first byte of a stage; a field ends on the last byte
    of a stage."""
    c, length, caps, status = _case(name)
    fam = c.family
    begins, ends, one_byte, empty, stage_end, empty_inside = set(), set(), set(), set(), set(), set()
    for w in c.waves_of("uniform"):
        if w.L > ws.COVER_MAX or w.L < fam.min_len:
            continue
        b, e = _rows(c, w, caps, status)
        assert len(b) >= 64 - ws.NEEDY_LANES
        wb, we = set(b.ravel().tolist()), set(e.ravel().tolist())
        begins |= wb
        ends |= we
        one_byte |= set(b[(e - b) == 1].tolist())
        empty |= set(b[(e == b) & (b >= 0)].tolist())
        empty_inside |= {o for o in b[(e == b) & (b >= 0)].tolist() if o < w.L}
        stage_end |= {o for o in e[(e > b) & (e % 64 == 0)].tolist() if o < w.L}
        assert w.L in set(b[e == b].tolist()), ("no empty field at L", w)
        if w.L >= fam.free_len:
            win = set(range(max(0, w.L - ws.WINDOW + 1), w.L + 1))
            assert win <= wb and win <= we, (w, sorted(win - wb), sorted(win - we))
            if w.L >= 24:                                                             # (a shorter line has fewer than 32 ways to be cut)
                assert len({tuple(r) for r in np.concatenate([b, e], axis=1).tolist()}) >= 32, w   # the separators depend on the lane
    top = max(L for L in ws.UNIFORM_L if L <= ws.COVER_MAX)
    assert set(range(fam.first_begin, top + 1)) <= begins, sorted(set(range(fam.first_begin, top + 1)) - begins)
    assert set(range(fam.first_end, top + 1)) <= ends, sorted(set(range(fam.first_end, top + 1)) - ends)
    assert {o % 2 for o in one_byte} == {0, 1}                                        # both halves of a pair: the DOUBLE entries
    assert {o for o in (64, 128, 192, 256) if o >= fam.min_len} <= empty and {64, 128, 192} <= stage_end
    assert (0 in empty) == fam.empty_at_0
    if fam.empty_in_stage:
        assert {64, 128, 192} <= empty_inside
    if name == "sweep":                                                               # the pattern made for the sweep leaves nothing out
        assert fam.first_begin == fam.first_end == fam.free_len == fam.min_len == 0 and fam.empty_at_0 and fam.empty_in_stage


def _walk(it, s):
    """single-byte walk of the packed tables -> (the byte in which the dead state was reached or None, finalId of the last state)"""
    t, died = it.start_row, None
    for pos, byte in enumerate(s):
        t = int(it.blob[((t & 0xFFFF) + int(it.cmap[byte])) // 4]) & 0xFFFF
        if t == 320 and died is None:                                                 # (state 0: the first row of the table)
            died = pos
    return died, int(it.final_id[(t - 320) // it.row_bytes])


@pytest.mark.parametrize("name", NAMES)
def test_dead_waves_die_where_they_say_and_two_format_waves_end_in_two_states(name):
    c, length, caps, status = _case(name)
    it = TdfaBlobInterp(B.GpuRegex(c.family.pattern))
    for w in c.waves_of("all_dead"):
        assert {_walk(it, s)[0] for s in c.lines[w.first:w.first + 64]} == {w.L}, w
    for w in c.waves_of("half_dead"):
        died = [_walk(it, s)[0] for s in c.lines[w.first:w.first + 64:2]]
        assert all(d is not None and d <= 4 for d in died) and len(set(died)) > 1, (w, died)
    two = c.waves_of("two_formats")
    assert len(two) == 2
    for w in two:
        fids = {_walk(it, s)[1] for s in c.lines[w.first:w.first + 64]}
        assert len(fids) >= 2 and 0xFFFF not in fids, (w, fids)
        assert status[w.first:w.first + 64].all()


@pytest.mark.parametrize("inst", ws.INSTANTIATIONS, ids=[i.id for i in ws.INSTANTIATIONS])
def test_each_instantiation_gets_its_table_format(inst, monkeypatch):
    ws.set_env(monkeypatch, inst)
    rx = B.GpuRegex(ws.FAMILIES[inst.family].pattern)
    assert rx.info()["engine"] == B.LC_ENGINE_TDFA
    blob = rx.table(B.LC_TABLE_TDFA_WIDE_BLOB if inst.compact else B.LC_TABLE_TDFA_BLOB, np.uint32)
    assert blob is not None and ws.table_format(blob) == (inst.block, inst.pair, inst.nogen), (inst, ws.table_format(blob))
    if inst.family == "alt":                                                          # general register programs in every format
        for which in (B.LC_TABLE_TDFA_BLOB, B.LC_TABLE_TDFA_WIDE_BLOB):
            assert not ws.table_format(rx.table(which, np.uint32))[2]
    if inst.family == "words70":                                                      # no compact tables: one launch
        assert rx.table(B.LC_TABLE_TDFA_WIDE_BLOB, np.uint32) is None
    if inst.id == "pair1-256-sweep":
        assert (int(blob[3]) & 0xFFFF) == 25


def _expect(caps, status, i):
    return [int(v) for v in caps[i]] if status[i] else None


@pytest.mark.parametrize("name", NAMES)
def test_single_byte_table_walk_equals_the_oracle(name):
    c, length, caps, status = _case(name)
    it = TdfaBlobInterp(B.GpuRegex(c.family.pattern))
    for i, s in enumerate(c.lines):
        assert it.fullmatch(s) == _expect(caps, status, i), c.label(i)


@pytest.mark.parametrize("name", ["sweep", "fields"])
def test_compact_and_one_stamp_pair_table_walks_equal_the_oracle(name, monkeypatch):
    monkeypatch.setenv("LC_TDFA_PAIR", "2")
    monkeypatch.setenv("LC_TDFA_COMPACT", "512")
    c, length, caps, status = _case(name)
    rx = B.GpuRegex(c.family.pattern)
    plain, p1 = TdfaBlobInterp(rx, compact=True), TdfaPair1Interp(rx)
    assert plain.block == 512 and plain.no_general
    doubles = 0
    for i, s in enumerate(c.lines):
        want = _expect(caps, status, i)
        assert plain.fullmatch(s) == want, c.label(i)
        for head in (0, 5):
            assert p1.fullmatch_pair1(s, head=head) == want, (head, c.label(i))
            doubles += p1.doubles
    assert doubles > 0                                                                # (the settled-double path ran)
