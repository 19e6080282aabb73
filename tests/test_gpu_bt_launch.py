"""The LAUNCH layer of the device backtracking engine (gpu_runtime.hip launchBt, bt_kernel.hpp bt_match_kernel) at its thresholds: the
second pass that re-walks a value which filled its 2048-word slice with 16384 words, the rule that hands every lane the large slice,
programs walked from global memory, the refusal, the scratch cache and the pool, the d_lines / d_nlines / d_from forms, the step budget.

The values come from the stack-depth family of tests/helpers/bt_launch_cases.py: one value costs 10 words of stack per "ab", so a value
sits exactly on either side of a cap.  Every launch here: status pre-filled with 9 and captures with -7 inside guarded allocations
(tests/helpers/guarded_launch.py), every status byte received one of LC_NOMATCH / LC_MATCH / LC_GAVE_UP -- the pending byte of the
two-pass protocol never leaves a match call --, status and captures equal to expected() bit for bit (decided values: OracleRegex
cross-checked against CPython's re; the conditions: tests/test_bt_launch_model.py), and bt_match_kernel among the launched kernels.
Nothing is timed; every case ends in an ordinary status byte."""
import numpy as np
import pytest

from loongcollector_amd import binding as B
from tests.helpers import bt_launch_cases as bl
from tests.helpers import fresh_thread
from tests.helpers.guarded_launch import CAPS_SENTINEL, STATUS_SENTINEL, GuardedResults

pytestmark = pytest.mark.gpu

FINAL = (B.LC_NOMATCH, B.LC_MATCH, B.LC_GAVE_UP)
PENDING_BYTE = 4      # bt_kernel.hpp:25 kBtPending


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return torch


def launch(torch, pattern, values, form="len", flags=0, lines=None, nlines=None, frm=None, status_fill=STATUS_SENTINEL, refused=False):
    """One match call over `values` -> (caps[N, 2G], status[N]) for ALL N rows (the sentinels around them asserted); lines / nlines /
    frm: lc_regex_match_device_from.  refused=True: the call must return LC_ERR_UNSUPPORTED."""
    dev = torch.device("cuda:0")
    rx = bl.compiled(pattern, flags)[0]
    data, off, length, sep = bl.pack(values, form)
    d_data = torch.from_numpy(data.copy()).to(dev)
    i32 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).to(dev)
    d_off, d_len = i32(off), i32(length)
    N = len(values)
    res = GuardedResults(torch, N, rx.groups, 0, status_fill)
    stream = torch.cuda.current_stream().cuda_stream
    B.launched_kernels()
    if refused:
        rc = rx._L.lc_regex_match_device_engine(rx.handle, B.LC_ENGINE_AUTO, d_data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), sep, N,
                                                rx.groups, res.d_caps.data_ptr(), res.d_status.data_ptr(), stream)
        assert rc == B.LC_ERR_UNSUPPORTED, rc
    elif lines is not None or nlines is not None or frm is not None:
        rx.match_device_from(d_data, d_off, d_len, N if lines is None else len(lines), res.d_caps, res.d_status, d_lines=i32(lines),
                             d_nlines=i32(None if nlines is None else [nlines]), d_from=i32(frm), sep_bytes=sep, stream=stream)
    else:
        rx.match_device(d_data, d_off, d_len, N, res.d_caps, res.d_status, sep_bytes=sep, stream=stream)
    torch.cuda.synchronize()
    names = B.launched_kernels().split(", ")
    assert refused or "bt_match_kernel" in names, names
    return res.read((len(pattern), form, N))


def check(got, exp, where, listed=None, status_fill=STATUS_SENTINEL):
    """the `listed` rows (default: all) hold final status bytes and equal the expectation; every other row is as it was"""
    (caps, status), (exp_caps, exp_status) = got, exp
    took = np.ones(len(status), bool) if listed is None else np.zeros(len(status), bool)
    if listed is not None:
        took[np.asarray(listed, np.int64)] = True
    assert set(status[took].tolist()) <= set(FINAL), (where, sorted(set(status[took].tolist())))
    wrong = (status != exp_status) | (caps != exp_caps).any(axis=1)
    untouched = (status == status_fill) & (caps == CAPS_SENTINEL).all(axis=1)
    bad = np.nonzero(np.where(took, wrong, ~untouched))[0]
    if bad.size:
        i = int(bad[0])
        pytest.fail("%s: %d rows differ; first: row %d%s, expected status %d caps %s, actual status %d caps %s" % (
            where, bad.size, i, "" if took[i] else " (NOT LISTED: must keep its sentinels)", int(exp_status[i]), exp_caps[i].tolist(),
            int(status[i]), caps[i].tolist()))


def row_of(values, got, value):
    i = values.index(value)
    return int(got[1][i]), got[0][i].tolist()


# ------------------------------------------------------------------------------------------------ the two slice caps
@pytest.mark.parametrize("form", ["len", "sep"])
def test_the_two_slice_caps(torch_dev, form):
    """P(0), V and N at k = 1, 201..204, 1635..1638: k = 202 is the last value pass 1 decides, 203 the first left pending, 1636 the last
    pass 2 decides, 1637 the first LC_GAVE_UP; N(k) needs 8 words less, so N(1637) -- 16 382 words -- is still decided."""
    p = bl.P(0)
    values = bl.values_of(bl.edge_ks(bl.NCAPS))
    assert len(values) == 18
    got = launch(torch_dev, p, values, form)
    check(got, bl.expected(p, values), "slice caps, %s form" % form)
    assert row_of(values, got, bl.V(203)) == (B.LC_MATCH, [404, 405]) and row_of(values, got, bl.V(1636)) == (B.LC_MATCH, [3270, 3271])
    assert row_of(values, got, bl.V(1637))[0] == B.LC_GAVE_UP and row_of(values, got, bl.V(1638))[0] == B.LC_GAVE_UP
    assert row_of(values, got, bl.N(1637)) == (B.LC_NOMATCH, [-1, -1]) and row_of(values, got, bl.N(1638)) == (B.LC_GAVE_UP, [-1, -1])


# ------------------------------------------------------------------------------------------------ where the pending values sit
def batch_with_pending(n, swap=0):
    """n short values (V / N at k = 1, 2, 3) with V(203) -- pending after pass 1, decided by pass 2 -- and V(1637) -- LC_GAVE_UP after
    pass 2 -- alternating over the slots 0, 63, 64, 127, 128 and n - 1"""
    short = bl.values_of(bl.SHORT_KS)
    values = [short[i % len(short)] for i in range(n)]
    slots = sorted({s for s in (0, 63, 64, 127, 128, n - 1) if s < n})
    for j, s in enumerate(slots):
        values[s] = (bl.V(bl.PENDING_K), bl.V(bl.GAVE_UP_K))[(j + swap) % 2]
    return values, slots


@pytest.mark.parametrize("n,lanes", [(65, 64), (200, 64), (1088, None), (8256, None)])
def test_pending_values_in_any_slot_are_taken_by_the_second_pass(torch_dev, monkeypatch, n, lanes):
    """n = 65, 200 under LC_BT_LANES=64: pass 1 is one block in a grid-stride loop, pass 2 one block.  n = 1088: 17 blocks, two retry
    blocks -- a pending value's slot belongs to a lane of the second.  n = 8256: 129 blocks x 64 lanes x 8 KB is above 64 MB, so the
    scratch comes from the stream-ordered pool, with pending values in it; 16 retry blocks."""
    if lanes:
        monkeypatch.setenv("LC_BT_LANES", str(lanes))
    else:
        monkeypatch.delenv("LC_BT_LANES", raising=False)
    p = bl.P(0)
    for swap in (0, 1):
        values, slots = batch_with_pending(n, swap)
        got = launch(torch_dev, p, values)
        check(got, bl.expected(p, values), "n = %d, lanes %s, arrangement %d" % (n, lanes, swap))
        assert {int(got[1][s]) for s in slots} == {B.LC_MATCH, B.LC_GAVE_UP}


def test_the_scratch_cache_grows_between_launches(torch_dev):
    """One thread (a fresh one: its cache starts empty), one stream: n = 64 (4 MB of scratch), n = 1088 (the block is freed and a
    larger one allocated), n = 64 again (the larger block is kept) -- each with a pending value and one that gives up."""
    p = bl.P(0)

    def body():
        torch_dev.cuda.set_device(0)
        out = []
        for n in (64, 1088, 64):
            values, _ = batch_with_pending(n)
            out.append((n, values, launch(torch_dev, p, values)))
        return out

    for n, values, got in fresh_thread.run(body):
        check(got, bl.expected(p, values), "cache, n = %d" % n)
        assert B.LC_MATCH in got[1][[0, n - 1]] and B.LC_GAVE_UP in got[1][[0, 63]]


# ------------------------------------------------------------------------------------------------ subset and device-count launches
@pytest.mark.parametrize("status_fill", [PENDING_BYTE, STATUS_SENTINEL])
def test_listed_rows_and_a_device_count(torch_dev, status_fill):
    """d_lines lists every third row in descending order, *d_nlines holds fewer rows than the list: the listed rows up to the count
    equal the expectation (pending values among them), every other row -- unlisted, or listed beyond the count -- keeps what it held,
    a stale pending byte included (pass 2 looks only at the rows pass 1 took)."""
    p = bl.P(0)
    edge = bl.values_of(bl.edge_ks(bl.NCAPS))
    short = bl.values_of(bl.SHORT_KS)
    N = 3 * len(edge) + 12
    values = [short[i % len(short)] for i in range(N)]
    lines = list(range(N - 1, -1, -3))
    for j, v in enumerate(edge):           # the edge values on listed rows, from the front of the list
        values[lines[j]] = v
    values[1] = bl.V(bl.PENDING_K)         # ... and pending ones the launch must not touch: unlisted,
    values[lines[-1]] = bl.V(bl.PENDING_K)  # and listed beyond the count
    count = len(lines) - 3
    assert count >= len(edge) and 1 not in lines
    exp = bl.expected(p, values)
    got = launch(torch_dev, p, values, lines=lines, nlines=count, status_fill=status_fill)
    check(got, exp, "listed rows, fill %d" % status_fill, listed=lines[:count], status_fill=status_fill)
    got = launch(torch_dev, p, values, lines=lines, status_fill=status_fill)          # the whole list, no device count
    check(got, exp, "listed rows, no count, fill %d" % status_fill, listed=lines, status_fill=status_fill)
    got = launch(torch_dev, p, values, nlines=N - 5, status_fill=status_fill)         # a device count alone: the first N - 5 rows
    check(got, exp, "device count alone, fill %d" % status_fill, listed=list(range(N - 5)), status_fill=status_fill)


# ------------------------------------------------------------------------------------------------ resume
def test_a_resumed_search_goes_pending_and_resumes_from_the_same_offset(torch_dev):
    """The search form of P(0) (LC_SYNTAX_SEARCH: group 1 is the whole match) with d_from = 0, 1 and one past the match's start: pass 2
    re-walks a pending value from ITS offset -- the expectation is the reference's search from that offset."""
    p, flags = bl.P(0), B.LC_SYNTAX_SEARCH
    values = [bl.V(203), b"cc" + bl.V(203), bl.V(204), bl.V(230), bl.V(3), bl.N(3), b"c" + bl.V(2) + b"c", bl.V(1640), b"", b"a"]
    starts = [(bl.reference(p, s, True, 0) or [0])[0] for s in values]
    assert starts[1] == 2 and starts[6] == 1
    for name, frm in (("0", [0] * len(values)), ("1", [1] * len(values)), ("one past the start", [b + 1 for b in starts])):
        pending = [s for s, f in zip(values, frm) if bl.SLICE_WORDS < bl.min_words(p, s, flags, min(f, len(s))) <= bl.RETRY_SLICE_WORDS]
        assert len(pending) >= 3, name
        exp = bl.expected(p, values, flags=flags, frm=frm)
        assert {B.LC_MATCH, B.LC_NOMATCH, B.LC_GAVE_UP} == set(exp[1].tolist()), name
        for form in ("len", "sep"):
            check(launch(torch_dev, p, values, form, flags=flags, frm=frm), exp, "resumed from %s, %s form" % (name, form))
    with pytest.raises(RuntimeError, match="LC_SYNTAX_SEARCH"):      # (the full-match form of the same pattern has nothing to resume)
        launch(torch_dev, p, values, frm=[0] * len(values))


# ------------------------------------------------------------------------------------------------ programs walked from global memory
@pytest.mark.parametrize("which", ["largest staged", "first unstaged", "700"])
def test_programs_on_either_side_of_the_stage(torch_dev, which):
    """The largest P(m) whose program fits the 48 KiB stage, the next one (walked from global memory) and P(700): the same values, the
    caps shifted by the m loop registers (m = 700: k = 132 is the last value pass 1 decides, k = 1567 the first LC_GAVE_UP)."""
    staged = bl.largest_staged_m()
    m = {"largest staged": staged, "first unstaged": staged + 1, "700": 700}[which]
    p = bl.P(m)
    assert (4 * len(bl.compiled(p)[1]) <= bl.STAGE_BYTES) == (which == "largest staged")
    ks = bl.edge_ks(bl.NCAPS + m)
    values = bl.values_of(ks)
    exp = bl.expected(p, values)
    for form in ("len", "sep"):
        got = launch(torch_dev, p, values, form)
        check(got, exp, "m = %d, %s form" % (m, form))
    first_up = (bl.RETRY_SLICE_WORDS - 16 - bl.NCAPS - m) // 10 + 1
    assert row_of(values, got, bl.V(first_up - 1))[0] == B.LC_MATCH and row_of(values, got, bl.V(first_up))[0] == B.LC_GAVE_UP
    if m == 700:
        assert first_up == 1567 and row_of(values, got, bl.V(133)) == (B.LC_MATCH, [264, 265])


# ------------------------------------------------------------------------------------------------ the large-slice rule
@pytest.mark.parametrize("m", [bl.M_SMALL_SLICE_LAST, bl.M_SMALL_SLICE_LAST + 1, bl.M_LARGE_SLICE])
def test_the_large_slice_rule(torch_dev, m):
    """BT_NCAPS + BT_NLOOP = 1856 still takes the small slice (96 stack entries: V(17) in pass 1, V(18) in pass 2); one register more
    and every lane has the large slice from the start, with no second pass: a value that fills it is final -- LC_GAVE_UP, never the
    pending byte.  m = 1900: V(1446) matches, V(1447) and N(1448) give up."""
    p = bl.P(m)
    assert bl.takes_large_slice(bl.NCAPS, m) == (m > bl.M_SMALL_SLICE_LAST)
    ks = bl.edge_ks(bl.NCAPS + m)
    values = bl.values_of(ks)
    exp = bl.expected(p, values)
    assert {B.LC_MATCH, B.LC_NOMATCH, B.LC_GAVE_UP} == set(exp[1].tolist())
    got = launch(torch_dev, p, values)
    check(got, exp, "m = %d" % m)
    if m == bl.M_SMALL_SLICE_LAST:
        assert row_of(values, got, bl.V(17)) == (B.LC_MATCH, [32, 33]) and row_of(values, got, bl.V(18)) == (B.LC_MATCH, [34, 35])
    if m == bl.M_LARGE_SLICE:
        assert row_of(values, got, bl.V(1446)) == (B.LC_MATCH, [2890, 2891])
        assert row_of(values, got, bl.V(1447)) == (B.LC_GAVE_UP, [-1, -1]) and row_of(values, got, bl.N(1448)) == (B.LC_GAVE_UP, [-1, -1])
    # ... and in a batch of several blocks, whose first launch has the lanes of the retry pass
    many = [values[i % len(values)] for i in range(1088)]
    check(launch(torch_dev, p, many), bl.expected(p, many), "m = %d, 1088 values" % m)


# ------------------------------------------------------------------------------------------------ the refusal
def test_the_refusal_above_16384_words_of_registers(torch_dev):
    """R(q): (?:)* loops, four instructions each -- the family's own loop takes five, and 16 316 of them do not fit a program.
    BT_NCAPS + BT_NLOOP = 16 320: need = 16 384, accepted, 32 stack entries: V(1) .. V(4) and every N are decided, V(5), V(6) give up.
    One register more: LC_ERR_UNSUPPORTED on the host, before any launch -- no byte of status or captures is written."""
    values = bl.values_of([1, 2, 3, 4, 5, 6])
    p = bl.R(bl.Q_ACCEPTED_LAST)
    got = launch(torch_dev, p, values)
    check(got, bl.expected(p, values), "16 320 registers")
    assert [int(got[1][values.index(bl.V(k))]) for k in (1, 2, 4, 5, 6)] == [1, 1, 1, 3, 3] and row_of(values, got, bl.V(1)) == (B.LC_MATCH, [0, 1])
    caps, status = launch(torch_dev, bl.R(bl.Q_ACCEPTED_LAST + 1), values, refused=True)
    assert (status == STATUS_SENTINEL).all() and (caps == CAPS_SENTINEL).all()
    assert "scratch" in B.load().lc_last_error().decode()


# ------------------------------------------------------------------------------------------------ the budget at its edge
@pytest.mark.parametrize("k", bl.BUDGET_KS)
def test_the_budget_at_its_edge(torch_dev, monkeypatch, k):
    """V(50) is decided in pass 1, V(203) in pass 2: with LC_BT_BUDGET = the steps its walk takes the value is decided, with one step
    less it is LC_GAVE_UP.  V(203) spends steps in pass 1 before it fills its slice: were the budget not fresh in pass 2, it would give
    up at min_budget too."""
    p = bl.P(0)
    assert (bl.min_words(p, bl.V(k)) > bl.SLICE_WORDS) == (k == 203)
    b = bl.min_budget(p, bl.V(k), bl.RETRY_SLICE_WORDS)
    assert b == bl.min_budget(p, bl.V(k), 1 << 20) and 500 < b < 1 << 20
    if k == 203:     # (pass 1 fills its slice before the smaller budget runs out: the value reaches pass 2 either way)
        assert bl.host_walk(bl.compiled(p)[1], bl.V(k), bl.SLICE_WORDS, b - 1) == -2
    values = [bl.V(1), bl.N(2), bl.V(k), bl.N(3)]
    for budget, want in ((b, B.LC_MATCH), (b - 1, B.LC_GAVE_UP)):
        monkeypatch.setenv("LC_BT_BUDGET", str(budget))
        got = launch(torch_dev, p, values)
        check(got, bl.expected(p, values, budget=budget), "k = %d, budget %d" % (k, budget))
        assert int(got[1][2]) == want and got[1].tolist()[:2] == [B.LC_MATCH, B.LC_NOMATCH]


# ------------------------------------------------------------------------------------------------ one processor-level check
@pytest.mark.parametrize("m,parsed_k,gave_up_k", [(0, 203, 1637), (bl.M_LARGE_SLICE, 1446, 1447)])
def test_the_parse_processor_counts_a_value_that_fills_the_large_slice(torch_dev, m, parsed_k, gave_up_k):
    """processor_parse_regex_gpu with Regex P(m), a 1000-event group: the event whose value neither pass decides is a parse failure
    AND counted as complexity-exceeded (boost's exception); the one pass 2 decides is parsed.  Every other event: the processor oracle."""
    from loongcollector_amd.processor import EventGroup, Processor
    from oracle.processor_oracle import LogEventModel, ProcessorOracle
    cfg = {"SourceKey": "content", "Regex": bl.P(m).decode(), "Keys": ["g"], "KeepingSourceWhenParseFail": True,
           "KeepingSourceWhenParseSucceed": False, "CopingRawLog": False, "RenamedSourceKey": "rawLog"}
    short = bl.values_of(bl.SHORT_KS)
    lines = [short[i % len(short)] for i in range(1000)]
    lines[100], lines[640], lines[999] = bl.V(parsed_k), bl.V(gave_up_k), bl.N(5)
    assert bl.expected(bl.P(m), [lines[100], lines[640], lines[999]])[1].tolist() == [B.LC_MATCH, B.LC_GAVE_UP, B.LC_NOMATCH]
    p, po = Processor(cfg), ProcessorOracle(cfg)
    g = EventGroup({"events": [{"contents": {"content": s.decode()}, "timestamp": 1, "type": 1} for s in lines]})
    p.process(g)
    want = [[(a, b.decode()) for a, b in ev.live()] for ev in po.process_group([LogEventModel([("content", s)]) for s in lines])]
    assert want[100] == [("g", "a")] and len(want[999]) == 1 and want[999][0][1] == lines[999].decode()
    want[640] = [(want[999][0][0], lines[640].decode())]     # (the oracle backtracks without a bound: here it is a failure, source kept)
    assert g.contents() == want
    c = p.counters()
    assert c["complexity_exceeded_events_total"] == 1 and c["undecided_events_total"] == 0
    assert c["out_failed_events_total"] == po.counters["out_failed"] + 1 and c["in_events_total"] == 1000
