"""strptime_kernel (csrc/strptime_kernel.hpp) at its edges, through the tables of tests/helpers/timestamp_edges.py: the calendar table
against the model AND Python's own calendar; the workgroup of 255 new values whose lane 0 parses the value before them again -- chosen
pairs on both sides of values 255 and 510, in every relation same_as_prev tells apart, at all four dword residues of both values --
through the spans entry and the captures entry (stride, column, line status, absent values); and the span end, with the byte the match
would go on with right behind every truncated value.  All six result arrays of every launch are compared, bit for bit, with
helpers/timestamp_model.strptime_ns and the rule of include/lc_timestamp.h; nothing is compared with the routine compiled for the host."""
import numpy as np
import pytest

from helpers import timestamp_edges as te

pytestmark = pytest.mark.gpu
TAIL = 8       # result entries behind the n values, painted and looked at again


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def run(torch, t, batch, ngroups=None, group=0, line_status=None):
    """one launch over the batch: the spans entry, or (ngroups given) the captures entry with match_value = 1 -> the six arrays"""
    dev = torch.device("cuda:0")
    n = len(batch.values)
    data, off, spans = batch.arrays(ngroups or 1, group)
    d_data, d_off, d_spans = (torch.from_numpy(a).to(dev) for a in (data, off, spans))
    out = {k: torch.full((n + TAIL,), 0x5A, dtype=v.dtype, device=dev) for k, v in t.device_outputs(1, dev).items()}
    stream = torch.cuda.current_stream().cuda_stream
    if ngroups is None:
        t.parse_spans_device(d_data, d_off, d_spans, n, out, stream=stream)
    else:
        d_line = torch.from_numpy(line_status).to(dev) if line_status is not None else None
        t.parse_captures_device(d_data, d_off, d_spans, ngroups, group, d_line, 1, n, out, stream=stream)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in te.KEYS}
    for k in te.KEYS:
        assert (res[k][n:] == 0x5A).all(), "%s: entries behind the %d values were written" % (k, n)
    return {k: res[k][:n] for k in te.KEYS}


def test_calendar_table_on_the_device_against_the_model_and_python_s_calendar():
    from loongcollector_amd import binding, timestamp
    torch = _torch()
    binding.launched_kernels()
    held = 0
    for fmt, rows in te.by_format(te.calendar_table()).items():
        batch = te.Batch(pad_front=3)
        for value, _ in rows:
            batch.add(value)
        res = run(torch, timestamp.GpuStrptime(fmt), batch)
        te.compare(res, fmt, batch.values, "calendar table, " + fmt)
        civil = np.array([-1 if secs is None else secs for _, secs in rows], np.int64)
        have = np.array([secs is not None for _, secs in rows])
        assert (res["status"][have] & te.LC_TS_OK).all() and np.array_equal(res["secs"][have], civil[have]), fmt
        held += int(have.sum())
    assert held > 6240 and "strptime_kernel" in binding.launched_kernels()


@pytest.mark.parametrize("variant", te.VARIANTS)
@pytest.mark.parametrize("fmt", [te.FRACTION_FORMAT, te.YEARLESS_FORMAT], ids=["fraction", "yearless"])
def test_same_as_prev_on_both_sides_of_a_workgroup_s_255_new_values(fmt, variant):
    """600 values, the chosen pairs (i - 1, i) around values 255 and 510 -- the first new values of workgroups 1 and 2, whose
    predecessors lane 0 parses again -- in `variant`; every launch at another residue of the values' first bytes"""
    from loongcollector_amd import timestamp
    torch = _torch()
    t = timestamp.GpuStrptime(fmt)
    for borders in te.BORDER_SETS:
        for pad_front in range(4):
            batch = te.border_batch(fmt, variant, pad_front, borders)
            te.compare(run(torch, t, batch), fmt, batch.values, "%s at %r, pad_front %d" % (variant, borders, pad_front))


@pytest.mark.parametrize("ngroups,group", [(1, 0), (3, 0), (3, 2)])
def test_the_captures_entry_stride_column_line_status_and_absent_values(ngroups, group):
    """the value is one group of a capture table whose other groups hold junk; a value exists where the line's status byte is 1 (bytes
    0, 2 and 3 take it away, also from the predecessors of the border pairs); line offsets with a separator byte between the lines"""
    from loongcollector_amd import binding, timestamp
    torch = _torch()
    fmt = te.FRACTION_FORMAT
    t = timestamp.GpuStrptime(fmt)
    cases = [("equal", None), ("predecessor_absent_negative", "line"), ("predecessor_absent_reversed", "reversed"), ("value_absent", "line"),
             ("fraction_length", None), ("first_byte", None)]
    for turn, (variant, absent_kind) in enumerate(cases):
        for borders in te.BORDER_SETS:
            pad_front = (turn + len(borders) + group) % 4
            batch = te.border_batch(fmt, variant, pad_front, borders, absent_kind=absent_kind, sprinkle=True, before=b"GET /x [", after=b"] 200\n")
            n = len(batch.values)
            # a line without a value has status 0, 2 or 3 -- unless its SPAN says so already, then the line may have matched
            line_status = np.ones(n, np.uint8)
            gone = [i for i, v in enumerate(batch.values) if v is None and batch.spans[i][0] >= 0 and batch.spans[i][1] >= batch.spans[i][0]]
            line_status[gone] = np.array([(0, 2, 3)[j % 3] for j in range(len(gone))], np.uint8)
            assert len(gone) > 50 and {0, 1, 2, 3} == set(line_status.tolist())
            res = run(torch, t, batch, ngroups, group, line_status)
            te.compare(res, fmt, batch.values, "captures (%d, %d), %s at %r" % (ngroups, group, variant, borders))
            if variant == "equal":
                assert res["same_as_prev"][list(borders)].all()
    # no line status: every good span is a value
    batch = te.border_batch(fmt, "equal", 1, te.BORDER_SETS[1], before=b"[", after=b"]\n")
    te.compare(run(torch, t, batch, ngroups, group, None), fmt, batch.values, "captures without a line status")
    dev = torch.device("cuda:0")
    d_data, d_off, d_spans = (torch.from_numpy(a).to(dev) for a in batch.arrays(ngroups, 0))
    out = t.device_outputs(len(batch.values), dev)
    for beyond in (ngroups, ngroups + 1):
        with pytest.raises(RuntimeError) as e:
            t.parse_captures_device(d_data, d_off, d_spans, ngroups, beyond, None, 1, len(batch.values), out)
        assert "rc=%d " % binding.LC_ERR_ARG in str(e.value)


@pytest.mark.parametrize("fmt,value", te.SPAN_END_VALUES, ids=[f for f, _ in te.SPAN_END_VALUES])
def test_the_walk_stops_at_the_span_end_of_every_truncation(fmt, value):
    """the dword source fetches whole dwords: bytes behind the span are in the register, and a read at i >= len would change the answer"""
    from loongcollector_amd import timestamp
    torch = _torch()
    t = timestamp.GpuStrptime(fmt)
    for pad_front in range(4):
        batch = te.span_end_batch(value, pad_front)
        res = run(torch, t, batch)
        te.compare(res, fmt, batch.values, "truncations at pad_front %d" % pad_front)
        assert res["status"][0] & te.LC_TS_OK and len({(int(s) & 1, int(x)) for s, x in zip(res["status"], res["secs"])}) > 4
