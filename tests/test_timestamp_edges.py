"""The timestamp parser's deterministic edge tables (tests/helpers/timestamp_edges.py) on a machine without a GPU: the product's PER-VALUE
ROUTINE (strptimeRun of csrc/strptime_vm.hpp compiled for the host) over the calendar table against BOTH references -- the model
(helpers/timestamp_model.strptime_ns) and Python's own calendar (datetime.date.toordinal), which shares no arithmetic with either --,
over every value of the 255-value border batches and over every truncation of the span-end values; and that the border batches are what
they say: the model and the rule give same_as_prev = 1 at the chosen pairs of the variants that share a prefix and nowhere else.
tests/test_gpu_timestamp_edges.py runs the same tables through strptime_kernel."""
import ctypes

import numpy as np
import pytest

from helpers import timestamp_edges as te
from helpers.timestamp_double import Format

SAME = {"equal": 1, "fraction_digits": 1, "fraction_length": 1, "last_byte": 0, "first_byte": 0, "predecessor_fails": 0, "predecessor_shorter": 0,
        "predecessor_absent_negative": 0, "predecessor_absent_reversed": 0, "value_absent": 0}


def test_calendar_table_equals_the_model_and_python_s_calendar():
    table = te.calendar_table()
    assert len(table) > 6300
    held = 0
    for fmt, rows in te.by_format(table).items():
        f = Format(fmt)
        for value, secs in rows:
            got = f.parse(value)
            status, want_secs, ns, matched, flen = te.model_row(fmt, value)
            assert got[0] == status and got[1] == want_secs and got[3:] == (matched, flen) and (ns is None or got[2] == ns), (fmt, value, got)
            if secs is not None:
                assert got[0] & te.LC_TS_OK and got[1] == secs and matched == len(value), (fmt, value, got, secs)
                held += 1
    assert held > 6240
    # the table is not flat: days beyond the month run on, the pivot of %y, a fraction from the buffer's 11th byte on
    f = Format(te.CALENDAR_FORMAT)
    assert f.parse(b"2100-02-29 23:59:60")[1] == f.parse(b"2100-03-02 00:00:00")[1] and f.parse(b"2000-02-29 00:00:00")[1] == 951782400
    assert (Format("%y%m%d").parse(b"680101")[1], Format("%y%m%d").parse(b"690101")[1]) == (3092601600, -31536000)
    assert Format("%s").parse(b"1700000000123456789")[1:] == (1700000000, 123456789, 19, 9)


@pytest.mark.parametrize("fmt", [te.FRACTION_FORMAT, te.YEARLESS_FORMAT])
def test_border_batches_are_what_they_say_and_the_routine_equals_the_model_on_them(fmt):
    f = Format(fmt)
    seen = set()
    for variant in te.VARIANTS:
        for borders in te.BORDER_SETS:
            for pad_front in range(4):
                batch = te.border_batch(fmt, variant, pad_front, borders)
                data, off, spans = batch.arrays()
                assert len(batch.values) == te.N_BORDER and len(data) % 16 == 0 and len(data) >= len(batch.blob) + 16
                want, _ = te.expected(fmt, batch.values)
                meant = SAME[variant] if fmt == te.FRACTION_FORMAT or not variant.startswith("fraction") else 1
                ones = set(np.nonzero(want["same_as_prev"])[0].tolist())
                assert ones == (set(borders) if meant else set()), (variant, borders, ones)
                for i in borders:      # what the variant is about
                    prev, cur = batch.values[i - 1], batch.values[i]
                    if variant == "value_absent":
                        assert cur is None and want["status"][i] == te.LC_TS_ABSENT and prev.startswith(batch.values[i + 1]) and want["status"][i - 1] & want["status"][i + 1] & 1
                    elif variant.startswith("predecessor_absent"):
                        assert prev is None and want["status"][i - 1] == te.LC_TS_ABSENT and want["status"][i] & 1
                    elif variant == "predecessor_fails":
                        assert not want["status"][i - 1] & 1 and want["status"][i] & 1 and len(prev) - len(cur) == (te.BORDERS.index(i) + pad_front) % 4
                    else:
                        assert want["status"][i - 1] & 1 and want["status"][i] & 1
                        lp, lc = (int(want["matched"][j] - want["frac_len"][j]) for j in (i - 1, i))
                        differ = [j for j in range(min(lp, lc)) if prev[j] != cur[j]]
                        assert (lp - lc, differ) == {"last_byte": (0, [lc - (2 if fmt == te.FRACTION_FORMAT else 1)]), "first_byte": (0, [0]),
                                                     "predecessor_shorter": (-1, differ)}.get(variant, (0, [])), (variant, prev, cur)
                    for j in (i - 1, i):   # both dword residues of both values occur over the launches
                        seen.add((j == i, int(off[j] + max(spans[j, 0], 0)) % 4))
                for v in {v for v in batch.values if v is not None}:
                    got = f.parse(v)
                    status, secs, ns, matched, flen = te.model_row(fmt, v)
                    assert got == (status, secs, ns, matched, flen), (fmt, v)
    assert seen == {(which, r) for which in (False, True) for r in range(4)}


@pytest.mark.parametrize("fmt,value", te.SPAN_END_VALUES, ids=[f for f, _ in te.SPAN_END_VALUES])
def test_routine_stops_at_the_span_end_of_every_truncation(fmt, value):
    """the full value lies in the buffer; the routine is told a shorter length: a read at i >= len would find the byte the match goes on with"""
    f = Format(fmt)
    buf = ctypes.create_string_buffer(value + b"0")
    assert f.parse(value)[0] & te.LC_TS_OK
    results = set()
    for k in range(len(value) + 1):
        st, secs, ns, m, fl = ctypes.c_uint8(), ctypes.c_int64(), ctypes.c_uint32(), ctypes.c_int32(), ctypes.c_int32()
        f.L.td_parse_one(f.h, buf, k, ctypes.byref(st), ctypes.byref(secs), ctypes.byref(ns), ctypes.byref(m), ctypes.byref(fl))
        status, want_secs, want_ns, matched, flen = te.model_row(fmt, value[:k])
        assert (st.value, secs.value, m.value, fl.value) == (status, want_secs, matched, flen) and (want_ns is None or ns.value == want_ns), (fmt, value[:k])
        results.add((st.value & 1, secs.value))
    assert len(results) > 4
