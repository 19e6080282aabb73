"""ctypes binding of the multiline splitter (include/lc_multiline.h); plumbing for tests and tools."""
import ctypes
import json

from . import binding
from .abi import LcMlRecord as _Record


class MultilineInitError(ValueError):
    pass


class Multiline:
    def __init__(self, **config):
        L = self._L = binding.load()
        text = json.dumps(config).encode("utf-8")
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        if L.lc_multiline_create(text, len(text), ctypes.byref(h), err, 512) != 0:
            raise MultilineInitError(err.value.decode("utf-8", "replace"))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_multiline_free(self._h)
            self._h = None

    @property
    def is_multiline(self):
        return bool(self._L.lc_multiline_is_multiline(self._h))

    @property
    def warnings(self):
        return self._L.lc_multiline_warnings(self._h).decode("utf-8", "replace")

    @property
    def patterns(self):
        m = self._L.lc_multiline_patterns(self._h)
        return {"start": bool(m & 1), "continue": bool(m & 2), "end": bool(m & 4)}

    def split(self, value: bytes):
        """-> (records [(begin, length, matched)], (input lines, unmatched lines, matched logs))"""
        recs = ctypes.POINTER(_Record)()
        n = ctypes.c_uint32()
        counters = (ctypes.c_uint32 * 3)()
        rc = self._L.lc_multiline_split_host(self._h, value, len(value), ctypes.byref(recs), ctypes.byref(n), counters)
        binding._check(rc, "lc_multiline_split_host")
        try:
            return [(recs[i].begin, recs[i].length, recs[i].matched & 1) for i in range(n.value)], tuple(counters)
        finally:
            self._L.lc_multiline_free_records(recs)


    def split_count(self, value: bytes):
        """the same call without building Python objects for the records (throughput measurements: the list of tuples costs more
        than the device trip) -> (number of records, counters)"""
        recs = ctypes.POINTER(_Record)()
        n = ctypes.c_uint32()
        counters = (ctypes.c_uint32 * 3)()
        rc = self._L.lc_multiline_split_host(self._h, value, len(value), ctypes.byref(recs), ctypes.byref(n), counters)
        binding._check(rc, "lc_multiline_split_host")
        self._L.lc_multiline_free_records(recs)
        return n.value, tuple(counters)

    def split_raw(self, value: bytes):
        """-> records [(begin, length, flag word)] with the LC_ML_LAST / LC_ML_RUN bits"""
        recs = ctypes.POINTER(_Record)()
        n = ctypes.c_uint32()
        counters = (ctypes.c_uint32 * 3)()
        rc = self._L.lc_multiline_split_host(self._h, value, len(value), ctypes.byref(recs), ctypes.byref(n), counters)
        binding._check(rc, "lc_multiline_split_host")
        try:
            return [(recs[i].begin, recs[i].length, recs[i].matched) for i in range(n.value)]
        finally:
            self._L.lc_multiline_free_records(recs)

    def process(self, group):
        """ProcessorSplitMultilineLogStringNative::Process on an EventGroup (loongcollector_amd.processor.EventGroup)."""
        from .processor import _lib
        binding._check(self._L.lc_multiline_process_group(self._h, _lib().lc_group_native(group._h)), "lc_multiline_process_group")

    def counters(self):
        """-> (matched lines, unmatched lines, matched events)"""
        c = (ctypes.c_uint64 * 3)()
        self._L.lc_multiline_counters(self._h, c)
        return tuple(int(x) for x in c)


class MergeMultiline:
    """processor_merge_multiline_log_native (MergeType "regex" or "flag") on event groups."""

    def __init__(self, **config):
        Multiline.__new__(Multiline)  # (binds the library's prototypes once)
        try:
            Multiline(StartPattern="x")
        except Exception:
            pass
        L = self._L = binding.load()
        text = json.dumps(config).encode("utf-8")
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        if L.lc_merge_multiline_create(text, len(text), ctypes.byref(h), err, 512) != 0:
            raise MultilineInitError(err.value.decode("utf-8", "replace"))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_merge_multiline_free(self._h)
            self._h = None

    def process(self, group):
        from .processor import _lib
        binding._check(self._L.lc_merge_multiline_process_group(self._h, _lib().lc_group_native(group._h)),
                       "lc_merge_multiline_process_group")

    def patterns(self):
        """bit 0 start, bit 1 continue, bit 2 end: the patterns the processor matches with -- MultilineOptions' own regexes (a trailing
        '$' and ".*"s stripped, ContinuePattern dropped when all three are given), not the splitter's reading; 0 in flag mode"""
        return int(self._L.lc_merge_multiline_patterns(self._h))

    def warnings(self):
        return self._L.lc_merge_multiline_warnings(self._h).decode("utf-8", "replace")

    def counters(self):
        """-> (merged events, unmatched events)"""
        c = (ctypes.c_uint64 * 2)()
        self._L.lc_merge_multiline_counters(self._h, c)
        return tuple(int(x) for x in c)


ML_HAS_START, ML_HAS_CONT, ML_HAS_END, ML_DISCARD, ML_FLUSH = 1, 2, 4, 8, 16
ML_LAST, ML_RUN = 0x80000000, 2


def bounds_device(mode, d_start, d_cont, d_end, d_nitems, max_items, d_off, nbytes, d_flags, records, record_cap, counts, stream=None,
                  check=True):
    """lc_multiline_bounds_device on torch tensors: three uint8 status tensors, the uint32 item count, the line table and the flag
    scratch on the device; `records` ((cap, 3) 32-bit words) on the device or in pinned host memory; `counts` (8 words) on the device.
    Any of them may be None (a NULL pointer).  Asynchronous on `stream`.  -> the status code (check=False: not raised)"""
    L = binding.load()
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = L.lc_multiline_bounds_device(mode, ptr(d_start), ptr(d_cont), ptr(d_end), ptr(d_nitems), max_items, ptr(d_off), nbytes,
                                      ptr(d_flags), ptr(records), record_cap, ptr(counts), stream)
    if check:
        binding._check(rc, "lc_multiline_bounds_device")
    return rc


def bounds_model(mode, flags, off=None, nbytes=0, raw=False):
    """lc_multiline_bounds_model: the device scan's code run on the host, slice by slice.  flags: one byte per item (bit 0 start,
    bit 1 continue, bit 2 end matched); off: the offsets[n+1] + separator table (byte records) or None (item records).
    -> (records [(begin, length, flags)], counts[8]); raw=True: both as uint32 arrays ((records, 3) and (8,))"""
    import numpy as np
    L = binding.load()
    fl = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8))
    n = int(fl.size)
    cap = n + 2
    recs = np.zeros((cap, 3), dtype=np.uint32)
    counts = np.zeros(8, dtype=np.uint32)
    o = None if off is None else np.ascontiguousarray(np.asarray(off, dtype=np.uint32))
    rc = L.lc_multiline_bounds_model(mode, fl.ctypes.data if n else None, n, None if o is None else o.ctypes.data, nbytes,
                                     recs.ctypes.data, cap, counts.ctypes.data)
    binding._check(rc, "lc_multiline_bounds_model")
    if raw:
        return recs[:int(counts[3])], counts
    return [tuple(int(x) for x in r) for r in recs[:int(counts[3])]], [int(x) for x in counts]
