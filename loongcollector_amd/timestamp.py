"""ctypes binding of the timestamp parser (include/lc_timestamp.h): GpuStrptime is the engine (strptime_kernel over values in device or
host memory, also straight from a parser's capture table), TimestampProcessor the processor_parse_timestamp_gpu plugin over event groups
(same shape as processor.Processor).  There is no CPU path: every parse needs a HIP device and raises otherwise."""
import ctypes

import numpy as np

from . import binding
from .abi import CLOCK, LcTsOut  # noqa: F401
from .processor import PluginProcessor

LC_TS_OK, LC_TS_HAS_YEAR, LC_TS_DST, LC_TS_EPOCH, LC_TS_ABSENT = 1, 2, 4, 8, 0x80
LC_TS_MAX_PROGRAM = 64


def _lib():
    return binding.load()


class GpuStrptime:
    """The engine: a SourceFormat compiled once.  Raises ValueError for a format beyond the kernel's program window."""

    def __init__(self, fmt):
        self._L = _lib()
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(256)
        fmt = fmt.encode("latin-1") if isinstance(fmt, str) else bytes(fmt)
        rc = self._L.lc_strptime_create(fmt, ctypes.byref(h), err, 256)
        if rc != binding.LC_OK:
            raise ValueError(err.value.decode() or "lc_strptime_create rc=%d" % rc)
        self.handle = h

    def program(self):
        w = (ctypes.c_uint32 * LC_TS_MAX_PROGRAM)()
        return list(w)[:self._L.lc_strptime_program(self.handle, w)]

    @staticmethod
    def device_outputs(n, device):
        """-> dict of torch tensors for one call: status u8, secs i64, nanos i32 (the bits of a u32), matched i32, frac_len i32,
        same_as_prev u8"""
        import torch
        return {"status": torch.empty(n, dtype=torch.uint8, device=device), "secs": torch.empty(n, dtype=torch.int64, device=device),
                "nanos": torch.empty(n, dtype=torch.int32, device=device), "matched": torch.empty(n, dtype=torch.int32, device=device),
                "frac_len": torch.empty(n, dtype=torch.int32, device=device), "same_as_prev": torch.empty(n, dtype=torch.uint8, device=device)}

    @staticmethod
    def _out(t):
        return LcTsOut(*(t[k].data_ptr() for k in ("status", "secs", "nanos", "matched", "frac_len", "same_as_prev")))

    def parse_spans_device(self, d_data, d_off, d_spans, n, out, stream=None):
        """torch device tensors: d_data u8[], d_off i32/u32[>= n], d_spans i32[n, 2]; out: device_outputs(); asynchronous"""
        o = self._out(out)
        binding._check(self._L.lc_strptime_parse_spans_device(self.handle, d_data.data_ptr(), d_off.data_ptr(), d_spans.data_ptr(), n,
                                                              ctypes.byref(o), ctypes.c_void_p(stream or 0)), "lc_strptime_parse_spans_device")

    def parse_captures_device(self, d_data, d_off, d_caps, ngroups, group, d_line_status, match_value, n, out, stream=None):
        """the value is group `group` of a parser's capture table d_caps i32[n, 2 * ngroups], present where d_line_status == match_value"""
        o = self._out(out)
        binding._check(self._L.lc_strptime_parse_captures_device(
            self.handle, d_data.data_ptr(), d_off.data_ptr(), d_caps.data_ptr(), ngroups, group,
            d_line_status.data_ptr() if d_line_status is not None else None, match_value, n, ctypes.byref(o), ctypes.c_void_p(stream or 0)),
            "lc_strptime_parse_captures_device")

    def parse_host(self, values):
        """list of bytes -> dict of numpy arrays (one device trip)"""
        n = len(values)
        blob = np.frombuffer(b"".join(values) + b"\0", np.uint8)
        lens = np.array([len(v) for v in values], np.uint32)
        off = np.zeros(n, np.int64)
        if n > 1:
            off[1:] = np.cumsum(lens[:-1])
        ptrs = (blob.ctypes.data + off).astype(np.uint64)
        res = {"status": np.zeros(n, np.uint8), "secs": np.zeros(n, np.int64), "nanos": np.zeros(n, np.uint32),
               "matched": np.zeros(n, np.int32), "frac_len": np.zeros(n, np.int32), "same_as_prev": np.zeros(n, np.uint8)}
        o = LcTsOut(*(res[k].ctypes.data for k in ("status", "secs", "nanos", "matched", "frac_len", "same_as_prev")))
        binding._check(self._L.lc_strptime_parse_host(self.handle, ptrs.ctypes.data, lens.ctypes.data, n, ctypes.byref(o)), "lc_strptime_parse_host")
        return res

    def close(self):
        if getattr(self, "handle", None):
            self._L.lc_strptime_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ClockedProcessor(PluginProcessor):
    """a plugin created with a clock: a callable returning epoch seconds; default time().  Its counters carry history_failure_total."""

    def __init__(self, config, clock=None, lib=None):
        self._clock = CLOCK(lambda user: int(clock())) if clock is not None else None
        self._create(config, ctypes.cast(self._clock, ctypes.c_void_p) if self._clock else None, None, create="create_with_clock", lib=lib)

    def counters(self):
        d = PluginProcessor.counters(self)
        d["history_failure_total"] = int(self._call("history_failures", self._h))
        return d


class TimestampProcessor(_ClockedProcessor):
    """processor_parse_timestamp_gpu; same config keys as processor_parse_timestamp_native.  clock: "now" of the year deduction and of
    the discard rule.  collect_alarms(): kind 0 PARSE_TIME_FAIL_ALARM, kind 1 OUTDATED_LOG_ALARM."""
    PREFIX, PLUGIN = "lc_timestamp_processor", "processor_parse_timestamp_gpu"

    def set_discard(self, enabled=True, interval=43200, onetime=False):
        self._L.lc_timestamp_processor_set_discard(self._h, int(enabled), interval, int(onetime))
