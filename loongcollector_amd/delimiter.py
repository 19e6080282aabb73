"""ctypes binding of the delimiter parser (include/lc_delimiter.h): GpuDelimiter is the engine (delim_split_kernel over lines in
device or host memory), DelimiterProcessor the processor_parse_delimiter_gpu plugin over event groups (same shape as
processor.Processor).  There is no CPU path: every split needs a HIP device and raises otherwise."""
import ctypes

import numpy as np

from . import binding
from .processor import PluginProcessor

LC_DELIM_FAIL, LC_DELIM_OK, LC_DELIM_BLANK = 0, 1, 2
LC_DELIM_EXTEND, LC_DELIM_KEEP, LC_DELIM_DISCARD = 0, 1, 2
LC_DELIM_DOUBLED = 0x80000000
MODES = {"extend": LC_DELIM_EXTEND, "keep": LC_DELIM_KEEP, "discard": LC_DELIM_DISCARD}


def _lib():
    return binding.load()


class GpuDelimiter:
    """The engine: separator (1..4 bytes), quote (one byte), OverflowedFieldsTreatment mode and the number of keys."""

    def __init__(self, separator, quote=b'"', mode="extend", n_keys=0):
        self._L = _lib()
        separator, quote = bytes(separator), bytes(quote)
        h = ctypes.c_void_p()
        rc = self._L.lc_delim_create(separator, len(separator), quote[0] if quote else 0x22, MODES[mode], n_keys, ctypes.byref(h))
        if rc != binding.LC_OK:
            raise ValueError("lc_delim_create rc=%d" % rc)
        self.handle = h

    @property
    def uses_quote(self):
        return bool(self._L.lc_delim_uses_quote(self.handle))

    def split_device(self, d_data, d_off, n, W, d_status, d_ncols, d_spans, stream=None):
        """torch device tensors: d_data u8[], d_off i32[n + 1], d_status u8[n], d_ncols i32[n], d_spans i32[n, W, 2]; asynchronous"""
        binding._check(self._L.lc_delim_split_device(self.handle, d_data.data_ptr(), d_off.data_ptr(), n, W, d_status.data_ptr(),
                                                     d_ncols.data_ptr(), d_spans.data_ptr() if W else None, ctypes.c_void_p(stream or 0)),
                       "lc_delim_split_device")

    def split_host(self, data, off, W):
        """numpy: data u8[], off[n + 1] -> (status u8[n], ncols u32[n], spans i32[n, W, 2]); the lines go up as views, one per line"""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.asarray(off, dtype=np.int64)
        n = len(off) - 1
        base = data.ctypes.data
        ptrs = (base + off[:-1]).astype(np.uint64)
        lens = (off[1:] - off[:-1]).astype(np.uint32)
        status = np.zeros(n, np.uint8)
        ncols = np.zeros(n, np.uint32)
        spans = np.full((n, W, 2), -1, np.int32)
        binding._check(self._L.lc_delim_split_host(self.handle, ptrs.ctypes.data, lens.ctypes.data, n, W, status.ctypes.data, ncols.ctypes.data,
                                                   spans.ctypes.data), "lc_delim_split_host")
        return status, ncols, spans

    def close(self):
        if getattr(self, "handle", None):
            self._L.lc_delim_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DelimiterProcessor(PluginProcessor):
    """processor_parse_delimiter_gpu; same config keys as processor_parse_delimiter_native.  collect_alarms(): every PARSE_LOG_FAIL_ALARM
    the reference would raise."""
    PREFIX, PLUGIN = "lc_delimiter_processor", "processor_parse_delimiter_gpu"

    def __init__(self, config, first_trip_columns=0, lib=None):
        self._create(config, lib=lib)
        if first_trip_columns:
            self._L.lc_delimiter_processor_set_first_trip_columns(self._h, first_trip_columns)
