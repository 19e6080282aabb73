"""ctypes binding of the JSON parser (include/lc_json.h): GpuJson is the engine (json_walk_kernel over lines in device or host memory),
JsonProcessor the processor_parse_json_gpu plugin over event groups (same shape as processor.Processor).  There is no CPU path: every
walk needs a HIP device and raises otherwise."""
import ctypes

import numpy as np

from . import binding
from .processor import PluginProcessor

LC_JSON_FAIL, LC_JSON_OK, LC_JSON_EMPTY, LC_JSON_DEEP = 0, 1, 2, 3
LC_JSON_STRING, LC_JSON_INT, LC_JSON_DOUBLE, LC_JSON_TRUE, LC_JSON_FALSE, LC_JSON_NULL, LC_JSON_OBJECT, LC_JSON_ARRAY = range(8)
LC_JSON_ESCAPED = 0x80000000
# lc_json_member_t
MEMBER = np.dtype([("kb", "<u4"), ("ke", "<u4"), ("vb", "<u4"), ("ve", "<u4"), ("type", "u1"), ("reserved", "u1", (3,))])


def _lib():
    return binding.load()


class GpuJson:
    """The engine; it has no configuration."""

    def __init__(self):
        self._L = _lib()

    def walk_device(self, d_data, d_off, n, W, d_status, d_nmembers, d_errpos, d_records, d_shadow, stream=None):
        """torch device tensors: d_data u8[], d_off i32[n + 1], d_status u8[n], d_nmembers i32[n], d_errpos i32[n], d_records u8[n, W, 20]
        (lc_json_member_t), d_shadow u8[len(d_data)]; asynchronous"""
        binding._check(self._L.lc_json_walk_device(d_data.data_ptr(), d_off.data_ptr(), n, W, d_status.data_ptr(), d_nmembers.data_ptr(),
                                                   d_errpos.data_ptr(), d_records.data_ptr() if W else None, d_shadow.data_ptr(),
                                                   ctypes.c_void_p(stream or 0)), "lc_json_walk_device")

    def walk_host(self, data, off, W):
        """numpy: data u8[], off[n + 1] -> (status u8[n], nmembers u32[n], errpos u32[n], records MEMBER[n, W], shadow u8[like data],
        the number of unescaped bytes that came back from the device); the lines go up as views, one per line"""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.asarray(off, dtype=np.int64)
        n = len(off) - 1
        assert n == 0 or off[0] == 0        # (the shadow comes back packed like the lines)
        ptrs = (data.ctypes.data + off[:-1]).astype(np.uint64)
        lens = (off[1:] - off[:-1]).astype(np.uint32)
        status = np.zeros(n, np.uint8)
        nmembers = np.zeros(n, np.uint32)
        errpos = np.zeros(n, np.uint32)
        records = np.zeros((n, W), MEMBER)
        shadow = np.zeros(max(len(data), 1), np.uint8)
        moved = ctypes.c_uint64(0)
        binding._check(self._L.lc_json_walk_host(ptrs.ctypes.data, lens.ctypes.data, n, W, status.ctypes.data, nmembers.ctypes.data,
                                                 errpos.ctypes.data, records.ctypes.data, shadow.ctypes.data, ctypes.byref(moved)),
                       "lc_json_walk_host")
        return status, nmembers, errpos, records, shadow, int(moved.value)


class JsonProcessor(PluginProcessor):
    """processor_parse_json_gpu; same config keys as processor_parse_json_native.  collect_alarms(): every PARSE_LOG_FAIL_ALARM the
    reference would raise."""
    PREFIX, PLUGIN = "lc_json_processor", "processor_parse_json_gpu"

    def __init__(self, config, first_trip_members=0, lib=None):
        self._create(config, lib=lib)
        if first_trip_members:
            self._L.lc_json_processor_set_first_trip_members(self._h, first_trip_members)
