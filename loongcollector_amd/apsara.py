"""ctypes binding of the Apsara log parser (include/lc_apsara.h): parse_device / parse_host are the engine (apsara_parse_kernel over
lines in device or host memory), ApsaraProcessor the processor_parse_apsara_gpu plugin over event groups (same shape as
processor.Processor).  There is no CPU path: every parse needs a HIP device and raises otherwise."""
import ctypes

import numpy as np

from . import binding
from .abi import APSARA_OUT_KEYS as OUT_KEYS, LcApsaraOut  # noqa: F401
from .timestamp import _ClockedProcessor

LC_APSARA_TIME_OK, LC_APSARA_EPOCH, LC_APSARA_CANON19 = 1, 2, 4
LC_APSARA_LEVEL, LC_APSARA_THREAD, LC_APSARA_FILE, LC_APSARA_LINE = 0, 1, 2, 3


def _lib():
    return binding.load()


def parse_device(d_data, d_off, n, W, d_out, stream=0):
    """d_data uint8, d_off int32[n + 1], d_out: dict of device tensors under OUT_KEYS (status u8[n], secs i64[n], nanos / npairs
    i32[n] read as u32, base i32[n, 4, 2], pairs i32[n, W, 3]).  Asynchronous on `stream`."""
    o = LcApsaraOut(*(d_out[k].data_ptr() for k in OUT_KEYS))
    binding._check(_lib().lc_apsara_parse_device(d_data.data_ptr(), d_off.data_ptr(), n, W, ctypes.byref(o), stream), "lc_apsara_parse_device")


def parse_host(lines, W, fill=None):
    """lines: list of bytes -> dict of numpy arrays under OUT_KEYS (pairs: int32[n, W, 3]; fill: the byte the arrays hold beforehand)"""
    n = len(lines)
    blob = np.frombuffer(b"".join(lines) + b"\0", np.uint8).copy()
    lens = np.array([len(v) for v in lines], np.uint32)
    off = np.zeros(n, np.uint64)
    if n:
        off[1:] = np.cumsum(lens[:-1])
    ptrs = (blob.ctypes.data + off).astype(np.uint64)
    shapes = {"status": ((n,), np.uint8), "secs": ((n,), np.int64), "nanos": ((n,), np.uint32), "base": ((n, 4, 2), np.int32),
              "npairs": ((n,), np.uint32), "pairs": ((n, max(W, 1), 3), np.int32)}
    res = {k: np.zeros(s, t) for k, (s, t) in shapes.items()}
    if fill is not None:
        for v in res.values():
            v.view(np.uint8)[...] = fill & 0xFF
    o = LcApsaraOut(*(res[k].ctypes.data for k in OUT_KEYS))
    binding._check(_lib().lc_apsara_parse_host(ptrs.ctypes.data, lens.ctypes.data, n, W, ctypes.byref(o)), "lc_apsara_parse_host")
    return res


class ApsaraProcessor(_ClockedProcessor):
    """processor_parse_apsara_gpu; same config keys as processor_parse_apsara_native.  clock: "now" of Timezone and of the discard rule.
    collect_alarms(): kind 0 PARSE_TIME_FAIL_ALARM, kind 1 OUTDATED_LOG_ALARM, kind 3 a failed trip."""
    PREFIX, PLUGIN = "lc_apsara_processor", "processor_parse_apsara_gpu"

    def set_discard(self, enabled=True, interval=43200):
        self._L.lc_apsara_processor_set_discard(self._h, int(enabled), interval)

    def replayed_lines(self):
        s = (ctypes.c_uint64 * 2)()
        self._L.lc_apsara_processor_replayed_lines(self._h, s)
        return int(s[0]), int(s[1])
