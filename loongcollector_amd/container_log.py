"""ctypes binding of the container stdout parser (include/lc_container_log.h): parse_device / parse_host are the engine
(clog_containerd_kernel / clog_docker_kernel over lines in device or host memory), ContainerLogProcessor the
processor_parse_container_log_gpu plugin over event groups (same shape as processor.Processor).  There is no CPU path: every parse needs
a HIP device and raises otherwise."""
import ctypes

import numpy as np

from . import binding
from .abi import CLOG_OUT_KEYS as OUT_KEYS, LcClogOut  # noqa: F401
from .processor import EventGroup, PluginProcessor

LC_CLOG_CONTAINERD, LC_CLOG_DOCKER = 1, 2
LC_CLOG_OK, LC_CLOG_FAIL_TIME, LC_CLOG_FAIL_SOURCE, LC_CLOG_FAIL_STREAM, LC_CLOG_FAIL_JSON = 0, 1, 2, 3, 4
LC_CLOG_STDERR, LC_CLOG_PARTIAL, LC_CLOG_ESCAPED, LC_CLOG_REPLAY = 1, 2, 4, 8
LC_CLOG_SPAN_TIME, LC_CLOG_SPAN_SOURCE, LC_CLOG_SPAN_CONTENT = 0, 1, 2


def _lib():
    return binding.load()


def set_group_format(group: EventGroup, fmt):
    """the group's LOG_FORMAT metadata: LC_CLOG_CONTAINERD / LC_CLOG_DOCKER (or any text)"""
    binding._check(_lib().lc_group_set_metadata(group._h, b"container.type", str(fmt).encode()), "lc_group_set_metadata")


def parse_device(fmt, d_data, d_off, n, d_out, d_shadow=None, stream=0):
    """d_data uint8, d_off int32[n + 1], d_out: dict of device tensors under OUT_KEYS (status / flags u8[n], spans i32[n, 3, 2],
    rewrite_begin i32[n]); d_shadow uint8, as long as d_data (Docker).  Asynchronous on `stream`."""
    o = LcClogOut(*(d_out[k].data_ptr() for k in OUT_KEYS))
    binding._check(_lib().lc_container_log_parse_device(fmt, d_data.data_ptr(), d_off.data_ptr(), n, ctypes.byref(o),
                                                        d_shadow.data_ptr() if d_shadow is not None else None, stream),
                   "lc_container_log_parse_device")


def parse_host(fmt, lines, fill=None):
    """lines: list of bytes -> dict of numpy arrays under OUT_KEYS plus "shadow" (uint8, sum of the lengths; fill: the byte every array
    holds beforehand) and "moved" (how many shadow bytes came back from the device)"""
    n = len(lines)
    blob = np.frombuffer(b"".join(lines) + b"\0", np.uint8).copy()
    lens = np.array([len(v) for v in lines], np.uint32)
    off = np.zeros(n, np.uint64)
    if n:
        off[1:] = np.cumsum(lens[:-1])
    ptrs = (blob.ctypes.data + off).astype(np.uint64)
    shapes = {"status": ((n,), np.uint8), "flags": ((n,), np.uint8), "spans": ((n, 3, 2), np.int32), "rewrite_begin": ((n,), np.int32),
              "shadow": ((len(blob),), np.uint8)}
    res = {k: np.zeros(s, t) for k, (s, t) in shapes.items()}
    if fill is not None:
        for v in res.values():
            v.view(np.uint8)[...] = fill & 0xFF
    o = LcClogOut(*(res[k].ctypes.data for k in OUT_KEYS))
    moved = ctypes.c_uint64(0)
    binding._check(_lib().lc_container_log_parse_host(fmt, ptrs.ctypes.data, lens.ctypes.data, n, ctypes.byref(o), res["shadow"].ctypes.data,
                                                      ctypes.byref(moved)), "lc_container_log_parse_host")
    res["shadow"] = res["shadow"][:-1]
    res["moved"] = int(moved.value)
    return res


class ContainerLogProcessor(PluginProcessor):
    """processor_parse_container_log_gpu; same config keys as processor_parse_container_log_native.  The format of a group is its
    LOG_FORMAT metadata (set_group_format).  collect_alarms(): kind 0 PARSE_LOG_FAIL_ALARM, kind 3 a failed trip."""
    PREFIX, PLUGIN = "lc_container_log_processor", "processor_parse_container_log_gpu"

    def __init__(self, config, config_name="", lib=None):
        self._create(config, lib=lib)
        self._L.lc_container_log_processor_set_config_name(self._h, config_name.encode("utf-8"))

    def counters(self):
        d = PluginProcessor.counters(self)
        s = (ctypes.c_uint64 * 2)()
        self._L.lc_container_log_processor_stream_counts(self._h, s)
        d["parse_stdout_total"], d["parse_stderr_total"] = int(s[0]), int(s[1])
        return d

    def replayed_lines(self):
        return int(self._L.lc_container_log_processor_replayed_lines(self._h))
