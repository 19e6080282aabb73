"""ctypes binding of the anchor processor (include/anchor/lc_anchor.h): locate_device / locate_host are the engine (anchor_locate_kernel over
values in device or host memory), Processor the Go plugin processor_anchor over logs ([[key, value], ...] each).  There is no CPU path:
every search needs a HIP device and raises otherwise."""
import ctypes
import json
import os

import numpy as np

from . import abi, binding

LC_ANCHOR_NO_START, LC_ANCHOR_NO_STOP = -1, -2
LC_ANCHOR_MAX_ANCHORS, LC_ANCHOR_MAX_NEEDLE = 16, 32
(LC_ANCHOR_ALARM_NO_KEY, LC_ANCHOR_ALARM_NO_START, LC_ANCHOR_ALARM_NO_STOP, LC_ANCHOR_ALARM_TRIP_FAILED) = range(1, 5)
COUNTERS = ("values", "fields", "no_start", "no_stop", "no_source_key", "failed_trips", "pairs_per_log")


LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "liblc_anchor.so")
_lib = None


def load():
    """liblc_anchor.so, which stands beside liblc_regex_gpu.so and is linked against it (that one is loaded first: one HIP runtime)"""
    global _lib
    if _lib is None:
        binding.load()
        _lib = abi.bind(ctypes.CDLL(LIB_PATH), abi.ANCHOR_PROTOTYPES)
    return _lib


class AnchorInitError(ValueError):
    pass


class Processor:
    """processor_anchor with the Go struct's field names: Processor(Anchors=[{"Start": "time:", "Stop": "\\t", "FieldName": "time"}],
    SourceKey="content", KeepSource=False, NoKeyError=True, NoAnchorError=True).  collect_alarms(): the (kind, text) pairs heard since
    the last call, kinds LC_ANCHOR_ALARM_*.  lib: another library that exports the lc_anchor_* processor entries (the tests' host double)."""

    def __init__(self, lib=None, **config):
        L = self._L = lib or load()
        text = json.dumps(config, ensure_ascii=False).encode("utf-8")
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        if L.lc_anchor_create(text, len(text), ctypes.byref(h), err, 512) != 0:
            raise AnchorInitError(err.value.decode("utf-8", "replace"))
        self._h = h
        self._alarms = []
        self._sink = abi.ALARM_SINK(lambda user, kind, msg, n: self._alarms.append((kind, ctypes.string_at(msg, n))))
        L.lc_anchor_set_alarm_sink(self._h, ctypes.cast(self._sink, ctypes.c_void_p), None)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_anchor_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @property
    def stride(self):
        """entries per row of the span arrays: the anchor count rounded up to an even number"""
        return int(self._L.lc_anchor_stride(self._h))

    def process_logs(self, logs):
        """logs: [[(key, value), ...], ...] (str) -> the same shape; one device trip for the batch"""
        text = json.dumps([[list(kv) for kv in log] for log in logs], ensure_ascii=False).encode("utf-8")
        out = ctypes.c_void_p()
        rc = self._L.lc_anchor_process_logs_json(self._h, text, len(text), ctypes.byref(out))
        if rc != 0:  # (every log counts as unchanged)
            if self._L is _lib:
                binding._check(rc, "lc_anchor_process_logs_json")
            raise RuntimeError("lc_anchor_process_logs_json failed: rc=%d" % rc)
        try:
            return [[tuple(kv) for kv in log] for log in json.loads(ctypes.string_at(out).decode("utf-8"))]
        finally:
            self._L.lc_anchor_free_string(out)

    def counters(self):
        c = (ctypes.c_uint64 * len(COUNTERS))()
        binding._check(self._L.lc_anchor_counters(self._h, c), "lc_anchor_counters")
        return dict(zip(COUNTERS, (int(x) for x in c)))

    def collect_alarms(self):
        got, self._alarms = self._alarms, []
        return got


def locate_device(proc, d_data, d_off, n, d_spans, stream=0):
    """d_data uint8, d_off int32[n + 1], d_spans int32[n][proc.stride][2] device tensors (16-byte aligned).  Asynchronous on `stream`."""
    binding._check(load().lc_anchor_locate_device(proc.handle, d_data.data_ptr(), d_off.data_ptr(), n, d_spans.data_ptr(), stream),
                   "lc_anchor_locate_device")


def locate_host(proc, values, fill=None):
    """values: list of bytes -> int32 numpy array [n][proc.stride][2] (fill: the byte the array holds beforehand)"""
    n = len(values)
    blob = np.frombuffer(b"".join(values) + b"\0", np.uint8).copy()
    lens = np.array([len(v) for v in values], np.uint32)
    off = np.zeros(n, np.uint64)
    if n:
        off[1:] = np.cumsum(lens[:-1])
    ptrs = (blob.ctypes.data + off).astype(np.uint64)
    spans = np.zeros((n, proc.stride, 2), np.int32)
    if fill is not None:
        spans.view(np.uint8)[...] = fill & 0xFF
    binding._check(load().lc_anchor_locate_host(proc.handle, ptrs.ctypes.data, lens.ctypes.data, n, spans.ctypes.data), "lc_anchor_locate_host")
    return spans
