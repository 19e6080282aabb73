"""ctypes binding of the key-value splitter (include/kvsplit/lc_kvsplit.h): split_device / split_host are the engine (kv_split_kernel over values
in device or host memory), Processor the Go plugin processor_split_key_value over logs ([[key, value], ...] each).  There is no CPU
path: every split needs a HIP device and raises otherwise."""
import ctypes
import json
import os

import numpy as np

from . import abi, binding

LC_KV_OK, LC_KV_REF_PANIC = 0, 1
LC_KV_NO_SEPARATOR, LC_KV_EMPTY_KEY = -1, -2
LC_KV_MAX_NEEDLE, LC_KV_DEFAULT_PAIRS = 32, 16
(LC_KV_ALARM_NO_SOURCE_KEY, LC_KV_ALARM_NO_SEPARATOR, LC_KV_ALARM_EMPTY_KEY, LC_KV_ALARM_REF_PANIC, LC_KV_ALARM_TRIP_FAILED) = range(1, 6)
COUNTERS = ("values", "pairs", "no_separator", "empty_keys", "no_source_key", "ref_panic", "mop_up", "failed_trips")


LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "liblc_kvsplit.so")
_lib = None


def load():
    """liblc_kvsplit.so, which stands beside liblc_regex_gpu.so and is linked against it (that one is loaded first: one HIP runtime)"""
    global _lib
    if _lib is None:
        binding.load()
        _lib = abi.bind(ctypes.CDLL(LIB_PATH), abi.KVSPLIT_PROTOTYPES)
    return _lib


class KvSplitInitError(ValueError):
    pass


def out_shapes(n, W):
    """-> {key: (shape, dtype)} of the result arrays for n values at W pairs per value"""
    return {"status": ((n,), np.uint8), "npairs": ((n,), np.uint32), "pairs": ((n, W, 4), np.int32)}


class Processor:
    """processor_split_key_value with the Go struct's field names: Processor(Delimiter=" ", Separator="=", Quote='"', KeepSource=False, ...).
    collect_alarms(): the (kind, text) pairs heard since the last call, kinds LC_KV_ALARM_*.  lib: another library that exports the
    lc_kvsplit_* processor entries (the tests' host double)."""

    def __init__(self, lib=None, **config):
        L = self._L = lib or load()
        text = json.dumps(config, ensure_ascii=False).encode("utf-8")
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        if L.lc_kvsplit_create(text, len(text), ctypes.byref(h), err, 512) != 0:
            raise KvSplitInitError(err.value.decode("utf-8", "replace"))
        self._h = h
        self._alarms = []
        self._sink = abi.ALARM_SINK(lambda user, kind, msg, n: self._alarms.append((kind, ctypes.string_at(msg, n))))
        L.lc_kvsplit_set_alarm_sink(self._h, ctypes.cast(self._sink, ctypes.c_void_p), None)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_kvsplit_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def process_logs(self, logs):
        """logs: [[(key, value), ...], ...] (str) -> the same shape; one device trip for the batch (and one mop-up trip)"""
        text = json.dumps([[list(kv) for kv in log] for log in logs], ensure_ascii=False).encode("utf-8")
        out = ctypes.c_void_p()
        rc = self._L.lc_kvsplit_process_logs_json(self._h, text, len(text), ctypes.byref(out))
        if rc != 0:  # (every log counts as unchanged)
            if self._L is _lib:
                binding._check(rc, "lc_kvsplit_process_logs_json")
            raise RuntimeError("lc_kvsplit_process_logs_json failed: rc=%d" % rc)
        try:
            return [[tuple(kv) for kv in log] for log in json.loads(ctypes.string_at(out).decode("utf-8"))]
        finally:
            self._L.lc_kvsplit_free_string(out)

    def counters(self):
        c = (ctypes.c_uint64 * len(COUNTERS))()
        binding._check(self._L.lc_kvsplit_counters(self._h, c), "lc_kvsplit_counters")
        return dict(zip(COUNTERS, (int(x) for x in c)))

    def collect_alarms(self):
        got, self._alarms = self._alarms, []
        return got

    def set_first_trip_pairs(self, W):
        self._L.lc_kvsplit_set_first_trip_pairs(self._h, W)


def split_device(proc, d_data, d_off, n, W, d_status, d_npairs, d_pairs, stream=0):
    """d_data uint8, d_off int32[n + 1], results as out_shapes(n, W) device tensors (d_pairs None with W = 0).  Asynchronous on `stream`."""
    binding._check(load().lc_kvsplit_device(proc.handle, d_data.data_ptr(), d_off.data_ptr(), n, W, d_status.data_ptr(), d_npairs.data_ptr(),
                                                    d_pairs.data_ptr() if d_pairs is not None else None, stream), "lc_kvsplit_device")


def split_host(proc, values, W=LC_KV_DEFAULT_PAIRS, fill=None):
    """values: list of bytes -> dict of numpy arrays (out_shapes; fill: the byte every array holds beforehand)"""
    n = len(values)
    blob = np.frombuffer(b"".join(values) + b"\0", np.uint8).copy()
    lens = np.array([len(v) for v in values], np.uint32)
    off = np.zeros(n, np.uint64)
    if n:
        off[1:] = np.cumsum(lens[:-1])
    ptrs = (blob.ctypes.data + off).astype(np.uint64)
    res = {k: np.zeros(s, t) for k, (s, t) in out_shapes(n, W).items()}
    if fill is not None:
        for v in res.values():
            v.view(np.uint8)[...] = fill & 0xFF
    binding._check(load().lc_kvsplit_host(proc.handle, ptrs.ctypes.data, lens.ctypes.data, n, W, res["status"].ctypes.data, res["npairs"].ctypes.data,
                                                  res["pairs"].ctypes.data if W else None), "lc_kvsplit_host")
    return res
