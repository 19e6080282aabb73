"""ctypes binding of the CSV decoder (include/csv/lc_csv.h): read_device / read_host are the engine (csv_split_kernel over values in device
or host memory), Processor the Go plugin processor_csv over logs ([[key, value], ...] each).  There is no CPU path: every read needs a
HIP device and raises otherwise."""
import ctypes
import json
import os

import numpy as np

from . import abi, binding

LC_CSV_OK, LC_CSV_EOF, LC_CSV_BARE_QUOTE, LC_CSV_QUOTE = 0, 1, 2, 3
LC_CSV_FOLD = 0x80000000
LC_CSV_PRESERVE_EXTRA = 16
(LC_CSV_ALARM_NO_SOURCE_KEY, LC_CSV_ALARM_DECODE, LC_CSV_ALARM_KEY_COUNT, LC_CSV_ALARM_TRIP_FAILED) = range(1, 5)
COUNTERS = ("values", "fields", "decode_errors", "eof_values", "key_count", "no_source_key", "mop_up", "failed_trips")


LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "liblc_csv.so")
_lib = None


def load():
    """liblc_csv.so, which stands beside liblc_regex_gpu.so and is linked against it (that one is loaded first: one HIP runtime)"""
    global _lib
    if _lib is None:
        binding.load()
        _lib = abi.bind(ctypes.CDLL(LIB_PATH), abi.CSV_PROTOTYPES)
    return _lib


class CsvInitError(ValueError):
    pass


def out_shapes(n, W):
    """-> {key: (shape, dtype)} of the result arrays for n values at W fields per value"""
    return {"status": ((n,), np.uint8), "count": ((n,), np.uint32), "fields": ((n, W, 2), np.int32)}


def fold(raw):
    """the text of a field whose span has LC_CSV_FOLD, from the bytes between its quotes"""
    return raw.replace(b'""', b'"').replace(b"\r\n", b"\n")


def field_texts(value, rows, count):
    """the first `count` rows of one value -> the fields' texts"""
    out = []
    for b, e in rows[:count].tolist():
        out.append(fold(value[b & 0x7FFFFFFF:e]) if b < 0 else value[b:e])
    return out


class Processor:
    """processor_csv with the Go struct's field names: Processor(SplitKeys=["a", "b"], SplitSep=",", PreserveOthers=True, ...).
    collect_alarms(): the (kind, text) pairs heard since the last call, kinds LC_CSV_ALARM_*.  lib: another library that exports the
    lc_csv_* processor entries (the tests' host double)."""

    def __init__(self, lib=None, **config):
        L = self._L = lib or load()
        text = json.dumps(config, ensure_ascii=False).encode("utf-8")
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        if L.lc_csv_create(text, len(text), ctypes.byref(h), err, 512) != 0:
            raise CsvInitError(err.value.decode("utf-8", "replace"))
        self._h = h
        self._alarms = []
        self._sink = abi.ALARM_SINK(lambda user, kind, msg, n: self._alarms.append((kind, ctypes.string_at(msg, n))))
        L.lc_csv_set_alarm_sink(self._h, ctypes.cast(self._sink, ctypes.c_void_p), None)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_csv_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def process_logs(self, logs):
        """logs: [[(key, value), ...], ...] (str) -> the same shape; one device trip for the batch (and one mop-up trip)"""
        text = json.dumps([[list(kv) for kv in log] for log in logs], ensure_ascii=False).encode("utf-8")
        out = ctypes.c_void_p()
        rc = self._L.lc_csv_process_logs_json(self._h, text, len(text), ctypes.byref(out))
        if rc != 0:  # (every log counts as unchanged)
            if self._L is _lib:
                binding._check(rc, "lc_csv_process_logs_json")
            raise RuntimeError("lc_csv_process_logs_json failed: rc=%d" % rc)
        try:
            return [[tuple(kv) for kv in log] for log in json.loads(ctypes.string_at(out).decode("utf-8"))]
        finally:
            self._L.lc_csv_free_string(out)

    def counters(self):
        c = (ctypes.c_uint64 * len(COUNTERS))()
        binding._check(self._L.lc_csv_counters(self._h, c), "lc_csv_counters")
        return dict(zip(COUNTERS, (int(x) for x in c)))

    def collect_alarms(self):
        got, self._alarms = self._alarms, []
        return got

    def set_first_trip_fields(self, W):
        self._L.lc_csv_set_first_trip_fields(self._h, W)


def read_device(proc, d_data, d_off, n, W, d_status, d_count, d_fields, stream=0):
    """d_data uint8, d_off int32[n + 1], results as out_shapes(n, W) device tensors (d_fields None with W = 0).  Asynchronous on `stream`."""
    binding._check(load().lc_csv_device(proc.handle, d_data.data_ptr(), d_off.data_ptr(), n, W, d_status.data_ptr(), d_count.data_ptr(),
                                        d_fields.data_ptr() if d_fields is not None else None, stream), "lc_csv_device")


def read_host(proc, values, W, fill=None):
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
    binding._check(load().lc_csv_host(proc.handle, ptrs.ctypes.data, lens.ctypes.data, n, W, res["status"].ctypes.data, res["count"].ctypes.data,
                                      res["fields"].ctypes.data if W else None), "lc_csv_host")
    return res
