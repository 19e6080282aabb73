"""ctypes binding of the field codecs (include/codec/lc_codec.h): apply_device / apply_host are the engine (base64 encode, base64 decode
and MD5 of values in device or host memory), Processor the Go plugins processor_base64_encoding, processor_base64_decoding and
processor_md5 over logs ([[key, value], ...] each), chosen by Op.  There is no CPU path: every call needs a HIP device and raises
otherwise."""
import ctypes
import json
import os

import numpy as np

from . import abi, binding

LC_CODEC_OUT, LC_CODEC_ERROR = 1, 2
LC_CODEC_ALARM_DECODE, LC_CODEC_ALARM_NO_KEY, LC_CODEC_ALARM_TRIP_FAILED = 1, 2, 3
COUNTERS = ("values", "out", "decode_errors", "no_key", "failed_trips")
OPS = ("base64_encode", "base64_decode", "md5")

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "liblc_codec.so")
_lib = None


def load():
    """liblc_codec.so, which stands beside liblc_regex_gpu.so and is linked against it (that one is loaded first: one HIP runtime)"""
    global _lib
    if _lib is None:
        binding.load()
        _lib = abi.bind(ctypes.CDLL(LIB_PATH), abi.CODEC_PROTOTYPES)
    return _lib


class CodecInitError(ValueError):
    """the create call's refusal; .code is its LC_ERR_* code"""

    def __init__(self, message, code):
        super().__init__(message)
        self.code = code


class Processor:
    """one of the three plugins with the Go struct's field names and the selector: Processor(Op="base64_decode", SourceKey="src",
    NewKey="dest", DecodeError=True).  collect_alarms(): the (kind, text) pairs heard since the last call, kinds LC_CODEC_ALARM_*.
    lib: another library that exports the lc_codec_* processor entries (the tests' host double)."""

    def __init__(self, lib=None, **config):
        L = self._L = lib or load()
        text = json.dumps(config, ensure_ascii=False).encode("utf-8")
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        rc = L.lc_codec_create(text, len(text), ctypes.byref(h), err, 512)
        if rc != 0:
            raise CodecInitError(err.value.decode("utf-8", "replace"), rc)
        self._h = h
        self.op = config["Op"]
        self._alarms = []
        self._sink = abi.ALARM_SINK(lambda user, kind, msg, n: self._alarms.append((kind, ctypes.string_at(msg, n))))
        L.lc_codec_set_alarm_sink(self._h, ctypes.cast(self._sink, ctypes.c_void_p), None)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_codec_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def process_logs(self, logs):
        """logs: [[(key, value), ...], ...] (str) -> the same shape; one device trip for the batch"""
        text = json.dumps([[list(kv) for kv in log] for log in logs], ensure_ascii=False).encode("utf-8")
        out = ctypes.c_void_p()
        rc = self._L.lc_codec_process_logs_json(self._h, text, len(text), ctypes.byref(out))
        if rc != 0:  # (every log counts as unchanged)
            if self._L is _lib:
                binding._check(rc, "lc_codec_process_logs_json")
            raise RuntimeError("lc_codec_process_logs_json failed: rc=%d" % rc)
        try:
            return [[tuple(kv) for kv in log] for log in json.loads(ctypes.string_at(out).decode("utf-8"))]
        finally:
            self._L.lc_codec_free_string(out)

    def apply(self, values):
        """values: list of bytes -> [(flags, output bytes or None, error offset or None)]; one device trip"""
        return apply_host(self, values)

    def counters(self):
        c = (ctypes.c_uint64 * len(COUNTERS))()
        binding._check(self._L.lc_codec_counters(self._h, c), "lc_codec_counters")
        return dict(zip(COUNTERS, (int(x) for x in c)))

    def collect_alarms(self):
        got, self._alarms = self._alarms, []
        return got


def _ptr(t):
    return t.data_ptr() if t is not None else None


def apply_device(proc, d_data, d_off, n, d_flags, d_err_off, d_out_off, d_out_len, d_out, out_cap, stream=0):
    """d_data uint8, d_off uint32/int32[n + 1], d_flags uint8[n], d_err_off uint32/int32[n] or None, d_out_off uint64/int64[n + 1],
    d_out_len uint32/int32[n], d_out uint8 (16-byte aligned) device tensors (d_out may be None with out_cap 0) -> (rc, needed).
    Synchronous on `stream`.  LC_ERR_OVERFLOW (6) and LC_ERR_ARG (5) come back as rc for the caller to act on, every other failure
    raises."""
    needed = ctypes.c_uint64(0)
    rc = load().lc_codec_apply_device(proc.handle, _ptr(d_data), _ptr(d_off), n, _ptr(d_flags), _ptr(d_err_off), _ptr(d_out_off), _ptr(d_out_len),
                                      _ptr(d_out), out_cap, ctypes.byref(needed), stream)
    if rc not in (0, 5, 6):
        binding._check(rc, "lc_codec_apply_device")
    return rc, int(needed.value)


def apply_host(proc, values):
    """values: list of bytes -> [(flags, output bytes or None, error offset or None)] through lc_codec_apply_host"""
    L = proc._L
    n = len(values)
    blob = np.frombuffer(b"".join(values) + b"\0", np.uint8).copy()
    lens = np.array([len(v) for v in values], np.uint32)
    off = np.zeros(n, np.uint64)
    if n:
        off[1:] = np.cumsum(lens[:-1])
    ptrs = (blob.ctypes.data + off).astype(np.uint64)
    flags = np.zeros(n, np.uint8)
    err_off = np.zeros(n, np.uint32)
    out_off = np.zeros(n + 1, np.uint64)
    out_len = np.zeros(n, np.uint32)
    out = ctypes.c_void_p()
    rc = L.lc_codec_apply_host(proc.handle, ptrs.ctypes.data, lens.ctypes.data, n, flags.ctypes.data, err_off.ctypes.data, out_off.ctypes.data,
                               out_len.ctypes.data, ctypes.byref(out))
    if rc != 0:
        if L is _lib:
            binding._check(rc, "lc_codec_apply_host")
        raise RuntimeError("lc_codec_apply_host failed: rc=%d" % rc)
    try:
        data = ctypes.string_at(out, int(out_off[n])) if out.value else b""
    finally:
        L.lc_codec_free_string(out)
    assert not (out_off % 16).any()
    return [(int(flags[i]), data[int(out_off[i]):int(out_off[i]) + int(out_len[i])] if flags[i] & LC_CODEC_OUT else None,
             int(err_off[i]) if flags[i] & LC_CODEC_ERROR else None) for i in range(n)]
