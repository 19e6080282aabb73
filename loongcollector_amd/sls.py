"""ctypes binding of the SLS encoder (include/sls/lc_sls.h): Plan + encode_device / match_encode_host are the engine (sls_size_kernel, the
scan, sls_write_kernel over what lc_regex_match_device left behind), append_tags the group's tags (host), Processor
processor_parse_regex_native followed by the SLS serializer in one call.  There is no CPU path for the encode: it needs a HIP device and
raises otherwise."""
import ctypes
import json
import os

import numpy as np

from . import abi, binding

LC_SLS_MAX_ITEMS, LC_SLS_MAX_KEY_BYTES = 256, 65536
OWN_COUNTERS = ("groups_device", "groups_host", "failed_trips", "bytes")
PARSE_COUNTERS = {"discarded": 0, "out_failed": 1, "out_key_not_found": 2, "out_successful": 3, "complexity_exceeded": 9, "undecided": 10,
                  "device_failed": 11}

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "liblc_sls.so")
_lib = None


def load():
    """liblc_sls.so, which stands beside liblc_regex_gpu.so and is linked against it (that one is loaded first: one HIP runtime)"""
    global _lib
    if _lib is None:
        binding.load()
        _lib = abi.bind(ctypes.CDLL(LIB_PATH), abi.SLS_PROTOTYPES)
    return _lib


class SlsPlanError(ValueError):
    pass


def _strings(values):
    values = [v if isinstance(v, bytes) else v.encode("utf-8") for v in values]
    # (addresses, not c_char_p: a value may hold NUL bytes)
    bufs = [ctypes.create_string_buffer(v, len(v) + 1) for v in values]
    ptrs = (ctypes.c_char_p * max(1, len(values)))(*[ctypes.cast(b, ctypes.c_char_p) for b in bufs])
    lens = (ctypes.c_uint32 * max(1, len(values)))(*[len(v) for v in values])
    return bufs, ptrs, lens


def _items(items):
    flat = [x for item in items for x in item]
    return (ctypes.c_uint32 * max(1, len(flat)))(*flat)


class Plan:
    """keys: the key table (bytes or str); matched / unmatched: [(key index, source), ...] with source 0 = the whole line, g >= 1 = capture
    group g.  lib: another library that exports lc_sls_plan_create / _free (the tests' host double)."""

    def __init__(self, keys, matched, unmatched=(), lib=None):
        L = self._L = lib or load()
        self._bufs, ptrs, lens = _strings(keys)
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(256)
        rc = L.lc_sls_plan_create(ptrs, lens, len(keys), _items(matched), len(matched), _items(unmatched), len(unmatched), ctypes.byref(h), err, 256)
        if rc != 0:
            raise SlsPlanError("lc_sls_plan_create: rc=%d %s" % (rc, err.value.decode("utf-8", "replace")))
        self._h = h
        self.rc = rc

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_sls_plan_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h


def scratch_bytes(n):
    return load().lc_sls_scratch_bytes(n)


def encode_device_rc(plan, d_data, d_off, d_len, sep_bytes, n, ngroups, d_caps, d_status, d_time, d_time_ns, enable_ns, d_out, out_cap, d_rec_off,
                     d_scratch, scratch_len, stream=0):
    """the entry's return code; every d_* is an address (int) or None"""
    return load().lc_sls_encode_device(plan.handle, d_data, d_off, d_len, sep_bytes, n, ngroups, d_caps, d_status, d_time, d_time_ns, enable_ns, d_out,
                                       out_cap, d_rec_off, d_scratch, scratch_len, stream)


def encode_device(plan, d_data, d_off, d_len, sep_bytes, n, ngroups, d_caps, d_status, d_time, d_time_ns, enable_ns, d_out, out_cap, d_rec_off,
                  d_scratch, stream=0):
    """device tensors (d_len, d_time_ns, d_caps with ngroups 0 and d_out with out_cap 0 may be None).  Asynchronous on `stream`."""
    def ptr(t):
        return t.data_ptr() if t is not None else None
    binding._check(encode_device_rc(plan, ptr(d_data), ptr(d_off), ptr(d_len), sep_bytes, n, ngroups, ptr(d_caps), ptr(d_status), ptr(d_time),
                                    ptr(d_time_ns), enable_ns, ptr(d_out), out_cap, ptr(d_rec_off), ptr(d_scratch),
                                    d_scratch.numel() * d_scratch.element_size(), stream), "lc_sls_encode_device")


def match_encode_host(plan, rx, lines, time, time_ns=None, enable_ns=0, want_rec_off=True, lib=None):
    """lines: list of bytes; rx: binding.GpuRegex -> (the records' bytes, rec_off uint64[n + 1] or None, status uint8[n])"""
    L = lib or load()
    n = len(lines)
    blob = np.frombuffer(b"".join(lines) + b"\0", np.uint8).copy()
    lens = np.array([len(v) for v in lines], np.uint32)
    off = np.zeros(n, np.uint64)
    if n:
        off[1:] = np.cumsum(lens[:-1])
    ptrs = (blob.ctypes.data + off).astype(np.uint64)
    t = np.ascontiguousarray(time, np.uint32)
    ns = np.ascontiguousarray(time_ns, np.int32) if time_ns is not None else None
    rec = np.zeros(n + 1, np.uint64) if want_rec_off else None
    status = np.zeros(max(1, n), np.uint8)
    out, out_len = ctypes.c_void_p(), ctypes.c_size_t()
    rc = L.lc_sls_match_encode_host(plan.handle, rx.handle if hasattr(rx, "handle") else rx, ptrs.ctypes.data, lens.ctypes.data, n, t.ctypes.data,
                                    ns.ctypes.data if ns is not None else None, enable_ns, ctypes.byref(out), ctypes.byref(out_len),
                                    rec.ctypes.data if rec is not None else None, status.ctypes.data)
    if rc != 0:
        binding._check(rc, "lc_sls_match_encode_host")
    return ctypes.string_at(out, out_len.value) if out_len.value else b"", rec, status[:n]


def append_tags(pairs, cap=None, lib=None):
    """pairs: [(key, value), ...] in the order to write -> the bytes behind the records; cap: the room offered (default: what is needed)"""
    L = lib or load()
    kb, kp, kl = _strings([k for k, _ in pairs])
    vb, vp_, vl = _strings([v for _, v in pairs])
    need = ctypes.c_size_t()
    rc = L.lc_sls_append_tags(kp, kl, vp_, vl, len(pairs), None, 0, ctypes.byref(need))
    if need.value == 0:
        return b""
    room = need.value if cap is None else cap
    buf = (ctypes.c_uint8 * max(1, room))()
    rc = L.lc_sls_append_tags(kp, kl, vp_, vl, len(pairs), buf, room, ctypes.byref(need))
    if rc != 0:
        raise OverflowError("lc_sls_append_tags: rc=%d, %d bytes needed" % (rc, need.value))
    return bytes(buf[:need.value])


class Processor:
    """processor_parse_regex_native's config -> serialize(group) = the SLS wire bytes of what that processor would leave.  lib: another
    library that exports the lc_sls_processor_* entries (the tests' host double)."""

    def __init__(self, config, lib=None):
        L = self._L = lib or load()
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        rc = L.lc_sls_processor_create(json.dumps(config).encode("utf-8"), ctypes.byref(h), err, 512)
        if rc != 0:
            raise ValueError("lc_sls_processor_create: rc=%d %s" % (rc, err.value.decode("utf-8", "replace")))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_sls_processor_destroy(self._h)
            self._h = None

    def serialize_rc(self, group, enable_ns=0):
        """group: an lc_event_group_t* -> (rc, bytes or None, fused); the bytes are copied out of the thread's block"""
        out, out_len, fused = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
        rc = self._L.lc_sls_processor_serialize(self._h, group, enable_ns, ctypes.byref(out), ctypes.byref(out_len), ctypes.byref(fused))
        if rc != 0:
            return rc, None, 0
        return 0, (ctypes.string_at(out, out_len.value) if out_len.value else b""), fused.value

    def serialize(self, group, enable_ns=0):
        rc, data, fused = self.serialize_rc(group, enable_ns)
        if rc != 0:
            raise RuntimeError("lc_sls_processor_serialize failed: rc=%d" % rc)
        return data, fused

    def counters(self):
        parse = (ctypes.c_uint64 * 12)()
        own = (ctypes.c_uint64 * len(OWN_COUNTERS))()
        assert self._L.lc_sls_processor_counters(self._h, parse, own) == 0
        out = {k: int(parse[i]) for k, i in PARSE_COUNTERS.items()}
        out.update(zip(OWN_COUNTERS, (int(x) for x in own)))
        return out
