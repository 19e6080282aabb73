"""ctypes binding of the JSON-lines encoder (include/jsonl/lc_jsonl.h): Plan + encode_device / match_encode_host are the engine
(jsonl_size_kernel, the scan, jsonl_write_kernel over what lc_regex_match_device left behind), head the group's tags in front of every
record (host), Processor processor_parse_regex_native followed by the JSON serializer in one call.  There is no CPU path for the encode:
it needs a HIP device and raises otherwise."""
import ctypes
import json
import os

import numpy as np

from . import abi, binding
from .sls import PARSE_COUNTERS, _items, _strings

LC_JSONL_MAX_ITEMS, LC_JSONL_MAX_KEY_BYTES, LC_JSONL_MAX_HEAD_BYTES = 256, 65536, 65536
OWN_COUNTERS = ("groups_device", "groups_host", "failed_trips", "bytes")

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "liblc_jsonl.so")
_lib = None


def load():
    """liblc_jsonl.so, which stands beside liblc_regex_gpu.so and is linked against it (that one is loaded first: one HIP runtime)"""
    global _lib
    if _lib is None:
        binding.load()
        _lib = abi.bind(ctypes.CDLL(LIB_PATH), abi.JSONL_PROTOTYPES)
    return _lib


class JsonlPlanError(ValueError):
    pass


class Plan:
    """keys: the key table (bytes or str); matched / unmatched: [(key index, source), ...] with source 0 = the whole line, g >= 1 = capture
    group g.  lib: another library that exports lc_jsonl_plan_create / _free (the tests' host double)."""

    def __init__(self, keys, matched, unmatched=(), lib=None):
        L = self._L = lib or load()
        self._bufs, ptrs, lens = _strings(keys)
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(256)
        rc = L.lc_jsonl_plan_create(ptrs, lens, len(keys), _items(matched), len(matched), _items(unmatched), len(unmatched), ctypes.byref(h), err, 256)
        if rc != 0:
            raise JsonlPlanError("lc_jsonl_plan_create: rc=%d %s" % (rc, err.value.decode("utf-8", "replace")))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_jsonl_plan_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h


def head_rc(pairs, cap=None, lib=None):
    """pairs: [(tag key, tag value), ...] in any order -> (rc, the head's bytes or None, the bytes needed); cap: the room offered"""
    L = lib or load()
    kb, kp, kl = _strings([k for k, _ in pairs])
    vb, vp_, vl = _strings([v for _, v in pairs])
    need = ctypes.c_size_t()
    room = LC_JSONL_MAX_HEAD_BYTES if cap is None else cap
    buf = (ctypes.c_uint8 * max(1, room))()
    rc = L.lc_jsonl_head(kp, kl, vp_, vl, len(pairs), buf, room, ctypes.byref(need))
    return rc, (bytes(buf[:need.value]) if rc == 0 else None), need.value


def head(pairs=(), cap=None, lib=None):
    rc, data, need = head_rc(list(pairs), cap, lib)
    if rc != 0:
        raise ValueError("lc_jsonl_head: rc=%d, %d bytes needed" % (rc, need))
    return data


def scratch_bytes(plan, n):
    return load().lc_jsonl_scratch_bytes(plan.handle, n)


def encode_device_rc(plan, d_data, d_off, d_len, sep_bytes, n, ngroups, d_caps, d_status, d_time, d_head, head_len, d_out, out_cap, d_rec_off,
                     d_scratch, scratch_len, stream=0):
    """the entry's return code; every d_* is an address (int) or None"""
    return load().lc_jsonl_encode_device(plan.handle, d_data, d_off, d_len, sep_bytes, n, ngroups, d_caps, d_status, d_time, d_head, head_len, d_out,
                                         out_cap, d_rec_off, d_scratch, scratch_len, stream)


def encode_device(plan, d_data, d_off, d_len, sep_bytes, n, ngroups, d_caps, d_status, d_time, d_head, head_len, d_out, out_cap, d_rec_off,
                  d_scratch, stream=0):
    """device tensors (d_len, d_caps with ngroups 0 and d_out with out_cap 0 may be None).  Asynchronous on `stream`."""
    def ptr(t):
        return t.data_ptr() if t is not None else None
    binding._check(encode_device_rc(plan, ptr(d_data), ptr(d_off), ptr(d_len), sep_bytes, n, ngroups, ptr(d_caps), ptr(d_status), ptr(d_time),
                                    ptr(d_head), head_len, ptr(d_out), out_cap, ptr(d_rec_off), ptr(d_scratch),
                                    d_scratch.numel() * d_scratch.element_size(), stream), "lc_jsonl_encode_device")


def match_encode_host(plan, rx, lines, time, head_bytes, want_rec_off=True, lib=None):
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
    hb = np.frombuffer(head_bytes, np.uint8).copy()
    rec = np.zeros(n + 1, np.uint64) if want_rec_off else None
    status = np.zeros(max(1, n), np.uint8)
    out, out_len = ctypes.c_void_p(), ctypes.c_size_t()
    rc = L.lc_jsonl_match_encode_host(plan.handle, rx.handle if hasattr(rx, "handle") else rx, ptrs.ctypes.data, lens.ctypes.data, n, t.ctypes.data,
                                      hb.ctypes.data, len(head_bytes), ctypes.byref(out), ctypes.byref(out_len),
                                      rec.ctypes.data if rec is not None else None, status.ctypes.data)
    if rc != 0:
        binding._check(rc, "lc_jsonl_match_encode_host")
    return ctypes.string_at(out, out_len.value) if out_len.value else b"", rec, status[:n]


def serialize_group_host(group, lib=None):
    """group: an lc_event_group_t* -> the JSON lines of its log events as they are"""
    L = lib or load()
    out, out_len = ctypes.c_void_p(), ctypes.c_size_t()
    rc = L.lc_jsonl_serialize_group_host(group, ctypes.byref(out), ctypes.byref(out_len))
    if rc != 0:
        raise RuntimeError("lc_jsonl_serialize_group_host failed: rc=%d" % rc)
    return ctypes.string_at(out, out_len.value) if out_len.value else b""


class Processor:
    """processor_parse_regex_native's config -> serialize(group) = the JSON lines of what that processor would leave.  lib: another
    library that exports the lc_jsonl_processor_* entries (the tests' host double)."""

    def __init__(self, config, lib=None):
        L = self._L = lib or load()
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        rc = L.lc_jsonl_processor_create(json.dumps(config).encode("utf-8"), ctypes.byref(h), err, 512)
        if rc != 0:
            raise ValueError("lc_jsonl_processor_create: rc=%d %s" % (rc, err.value.decode("utf-8", "replace")))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_jsonl_processor_destroy(self._h)
            self._h = None

    def serialize_rc(self, group):
        """group: an lc_event_group_t* -> (rc, bytes or None, fused); the bytes are copied out of the thread's block"""
        out, out_len, fused = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
        rc = self._L.lc_jsonl_processor_serialize(self._h, group, ctypes.byref(out), ctypes.byref(out_len), ctypes.byref(fused))
        if rc != 0:
            return rc, None, 0
        return 0, (ctypes.string_at(out, out_len.value) if out_len.value else b""), fused.value

    def serialize(self, group):
        rc, data, fused = self.serialize_rc(group)
        if rc != 0:
            raise RuntimeError("lc_jsonl_processor_serialize failed: rc=%d" % rc)
        return data, fused

    def counters(self):
        parse = (ctypes.c_uint64 * 12)()
        own = (ctypes.c_uint64 * len(OWN_COUNTERS))()
        assert self._L.lc_jsonl_processor_counters(self._h, parse, own) == 0
        out = {k: int(parse[i]) for k, i in PARSE_COUNTERS.items()}
        out.update(zip(OWN_COUNTERS, (int(x) for x in own)))
        return out
