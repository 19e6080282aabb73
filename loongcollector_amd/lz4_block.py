"""ctypes binding of the LZ4 block writer (include/lz4/lc_lz4.h): Lz4 holds a chunk size; compress_device / compress_host are the engine
(lz4_match_kernel, the scans, lz4_size_kernel, lz4_emit_kernel), match_encode_compress_host the agent's trip: lines up, the regex match,
the SLS records, the tags, one block down.  There is no CPU path: it needs a HIP device and raises otherwise.  (Not lz4.py: that name
is the PyPI module's.)"""
import ctypes
import os

import numpy as np

from . import abi, binding, sls

LC_LZ4_MAX_SEGMENT = 0x7E000000
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "liblc_lz4.so")
_lib = None


def load():
    """liblc_lz4.so, which stands beside liblc_regex_gpu.so and liblc_sls.so and is linked against both (loaded first: one HIP runtime)"""
    global _lib
    if _lib is None:
        sls.load()
        _lib = abi.bind(ctypes.CDLL(LIB_PATH), abi.LZ4_PROTOTYPES)
    return _lib


def bound(n):
    return load().lc_lz4_bound(n)


class Lz4:
    """chunk_bytes: a multiple of 64 from 64 to 65536; 0 = the library's default"""

    def __init__(self, chunk_bytes=0):
        L = self._L = load()
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(256)
        rc = L.lc_lz4_create(chunk_bytes, ctypes.byref(h), err, 256)
        if rc != 0:
            raise ValueError("lc_lz4_create: rc=%d %s" % (rc, err.value.decode("utf-8", "replace")))
        self._h = h
        self.chunk_bytes = L.lc_lz4_chunk_bytes(h)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.lc_lz4_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def scratch_bytes(self, total_in, n_seg):
        return self._L.lc_lz4_scratch_bytes(self._h, total_in, n_seg)

    def compress_device_rc(self, d_in, d_seg_begin, d_seg_len, n_seg, d_out, out_cap, d_out_off, d_scratch, scratch_len, stream=0):
        """the entry's return code; every d_* is an address (int) or None"""
        return self._L.lc_lz4_compress_device(self._h, d_in, d_seg_begin, d_seg_len, n_seg, d_out, out_cap, d_out_off, d_scratch, scratch_len, stream)

    def compress_device(self, d_in, d_seg_begin, d_seg_len, n_seg, d_out, out_cap, d_out_off, d_scratch, stream=0):
        """device tensors (d_out with out_cap 0 may be None).  Asynchronous on `stream`."""
        def ptr(t):
            return t.data_ptr() if t is not None else None
        binding._check(self.compress_device_rc(ptr(d_in), ptr(d_seg_begin), ptr(d_seg_len), n_seg, ptr(d_out), out_cap, ptr(d_out_off), ptr(d_scratch),
                                               d_scratch.numel() * d_scratch.element_size() if d_scratch is not None else 0, stream),
                       "lc_lz4_compress_device")

    def compress_host_view(self, segs):
        """segs: list of bytes -> (address of the blocks, out_off uint64[n + 1]); the view is valid until the thread's next lc_lz4_* call"""
        n = len(segs)
        bufs = [np.frombuffer(s, np.uint8) if len(s) else np.zeros(1, np.uint8) for s in segs]
        ptrs = np.array([b.ctypes.data for b in bufs] or [0], np.uint64)
        lens = np.array([len(s) for s in segs] or [0], np.uint32)
        off = np.zeros(n + 1, np.uint64)
        out = ctypes.c_void_p()
        rc = self._L.lc_lz4_compress_host(self._h, ptrs.ctypes.data, lens.ctypes.data, n, ctypes.byref(out), off.ctypes.data)
        if rc != 0:
            binding._check(rc, "lc_lz4_compress_host")
        return out.value, off

    def compress_host(self, segs):
        """segs: list of bytes -> the list of their blocks"""
        at, off = self.compress_host_view(segs)
        return [ctypes.string_at(at + int(off[s]), int(off[s + 1] - off[s])) for s in range(len(segs))]

    def match_encode_compress_host(self, plan, rx, lines, time, time_ns=None, enable_ns=0, tags=b"", want_rec_off=True):
        """lines: list of bytes; rx: binding.GpuRegex; tags: the bytes of sls.append_tags
        -> (the block, raw_len, rec_off uint64[n + 1] or None, status uint8[n])"""
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
        tag_buf = np.frombuffer(tags, np.uint8) if tags else None
        out, out_len, raw_len = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()
        rc = self._L.lc_lz4_match_encode_compress_host(
            self._h, plan.handle, rx.handle if hasattr(rx, "handle") else rx, ptrs.ctypes.data, lens.ctypes.data, n, t.ctypes.data,
            ns.ctypes.data if ns is not None else None, enable_ns, tag_buf.ctypes.data if tag_buf is not None else None, len(tags),
            ctypes.byref(out), ctypes.byref(out_len), ctypes.byref(raw_len), rec.ctypes.data if rec is not None else None, status.ctypes.data)
        if rc != 0:
            binding._check(rc, "lc_lz4_match_encode_compress_host")
        return ctypes.string_at(out, out_len.value), raw_len.value, rec, status[:n]


def thread_release():
    load().lc_lz4_thread_release()
