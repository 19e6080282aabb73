"""ctypes binding of the desensitize processor (include/lc_desensitize.h): GpuDesensitize is the engine (the match kernels in rounds,
desens_collect_kernel, desens_size_kernel, desens_write_kernel over values in device or host memory), DesensitizeProcessor the
processor_desensitize_gpu plugin over event groups (same shape as processor.Processor).  There is no CPU path: every apply needs a HIP
device and raises otherwise."""
import ctypes

import numpy as np

from . import binding
from .abi import LcDesensStats  # noqa: F401
from .processor import PluginProcessor

LC_DESENS_CONST, LC_DESENS_MD5 = 0, 1
LC_DESENS_CHANGED, LC_DESENS_GAVE_UP = 1, 2
LC_ERR_OVERFLOW = 6


class DesensitizeOverflow(RuntimeError):
    """the output did not fit (or would pass 2^32 - 1 bytes); .needed is the size the call reported"""

    def __init__(self, needed):
        RuntimeError.__init__(self, "desensitize: the output needs %d bytes" % needed)
        self.needed = needed


def _lib():
    return binding.load()


def _bytes(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


class GpuDesensitize:
    """lc_desens_*: method "const" | "md5"; before / content: the two halves of the pattern; replacing: ReplacingString (const)"""

    def __init__(self, method, before, content, replacing=b"", replacing_all=False, lib=None):
        self._L = lib or _lib()
        before, content, replacing = _bytes(before), _bytes(content), _bytes(replacing)
        h, warning = ctypes.c_void_p(), ctypes.c_int(0)
        err = ctypes.create_string_buffer(512)
        rc = self._L.lc_desens_create({"const": LC_DESENS_CONST, "md5": LC_DESENS_MD5}[method], before, len(before), content, len(content),
                                      replacing, len(replacing), 1 if replacing_all else 0, ctypes.byref(h), ctypes.byref(warning), err, 512)
        if rc != binding.LC_OK:
            raise ValueError(err.value.decode("utf-8", "replace"))
        self._h = h
        self.pass_through = bool(warning.value)

    def info(self):
        """lc_regex_info of the compiled search"""
        out = binding.LcRegexInfo()
        binding._check(self._L.lc_regex_info(self._L.lc_desens_regex(self._h), ctypes.byref(out)), "lc_regex_info")
        return {k: getattr(out, k) for k, _ in binding.LcRegexInfo._fields_}

    def apply_device(self, d_data, d_off, d_len, n, d_flags, d_out_off, d_out, stream=0):
        """d_data uint8, d_off uint32 / int32 [n] (with d_len) or [n + 1] (d_len None), d_flags uint8[n], d_out_off int64[n + 1],
        d_out uint8 (or None: size query).  -> (needed, stats dict); raises DesensitizeOverflow when d_out is too small."""
        needed = ctypes.c_uint64(0)
        stats = LcDesensStats()
        rc = self._L.lc_desens_apply_device(self._h, d_data.data_ptr(), d_off.data_ptr(), d_len.data_ptr() if d_len is not None else None, n,
                                            d_flags.data_ptr(), d_out_off.data_ptr(), d_out.data_ptr() if d_out is not None else None,
                                            d_out.numel() if d_out is not None else 0, ctypes.byref(needed), ctypes.byref(stats), stream)
        if rc == LC_ERR_OVERFLOW:
            raise DesensitizeOverflow(int(needed.value))
        binding._check(rc, "lc_desens_apply_device")
        return int(needed.value), {"rounds": stats.rounds, "pass_through": stats.pass_through, "searches": int(stats.searches)}

    def apply_host(self, values):
        """values: list of bytes -> (list of the new value, or None for an unchanged one; flags uint8[n]; stats dict)"""
        n = len(values)
        blob = np.frombuffer(b"".join(values) + b"\0", np.uint8).copy()
        lens = np.array([len(v) for v in values], np.uint32)
        at = np.zeros(n, np.uint64)
        if n:
            at[1:] = np.cumsum(lens[:-1])
        ptrs = (blob.ctypes.data + at).astype(np.uint64)
        flags = np.zeros(n, np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        out = ctypes.c_void_p()
        stats = LcDesensStats()
        rc = self._L.lc_desens_apply_host(self._h, ptrs.ctypes.data, lens.ctypes.data, n, flags.ctypes.data, out_off.ctypes.data,
                                          ctypes.byref(out), ctypes.byref(stats))
        if rc == LC_ERR_OVERFLOW:
            raise DesensitizeOverflow(0)
        binding._check(rc, "lc_desens_apply_host")
        try:
            new = ctypes.string_at(out, int(out_off[n])) if out.value else b""
        finally:
            self._L.lc_free(out)
        res = [new[int(out_off[i]):int(out_off[i + 1])] if flags[i] & LC_DESENS_CHANGED else None for i in range(n)]
        return res, flags, {"rounds": stats.rounds, "pass_through": stats.pass_through, "searches": int(stats.searches)}

    def close(self):
        if getattr(self, "_h", None):
            self._L.lc_desens_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DesensitizeProcessor(PluginProcessor):
    """processor_desensitize_gpu; same config keys as processor_desensitize_native.  collect_alarms(): kind 1 a search gave up, kind 3 a
    failed trip."""
    PREFIX, PLUGIN = "lc_desensitize", "processor_desensitize_gpu"

    def rounds(self):
        return int(self._L.lc_desensitize_rounds(self._h))

    def info(self):
        out = binding.LcRegexInfo()
        binding._check(self._L.lc_regex_info(self._L.lc_desens_regex(self._L.lc_desensitize_engine(self._h)), ctypes.byref(out)), "lc_regex_info")
        return {k: getattr(out, k) for k, _ in binding.LcRegexInfo._fields_}
