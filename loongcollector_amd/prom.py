"""ctypes binding of the Prometheus text-line parser (include/lc_prom.h): parse_device / parse_host are the engine (prom_parse_kernel
over lines in device or host memory), PromProcessor the processor_prom_parse_metric_gpu plugin over event groups (same shape as
processor.Processor), RawGroup a group of raw events whose metric events can be read back.  There is no CPU path: every parse needs a
HIP device and raises otherwise."""
import ctypes

import numpy as np

from . import binding
from .abi import PROM_OUT_KEYS as OUT_KEYS, LcPromOut  # noqa: F401
from .processor import EventGroup, PluginProcessor

LC_PROM_OK = 0
(LC_PROM_FAIL_NAME, LC_PROM_FAIL_NAME_END, LC_PROM_FAIL_EQUAL, LC_PROM_FAIL_LABEL_NAME, LC_PROM_FAIL_QUOTE, LC_PROM_FAIL_LABEL_VALUE_END,
 LC_PROM_FAIL_LABEL_VALUE_NEXT, LC_PROM_FAIL_COMMA_OR_BRACE, LC_PROM_FAIL_VALUE_END, LC_PROM_FAIL_VALUE, LC_PROM_FAIL_TIME_END,
 LC_PROM_FAIL_TIMESTAMP, LC_PROM_FAIL_TIMESTAMP_OVERFLOW, LC_PROM_FAIL_TIMESTAMP_SMALL, LC_PROM_FAIL_TIMESTAMP_NAN) = range(1, 16)
LC_PROM_VALUE_HOST, LC_PROM_TIME_HOST, LC_PROM_HAS_TIME, LC_PROM_ANY_ESCAPE = 1, 2, 4, 8
LC_PROM_LABEL_ESCAPED = 0x80000000
LC_PROM_DEFAULT_LABELS = 16
SCRAPE_TIMESTAMP = "prometheus.scrape.timestamp.millisec"  # the name lc_group_set_metadata knows the scrape timestamp by


def out_shapes(n, W):
    """-> {key: (shape, dtype)} of the result arrays for n lines at W labels per line"""
    return {"status": ((n,), np.uint8), "flags": ((n,), np.uint8), "name": ((n, 2), np.int32), "value": ((n,), np.uint64),
            "value_span": ((n, 2), np.int32), "time_span": ((n, 2), np.int32), "secs": ((n,), np.int64), "nanos": ((n,), np.uint32),
            "nlabels": ((n,), np.uint32), "labels": ((n, W, 4), np.int32)}


def _lib():
    return binding.load()


class RawGroup(EventGroup):
    """A group as the scraper hands it over: one RawEvent per exposition line (`lines`: bytes; None: a log event, i.e. an event that is
    no RawEvent), the scrape timestamp as metadata (`scrape_ms`: int or any text; None: not set)."""

    def __init__(self, lines, scrape_ms=None):
        self._L = _lib()
        self._h = self._L.lc_group_new()
        for line in lines:
            if line is None:
                binding._check(self._L.lc_group_add_log_event(self._h, b"content", b"not a raw event"), "lc_group_add_log_event")
            else:
                binding._check(self._L.lc_group_add_raw_event(self._h, line, len(line)), "lc_group_add_raw_event")
        if scrape_ms is not None:
            binding._check(self._L.lc_group_set_metadata(self._h, SCRAPE_TIMESTAMP.encode(), str(scrape_ms).encode()), "lc_group_set_metadata")

    def events(self):
        """-> per event: {"type", "secs", "nanos"} and for a metric event "name" (bytes), "bits" (int), "tags" ([(key, value)] bytes)"""
        L, h, out = self._L, self._h, []
        for i in range(len(self)):
            secs, nanos, has = ctypes.c_int64(), ctypes.c_uint32(), ctypes.c_int()
            L.lc_group_event_timestamp(h, i, ctypes.byref(secs), ctypes.byref(nanos), ctypes.byref(has))
            ev = {"type": int(L.lc_group_event_type(h, i)), "secs": int(secs.value), "nanos": int(nanos.value) if has.value else None}
            if ev["type"] == 2:
                p, n, bits = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()
                binding._check(L.lc_group_metric_name(h, i, ctypes.byref(p), ctypes.byref(n)), "lc_group_metric_name")
                ev["name"] = ctypes.string_at(p, n.value) if n.value else b""
                binding._check(L.lc_group_metric_value_bits(h, i, ctypes.byref(bits)), "lc_group_metric_value_bits")
                ev["bits"] = int(bits.value)
                tags = []
                for k in range(int(L.lc_group_metric_tag_count(h, i))):
                    kp, kn, vp_, vn = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_void_p(), ctypes.c_size_t()
                    binding._check(L.lc_group_metric_tag(h, i, k, ctypes.byref(kp), ctypes.byref(kn), ctypes.byref(vp_), ctypes.byref(vn)), "lc_group_metric_tag")
                    tags.append((ctypes.string_at(kp, kn.value) if kn.value else b"", ctypes.string_at(vp_, vn.value) if vn.value else b""))
                ev["tags"] = tags
            out.append(ev)
        return out


def parse_device(honor_timestamps, d_data, d_off, n, d_out, W, stream=0):
    """d_data uint8, d_off int32[n + 1], d_out: dict of device tensors under OUT_KEYS (out_shapes(n, W)).  Asynchronous on `stream`.  Tokens
    flagged LC_PROM_VALUE_HOST / LC_PROM_TIME_HOST are the caller's to finish."""
    o = LcPromOut(*(d_out[k].data_ptr() if d_out[k] is not None else None for k in OUT_KEYS))
    binding._check(_lib().lc_prom_parse_device(int(bool(honor_timestamps)), d_data.data_ptr(), d_off.data_ptr(), n, ctypes.byref(o), W, stream),
                   "lc_prom_parse_device")


def parse_host(lines, honor_timestamps=True, W=LC_PROM_DEFAULT_LABELS, fill=None):
    """lines: list of bytes -> dict of numpy arrays under OUT_KEYS (fill: the byte every array holds beforehand) plus "deferred" (how many
    tokens the host finished with strtod)"""
    n = len(lines)
    blob = np.frombuffer(b"".join(lines) + b"\0", np.uint8).copy()
    lens = np.array([len(v) for v in lines], np.uint32)
    off = np.zeros(n, np.uint64)
    if n:
        off[1:] = np.cumsum(lens[:-1])
    ptrs = (blob.ctypes.data + off).astype(np.uint64)
    res = {k: np.zeros(s, t) for k, (s, t) in out_shapes(n, W).items()}
    if fill is not None:
        for v in res.values():
            v.view(np.uint8)[...] = fill & 0xFF
    o = LcPromOut(*(res[k].ctypes.data for k in OUT_KEYS))
    deferred = ctypes.c_uint64(0)
    binding._check(_lib().lc_prom_parse_host(int(bool(honor_timestamps)), ptrs.ctypes.data, lens.ctypes.data, n, ctypes.byref(o), W, ctypes.byref(deferred)),
                   "lc_prom_parse_host")
    res["deferred"] = int(deferred.value)
    return res


class PromProcessor(PluginProcessor):
    """processor_prom_parse_metric_gpu; the config keys of processor_prom_parse_metric_native that bear on it (job_name, honor_timestamps;
    lc_prom.h).  collect_alarms(): kind 1 an unparsable scrape timestamp, kind 3 a failed trip."""
    PREFIX, PLUGIN = "lc_prom_processor", "processor_prom_parse_metric_gpu"

    def __init__(self, config, config_name="", lib=None):
        self._create(config, lib=lib)
        self._L.lc_prom_processor_set_config_name(self._h, config_name.encode("utf-8"))

    def deferred_tokens(self):
        return int(self._L.lc_prom_processor_deferred_tokens(self._h))

    def mop_up_lines(self):
        return int(self._L.lc_prom_processor_mop_up_lines(self._h))

    def set_first_trip_labels(self, W):
        self._L.lc_prom_processor_set_first_trip_labels(self._h, W)
