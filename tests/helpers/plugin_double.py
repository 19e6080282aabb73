"""What the Product classes of the suite share: one plugin instance of a library (a host double, or the real one) opened by its C
prefix -- create with the error text, the alarm sink into a list, warnings(), the raw counters and destroy.  A subclass keeps what is
its own: how a group goes through (the double's *_process_json_rc shim), its setters, and the shape of its counters."""
import ctypes
import json

from loongcollector_amd import abi
from loongcollector_amd.processor import COUNTER_NAMES


class Product:
    PREFIX = None          # "lc_delimiter_processor": <PREFIX>_create, _destroy, _warnings, _counters, _set_alarm_sink
    FREE = "lc_free"       # what releases a string the library handed out
    ALARM_TEXT = "latin-1"  # alarms are (kind, message decoded so); None: the message stays bytes

    def _fn(self, name):
        return getattr(self.L, "%s_%s" % (self.PREFIX, name))

    def __init__(self, config, L, *create_args, create="create"):
        """<PREFIX>_<create>(config (a dict, or the JSON text as bytes), *create_args, &handle, err, 512); raises ValueError with the library's text"""
        self.L = L
        self.h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        self.rc = self._fn(create)(config if isinstance(config, bytes) else json.dumps(config).encode(), *create_args, ctypes.byref(self.h), err, 512)
        if self.rc != 0:
            self.h = None
            raise ValueError(err.value.decode("utf-8", "replace"))
        self.alarms = []
        text = (lambda b: b.decode(self.ALARM_TEXT)) if self.ALARM_TEXT else (lambda b: b)
        self._cb = abi.ALARM_SINK(lambda user, kind, msg, n: self.alarms.append((kind, text(ctypes.string_at(msg, n)))))
        self._fn("set_alarm_sink")(self.h, ctypes.cast(self._cb, ctypes.c_void_p), None)

    def __del__(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def take_text(self, p, encoding="utf-8", free=None):
        """the text of a string the library handed out, which is released"""
        try:
            return ctypes.string_at(p).decode(encoding)
        finally:
            getattr(self.L, free or self.FREE)(p)

    def warnings(self):
        return [w for w in self.take_text(self._fn("warnings")(self.h)).split("\n") if w]

    def counter_values(self):
        c = (ctypes.c_uint64 * len(COUNTER_NAMES))()
        assert self._fn("counters")(self.h, c) == 0
        return [int(x) for x in c]

    def counters(self):
        return dict(zip(COUNTER_NAMES, self.counter_values()))


def clock_arg(product, now):
    """create_with_clock's (clock, user) for a product whose .now is read at every call; (None, None) when now is None"""
    product.now = now
    product._clock = abi.CLOCK(lambda user: product.now) if now is not None else None
    return (ctypes.cast(product._clock, ctypes.c_void_p) if product._clock else None, None)
