"""processor_string_replace on the CPU: the product's processor code (csrc/processor_string_replace_gpu.cpp) over the host double of the
device trip (tests/native/strrep_double.cpp, which runs the per-value routines of csrc/strrep_vm.hpp)."""
import ctypes

from helpers import native_build
from loongcollector_amd import abi, string_replace

# the double's own entries, and the rows of abi.STRREP_PROTOTYPES it answers (it has no device entry and no thread state)
LOCAL = {"sd_fail_next_trips": (None, [ctypes.c_int]), "sd_trip_stats": (None, [ctypes.POINTER(ctypes.c_uint64)])}
LOCAL.update({k: v for k, v in abi.STRREP_PROTOTYPES.items() if k not in ("lc_strrep_apply_device", "lc_strrep_thread_release")})


def double():
    return native_build.load_double("strrep_double", ["processor_string_replace_gpu.cpp", "strrep_double.cpp"], LOCAL)


def trip_stats(L):
    s = (ctypes.c_uint64 * 2)()
    L.sd_trip_stats(s)
    return {"trips": int(s[0]), "values": int(s[1])}


def processor(**config):
    return string_replace.Processor(lib=double(), **config)
