"""The field codec processors on the CPU: the product's processor code (csrc/processor_codec_gpu.cpp) over the host double of the device
trip (tests/native/codec_double.cpp, which runs the per-unit routines of csrc/codec_vm.hpp)."""
import ctypes

from helpers import native_build
from loongcollector_amd import abi, codec

# the double's own entries, and the rows of abi.CODEC_PROTOTYPES it answers (it has no device entry and no thread state)
LOCAL = {"cd_fail_next_trips": (None, [ctypes.c_int]), "cd_trip_stats": (None, [ctypes.POINTER(ctypes.c_uint64)])}
LOCAL.update({k: v for k, v in abi.CODEC_PROTOTYPES.items() if k not in ("lc_codec_apply_device", "lc_codec_thread_release", "lc_codec_set_trip_bytes")})


def double():
    return native_build.load_double("codec_double", ["processor_codec_gpu.cpp", "codec_double.cpp"], LOCAL)


def trip_stats(L):
    s = (ctypes.c_uint64 * 2)()
    L.cd_trip_stats(s)
    return {"trips": int(s[0]), "values": int(s[1])}


def processor(**config):
    return codec.Processor(lib=double(), **config)
