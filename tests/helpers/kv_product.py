"""processor_split_key_value on the CPU: the product's processor code (csrc/processor_split_key_value_gpu.cpp) over the host double of
the device trip (tests/native/kv_double.cpp, which runs the per-value routine of csrc/kv_vm.hpp), and scratch trees that hold a mutated
copy of the routine."""
import ctypes
import os
import shutil

from helpers import kv_cases, kv_model, native_build
from loongcollector_amd import abi, kvsplit

ROOT = kv_cases.ROOT
# the double's own entries, and the rows of abi.KVSPLIT_PROTOTYPES it answers (it has no device entry and no thread state)
LOCAL = {"kd_fail_next_trips": (None, [ctypes.c_int]), "kd_trip_stats": (None, [ctypes.POINTER(ctypes.c_uint64)])}
LOCAL.update({k: v for k, v in abi.KVSPLIT_PROTOTYPES.items() if k not in ("lc_kvsplit_device", "lc_kvsplit_thread_release")})


def double():
    return native_build.load_double("kv_double", ["processor_split_key_value_gpu.cpp", "kv_double.cpp"], LOCAL)


def trip_stats(L):
    s = (ctypes.c_uint64 * 3)()
    L.kd_trip_stats(s)
    return {"trips": int(s[0]), "values": int(s[1]), "last_W": int(s[2])}


def processor(**config):
    return kvsplit.Processor(lib=double(), **config)


def model_logs(config, logs):
    """the model's processLog over logs of (key, value) str pairs -> (logs of (str, str) tuples, [(kind, bytes)] alarms in order)"""
    out, alarms = [], []
    for log in logs:
        contents, heard = kv_model.process_log(config, [[k.encode("utf-8"), v.encode("utf-8")] for k, v in log])
        out.append([(k.decode("utf-8"), v.decode("utf-8")) for k, v in contents])
        alarms += heard
    return out, alarms


def mutated_host_check(tmp_path, old, new):
    """a scratch tree with csrc/kv_vm.hpp changed (old -> new, exactly one occurrence) -> the host check program built from it"""
    tree = os.path.join(str(tmp_path), "tree")
    for d in (os.path.join("loongcollector_amd", "csrc"), os.path.join("tests", "native")):
        os.makedirs(os.path.join(tree, d))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(tree, "include"))
    with open(os.path.join(ROOT, "loongcollector_amd", "csrc", "kv_vm.hpp"), encoding="utf-8") as f:
        text = f.read()
    assert text.count(old) == 1, old
    with open(os.path.join(tree, "loongcollector_amd", "csrc", "kv_vm.hpp"), "w", encoding="utf-8") as f:
        f.write(text.replace(old, new))
    src = os.path.join(tree, "tests", "native", "kv_host_check.cpp")
    shutil.copy(os.path.join(ROOT, "tests", "native", "kv_host_check.cpp"), src)
    return kv_cases.build_host_check(tmp_path, source=src)
