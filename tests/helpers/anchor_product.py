"""processor_anchor on the CPU: the product's processor code (csrc/processor_anchor_gpu.cpp) over the host double of the device trip
(tests/native/anchor_double.cpp, which runs the per-value routine of csrc/anchor_vm.hpp), and scratch trees that hold a mutated copy of
the routine."""
import ctypes
import os
import shutil

from helpers import anchor_cases, anchor_model, native_build
from loongcollector_amd import abi, anchor

ROOT = anchor_cases.ROOT
# the double's own entries, and the rows of abi.ANCHOR_PROTOTYPES it answers (it has no device entry and no thread state)
LOCAL = {"ad_fail_next_trips": (None, [ctypes.c_int]), "ad_trip_stats": (None, [ctypes.POINTER(ctypes.c_uint64)])}
LOCAL.update({k: v for k, v in abi.ANCHOR_PROTOTYPES.items() if k not in ("lc_anchor_locate_device", "lc_anchor_thread_release")})


def double():
    return native_build.load_double("anchor_double", ["processor_anchor_gpu.cpp", "anchor_double.cpp"], LOCAL)


def trip_stats(L):
    s = (ctypes.c_uint64 * 2)()
    L.ad_trip_stats(s)
    return {"trips": int(s[0]), "values": int(s[1])}


def processor(**config):
    return anchor.Processor(lib=double(), **config)


def model_logs(config, logs):
    """the model's ProcessLog over logs of (key, value) str pairs -> (logs of (str, str) tuples, [(kind, bytes)] alarms in order, the
    pairs-per-log sum)"""
    out, alarms, metric = [], [], 0
    for log in logs:
        contents, heard, pairs = anchor_model.process_log(config, [[k, v] for k, v in log])
        out.append([(k.decode("utf-8"), v.decode("utf-8")) for k, v in contents])
        alarms += heard
        metric += pairs
    return out, alarms, metric


def mutated_host_check(tmp_path, old, new):
    """a scratch tree with csrc/anchor_vm.hpp changed (old -> new, exactly one occurrence) -> the host check program built from it"""
    tree = os.path.join(str(tmp_path), "tree")
    for d in (os.path.join("loongcollector_amd", "csrc"), os.path.join("tests", "native")):
        os.makedirs(os.path.join(tree, d))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(tree, "include"))
    with open(os.path.join(ROOT, "loongcollector_amd", "csrc", "anchor_vm.hpp"), encoding="utf-8") as f:
        text = f.read()
    assert text.count(old) == 1, old
    with open(os.path.join(tree, "loongcollector_amd", "csrc", "anchor_vm.hpp"), "w", encoding="utf-8") as f:
        f.write(text.replace(old, new))
    src = os.path.join(tree, "tests", "native", "anchor_host_check.cpp")
    shutil.copy(os.path.join(ROOT, "tests", "native", "anchor_host_check.cpp"), src)
    return anchor_cases.build_host_check(tmp_path, source=src)
