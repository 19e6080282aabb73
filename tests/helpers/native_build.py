"""The one recipe for the host doubles of the CPU suite: the product's host sources compiled next to a tests/native/*_double.cpp that
stands in for the device trip, into tests/_build/lib<name>.so.  (The stand-alone sanitizer programs and the reference-linked builders
have their own compile lines.)"""
import ctypes
import functools
import os
import subprocess

from loongcollector_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "loongcollector_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
INCLUDE = os.path.join(ROOT, "include")
OUT_DIR = os.path.join(ROOT, "tests", "_build")
_LOADED = {}
_newest = None


def newest_source():
    """mtime of the newest file under csrc, include and tests/native: an output older than it is stale (build.py's rule for objects)"""
    global _newest
    if _newest is None:
        _newest = max(os.path.getmtime(os.path.join(d, f)) for top in (CSRC, INCLUDE, NATIVE) for d, _, files in os.walk(top) for f in files)
    return _newest


def source(name):
    """a source named by its file name: tests/native first, then csrc"""
    for d in (NATIVE, CSRC):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    raise FileNotFoundError(name)


@functools.lru_cache(maxsize=None)
def _oracle_built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


def oracle_link():
    """link flags for oracle/liboracle.so (the matcher that answers a double's searches), built if need be (once per process)"""
    _oracle_built()
    d = os.path.join(ROOT, "oracle")
    return ["-L" + d, "-loracle", "-Wl,-rpath," + d]


def build_shared(name, sources, extra=()):
    """sources: file names under tests/native or csrc; extra: further compiler and linker arguments -> tests/_build/lib<name>.so"""
    os.makedirs(OUT_DIR, exist_ok=True)
    so = os.path.join(OUT_DIR, "lib%s.so" % name)
    if not os.path.exists(so) or os.path.getmtime(so) < newest_source():
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-w", "-I", INCLUDE, "-I", CSRC, "-o", so] +
                              [source(s) for s in sources] + list(extra) + ["-Wl,--no-undefined", "-Wl,-Bsymbolic"])
    return so


def load_double(name, sources, local, extra=()):
    """the double as a CDLL, once per process: its lc_* entry points bound by abi.bind, its test-only ones by `local`, a table of the same
    form (name -> (restype, [argtypes]))"""
    if name not in _LOADED:
        _LOADED[name] = abi.bind(ctypes.CDLL(build_shared(name, sources, extra)), local)
    return _LOADED[name]
