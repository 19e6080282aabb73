"""liblc_anchor.so, the anchor processor's own library: abi.ANCHOR_PROTOTYPES equals the declarations of include/anchor/lc_anchor.h (names,
parameter counts, the kind of every parameter and return) and the library's exports, as tests/test_abi_table.py holds abi.PROTOTYPES to
include/*.h and liblc_regex_gpu.so -- whose ABI this library leaves as it is."""
import os
import re
import subprocess

import test_abi_table as main_table
from loongcollector_amd import abi, anchor

HEADER = os.path.join(main_table.ROOT, "include", "anchor", "lc_anchor.h")


def declarations():
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    fn_types = main_table.header_declarations()[1]  # (lc_alarm_sink_t of lc_processor.h)
    out = {}
    for ret, name, params in main_table.DECLARATION.findall(text):
        if "typedef" not in ret:
            out[name] = (" ".join(ret.split()), [p.strip() for p in " ".join(params.split()).split(",") if p.strip() not in ("", "void")])
    return out, fn_types


def test_the_table_equals_the_header():
    decl, fn_types = declarations()
    assert len(decl) == 10 and set(decl) == set(abi.ANCHOR_PROTOTYPES) and not set(decl) & set(abi.PROTOTYPES)
    for other in (abi.KVSPLIT_PROTOTYPES, abi.CSV_PROTOTYPES, abi.SLS_PROTOTYPES):
        assert not set(decl) & set(other)
    for name, (ret, params) in decl.items():
        restype, argtypes = abi.ANCHOR_PROTOTYPES[name]
        assert main_table.c_kind(ret, fn_types, False) == main_table.ctypes_kind(restype), name
        assert [main_table.c_kind(p, fn_types, True) for p in params] == [main_table.ctypes_kind(a) for a in argtypes], name


def test_the_table_equals_the_exports_and_the_main_library_exports_none_of_it():
    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {w[2] for w in (line.split() for line in out.splitlines()) if len(w) == 3 and w[1] in "TW" and w[2].startswith("lc_")}
    assert exports(anchor.LIB_PATH) == set(abi.ANCHOR_PROTOTYPES)
    assert not exports(main_table.binding.LIB_PATH) & set(abi.ANCHOR_PROTOTYPES)


def test_the_header_states_what_is_defined_here():
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    assert "DEFINED here" in text and "LC_ANCHOR_MAX_ANCHORS 16u" in text and "LC_ANCHOR_MAX_NEEDLE 32u" in text
    assert anchor.LC_ANCHOR_NO_START == -1 and anchor.LC_ANCHOR_NO_STOP == -2 and len(anchor.COUNTERS) == 7
