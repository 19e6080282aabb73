"""liblc_sls.so, the SLS encoder's own library: abi.SLS_PROTOTYPES equals the declarations of include/sls/lc_sls.h (names, parameter
counts, the kind of every parameter and return) and the library's exports, as tests/test_abi_table.py holds abi.PROTOTYPES to
include/*.h and liblc_regex_gpu.so, tests/test_kv_abi.py abi.KVSPLIT_PROTOTYPES to liblc_kvsplit.so and tests/test_csv_abi.py
abi.CSV_PROTOTYPES to liblc_csv.so -- whose ABIs this library leaves as they are."""
import os
import re
import subprocess

import test_abi_table as main_table
from loongcollector_amd import abi, csv_decode, kvsplit, sls

HEADER = os.path.join(main_table.ROOT, "include", "sls", "lc_sls.h")


def declarations():
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    fn_types = main_table.header_declarations()[1]
    out = {}
    for ret, name, params in main_table.DECLARATION.findall(text):
        if "typedef" not in ret:
            out[name] = (" ".join(ret.split()), [p.strip() for p in " ".join(params.split()).split(",") if p.strip() not in ("", "void")])
    return out, fn_types


def test_the_table_equals_the_header():
    decl, fn_types = declarations()
    assert len(decl) == 12 and set(decl) == set(abi.SLS_PROTOTYPES)
    assert not set(decl) & (set(abi.PROTOTYPES) | set(abi.KVSPLIT_PROTOTYPES) | set(abi.CSV_PROTOTYPES))
    for name, (ret, params) in decl.items():
        restype, argtypes = abi.SLS_PROTOTYPES[name]
        assert main_table.c_kind(ret, fn_types, False) == main_table.ctypes_kind(restype), name
        assert [main_table.c_kind(p, fn_types, True) for p in params] == [main_table.ctypes_kind(a) for a in argtypes], name


def test_the_header_states_its_differences_from_the_reference_and_how_the_tags_are_pinned():
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    block = text[text.index("DEFINED here"):text.index("Kept as the reference has them")]
    assert "A RECORD OF 4 GiB IS NOT WRITTEN" in block and "A ROW OUTSIDE ITS LINE IS CUT" in block
    assert "PINNED ON THE MODEL" in block and "lc_sls_append_tags" in block and "tests/helpers/sls_wire.py" in block


def test_the_table_equals_the_exports_and_the_other_libraries_export_none_of_it():
    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {w[2] for w in (line.split() for line in out.splitlines()) if len(w) == 3 and w[1] in "TW" and w[2].startswith("lc_")}
    assert exports(sls.LIB_PATH) == set(abi.SLS_PROTOTYPES)
    assert not exports(main_table.binding.LIB_PATH) & set(abi.SLS_PROTOTYPES)
    assert exports(kvsplit.LIB_PATH) == set(abi.KVSPLIT_PROTOTYPES)
    assert exports(csv_decode.LIB_PATH) == set(abi.CSV_PROTOTYPES)
