"""liblc_lz4.so, the LZ4 block writer's own library: abi.LZ4_PROTOTYPES equals the declarations of include/lz4/lc_lz4.h (names, parameter
counts, the kind of every parameter and return) and the library's exports, as tests/test_sls_abi.py holds abi.SLS_PROTOTYPES to
liblc_sls.so -- and the other five libraries, whose ABIs this one leaves as they are, export none of it."""
import os
import re
import subprocess

import test_abi_table as main_table
from loongcollector_amd import abi, anchor, csv_decode, kvsplit, lz4_block, sls

HEADER = os.path.join(main_table.ROOT, "include", "lz4", "lc_lz4.h")


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
    assert len(decl) == 9 and set(decl) == set(abi.LZ4_PROTOTYPES)
    others = set(abi.PROTOTYPES) | set(abi.KVSPLIT_PROTOTYPES) | set(abi.CSV_PROTOTYPES) | set(abi.SLS_PROTOTYPES) | set(abi.ANCHOR_PROTOTYPES)
    assert not set(decl) & others
    for name, (ret, params) in decl.items():
        restype, argtypes = abi.LZ4_PROTOTYPES[name]
        assert main_table.c_kind(ret, fn_types, False) == main_table.ctypes_kind(restype), name
        assert [main_table.c_kind(p, fn_types, True) for p in params] == [main_table.ctypes_kind(a) for a in argtypes], name


def test_the_header_states_what_is_defined_here():
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    block = text[text.index("DEFINED here"):text.index("Kept as the reference has it")]
    assert "VALID LZ4, NOT LZ4_compress_default's BYTES" in block and "the server only ever decodes" in block
    assert "THE CHUNK RULE" in block and "What it costs" in block
    assert "NO ZSTD" in block
    assert "THIS IS NOT THE PATH THE LIBRARY EXISTS FOR" in text


def test_the_table_equals_the_exports_and_the_other_libraries_export_none_of_it():
    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {w[2] for w in (line.split() for line in out.splitlines()) if len(w) == 3 and w[1] in "TW" and w[2].startswith("lc_")}
    assert exports(lz4_block.LIB_PATH) == set(abi.LZ4_PROTOTYPES)
    for path in (main_table.binding.LIB_PATH, kvsplit.LIB_PATH, csv_decode.LIB_PATH, sls.LIB_PATH, anchor.LIB_PATH):
        assert not exports(path) & set(abi.LZ4_PROTOTYPES), path
    assert exports(sls.LIB_PATH) == set(abi.SLS_PROTOTYPES)
    assert exports(anchor.LIB_PATH) == set(abi.ANCHOR_PROTOTYPES)
