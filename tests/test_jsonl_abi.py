"""liblc_jsonl.so, the JSON-lines encoder's own library: abi.JSONL_PROTOTYPES equals the declarations of include/jsonl/lc_jsonl.h (names,
parameter counts, the kind of every parameter and return) and the library's exports, as tests/test_lz4_abi.py holds abi.LZ4_PROTOTYPES to
liblc_lz4.so -- and the other six libraries, whose ABIs this one leaves as they are, export none of it."""
import os
import re
import subprocess

import test_abi_table as main_table
from loongcollector_amd import abi, anchor, csv_decode, jsonl, kvsplit, lz4_block, sls

HEADER = os.path.join(main_table.ROOT, "include", "jsonl", "lc_jsonl.h")


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
    assert len(decl) == 12 and set(decl) == set(abi.JSONL_PROTOTYPES)
    others = (set(abi.PROTOTYPES) | set(abi.KVSPLIT_PROTOTYPES) | set(abi.CSV_PROTOTYPES) | set(abi.SLS_PROTOTYPES) | set(abi.ANCHOR_PROTOTYPES) |
              set(abi.LZ4_PROTOTYPES))
    assert not set(decl) & others
    for name, (ret, params) in decl.items():
        restype, argtypes = abi.JSONL_PROTOTYPES[name]
        assert main_table.c_kind(ret, fn_types, False) == main_table.ctypes_kind(restype), name
        assert [main_table.c_kind(p, fn_types, True) for p in params] == [main_table.ctypes_kind(a) for a in argtypes], name


def test_the_header_states_what_is_defined_here_and_what_is_pinned_on_the_model():
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    defined = text[text.index("DEFINED here"):text.index("PINNED ON THE MODEL")]
    assert "A RECORD OF 4 GiB IS NOT WRITTEN" in defined and "A ROW OUTSIDE ITS LINE IS CUT" in defined
    assert "AN EVENT THAT IS NOT A LOG EVENT IS SKIPPED" in defined and "the group takes the host path" in defined
    assert "NO BYTES IS NOT AN ERROR" in defined
    pinned = text[text.index("PINNED ON THE MODEL"):text.index("Kept as the reference has them")]
    assert "rapidjson is not part of the test environment" in pinned and "tests/helpers/jsonl_model.py" in pinned
    assert "json.dumps" in pinned and "rest on reading the reference's source alone" in pinned
    assert "THE NUL RULE" in text and "CUT AT THEIR FIRST 0x00 BYTE" in text
    assert "#define LC_JSONL_MAX_HEAD_BYTES 65536u" in text


def test_the_table_equals_the_exports_and_the_other_libraries_export_none_of_it():
    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {w[2] for w in (line.split() for line in out.splitlines()) if len(w) == 3 and w[1] in "TW" and w[2].startswith("lc_")}
    assert exports(jsonl.LIB_PATH) == set(abi.JSONL_PROTOTYPES)
    for path in (main_table.binding.LIB_PATH, kvsplit.LIB_PATH, csv_decode.LIB_PATH, sls.LIB_PATH, anchor.LIB_PATH, lz4_block.LIB_PATH):
        assert not exports(path) & set(abi.JSONL_PROTOTYPES), path
    assert exports(kvsplit.LIB_PATH) == set(abi.KVSPLIT_PROTOTYPES)
    assert exports(csv_decode.LIB_PATH) == set(abi.CSV_PROTOTYPES)
    assert exports(sls.LIB_PATH) == set(abi.SLS_PROTOTYPES)
    assert exports(anchor.LIB_PATH) == set(abi.ANCHOR_PROTOTYPES)
    assert exports(lz4_block.LIB_PATH) == set(abi.LZ4_PROTOTYPES)
