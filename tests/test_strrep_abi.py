"""liblc_strrep.so, the string-replace processor's own library: abi.STRREP_PROTOTYPES equals the declarations of
include/strrep/lc_strrep.h (names, parameter counts, the kind of every parameter and return) and the library's exports, as
tests/test_abi_table.py holds abi.PROTOTYPES to include/*.h and liblc_regex_gpu.so -- whose ABI this library leaves as it is -- and the
create call refuses what the header says it refuses, each with its own message."""
import os
import re
import subprocess

import pytest

import test_abi_table as main_table
from helpers import strrep_model as model
from loongcollector_amd import abi, string_replace as sr

HEADER = os.path.join(main_table.ROOT, "include", "strrep", "lc_strrep.h")
LC_ERR_UNSUPPORTED, LC_ERR_ARG = 2, 5


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
    assert len(decl) == 9 and set(decl) == set(abi.STRREP_PROTOTYPES) and not set(decl) & set(abi.PROTOTYPES)
    for other in (abi.KVSPLIT_PROTOTYPES, abi.CSV_PROTOTYPES, abi.SLS_PROTOTYPES, abi.ANCHOR_PROTOTYPES, abi.LZ4_PROTOTYPES, abi.JSONL_PROTOTYPES):
        assert not set(decl) & set(other)
    for name, (ret, params) in decl.items():
        restype, argtypes = abi.STRREP_PROTOTYPES[name]
        assert main_table.c_kind(ret, fn_types, False) == main_table.ctypes_kind(restype), name
        assert [main_table.c_kind(p, fn_types, True) for p in params] == [main_table.ctypes_kind(a) for a in argtypes], name


def test_the_table_equals_the_exports_and_the_main_library_exports_none_of_it():
    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {w[2] for w in (line.split() for line in out.splitlines()) if len(w) == 3 and w[1] in "TW" and w[2].startswith("lc_")}
    assert exports(sr.LIB_PATH) == set(abi.STRREP_PROTOTYPES)
    assert not exports(main_table.binding.LIB_PATH) & set(abi.STRREP_PROTOTYPES)
    needed = subprocess.run(["readelf", "-d", sr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "liblc_regex_gpu.so" in needed  # linked against the main library, as liblc_anchor.so is


def test_the_header_states_what_is_defined_here():
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    assert "DEFINED here" in text and "LC_STRREP_MAX_MATCH 32u" in text and "LC_STRREP_MAX_REPLACE 256u" in text
    assert "READ OFF THE SOURCE" in text and "stays with the Go plugin" in text
    assert sr.LC_STRREP_CHANGED == 1 and sr.LC_STRREP_ERROR == 2 and len(sr.COUNTERS) == 5
    assert (sr.LC_STRREP_MAX_MATCH, sr.LC_STRREP_MAX_REPLACE) == (model.MAX_MATCH, model.MAX_REPLACE) == (32, 256)


REFUSALS = [
    ({"Method": "const", "Match": "m"}, LC_ERR_ARG, "no source key error"),
    ({"SourceKey": "", "Method": "unquote"}, LC_ERR_ARG, "no source key error"),
    ({"SourceKey": "k"}, LC_ERR_ARG, "no method error"),
    ({"SourceKey": "k", "Method": "md5"}, LC_ERR_ARG, "no method error"),
    ({"SourceKey": "k", "Method": "const"}, LC_ERR_ARG, "no match error"),
    ({"SourceKey": "k", "Method": "const", "Match": ""}, LC_ERR_ARG, "no match error"),
    ({"SourceKey": "k", "Method": "regex", "Match": "a+"}, LC_ERR_UNSUPPORTED, "stays with the Go plugin"),
    ({"SourceKey": "k", "Method": "const", "Match": "m" * 33}, LC_ERR_UNSUPPORTED, "Match is 33 bytes long"),
    ({"SourceKey": "k", "Method": "const", "Match": "啊" * 11}, LC_ERR_UNSUPPORTED, "Match is 33 bytes long"),
    ({"SourceKey": "k", "Method": "const", "Match": "m", "ReplaceString": "r" * 257}, LC_ERR_UNSUPPORTED, "ReplaceString is 257 bytes long"),
]


@pytest.mark.parametrize("config,code,message", REFUSALS, ids=[r[2].replace(" ", "_") + str(i) for i, r in enumerate(REFUSALS)])
def test_create_refusals_and_their_messages(config, code, message):
    """(the create call touches no device)"""
    with pytest.raises(sr.StringReplaceInitError) as err:
        sr.Processor(**config)
    assert message in str(err.value) and err.value.code == code
    assert message in model.init_error(config)


def test_create_accepts_the_bounds_and_ignores_the_timeout():
    p = sr.Processor(SourceKey="k", Method="const", Match="m" * 32, ReplaceString="r" * 256, RegexTimeoutMs=5, DestKey="d")
    assert p.handle and p.counters() == dict.fromkeys(sr.COUNTERS, 0)
    assert sr.Processor(SourceKey="k", Method="unquote", Match="ignored", RegexTimeoutMs=-1).handle
