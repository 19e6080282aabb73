"""liblc_codec.so, the field codecs' own library: abi.CODEC_PROTOTYPES equals the declarations of include/codec/lc_codec.h (names,
parameter counts, the kind of every parameter and return) and the library's exports, as tests/test_abi_table.py holds abi.PROTOTYPES to
include/*.h and liblc_regex_gpu.so -- whose ABI this library leaves as it is -- the create call refuses a missing or unknown Op and
nothing else, and the argument errors that need no device."""
import ctypes
import os
import re
import subprocess

import pytest

import test_abi_table as main_table
from helpers import codec_model as model
from loongcollector_amd import abi, codec

HEADER = os.path.join(main_table.ROOT, "include", "codec", "lc_codec.h")
LC_ERR_ARG = 5


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
    assert len(decl) == 10 and set(decl) == set(abi.CODEC_PROTOTYPES) and not set(decl) & set(abi.PROTOTYPES)
    for other in (abi.KVSPLIT_PROTOTYPES, abi.CSV_PROTOTYPES, abi.SLS_PROTOTYPES, abi.ANCHOR_PROTOTYPES, abi.LZ4_PROTOTYPES, abi.JSONL_PROTOTYPES,
                  abi.STRREP_PROTOTYPES):
        assert not set(decl) & set(other)
    for name, (ret, params) in decl.items():
        restype, argtypes = abi.CODEC_PROTOTYPES[name]
        assert main_table.c_kind(ret, fn_types, False) == main_table.ctypes_kind(restype), name
        assert [main_table.c_kind(p, fn_types, True) for p in params] == [main_table.ctypes_kind(a) for a in argtypes], name


def test_the_table_equals_the_exports_and_the_main_library_exports_none_of_it():
    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {w[2] for w in (line.split() for line in out.splitlines()) if len(w) == 3 and w[1] in "TW" and w[2].startswith("lc_")}
    assert exports(codec.LIB_PATH) == set(abi.CODEC_PROTOTYPES)
    assert not exports(main_table.binding.LIB_PATH) & set(abi.CODEC_PROTOTYPES)
    needed = subprocess.run(["readelf", "-d", codec.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "liblc_regex_gpu.so" in needed  # linked against the main library, as liblc_strrep.so is


def test_the_header_states_what_is_defined_here():
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    assert "DEFINED here" in text and "ARE the definition" in text and "READ OFF THE SOURCE" in text and "BINARY VALUES" in text
    for name in ("BASE64_D_ALARM", "BASE64_D_FIND_ALARM", "BASE64_E_FIND_ALARM", "MD5_FIND_ALARM", "illegal base64 data at input byte",
                 "d41d8cd98f00b204e9800998ecf8427e"):
        assert name in text, name
    assert (codec.LC_CODEC_OUT, codec.LC_CODEC_ERROR) == (model.OUT, model.ERROR) == (1, 2)
    assert codec.COUNTERS == model.COUNTERS and len(codec.COUNTERS) == 5 and codec.OPS == model.OPS
    assert (codec.LC_CODEC_ALARM_DECODE, codec.LC_CODEC_ALARM_NO_KEY, codec.LC_CODEC_ALARM_TRIP_FAILED) == \
        (model.ALARM_DECODE, model.ALARM_NO_KEY, model.ALARM_TRIP_FAILED)


@pytest.mark.parametrize("config", [{}, {"SourceKey": "src", "NewKey": "dest"}, {"Op": ""}, {"Op": "base32"}, {"Op": "MD5"}, {"Op": 5}],
                         ids=["empty", "no_op", "empty_op", "base32", "upper_case", "a_number"])
def test_create_refuses_a_missing_or_unknown_op(config):
    """(the create call touches no device)"""
    with pytest.raises(codec.CodecInitError) as err:
        _create(config)
    assert "Op" in str(err.value) and "base64_encode" in str(err.value) and err.value.code == LC_ERR_ARG
    assert model.init_error(config) == "Op"


def _create(config):
    import json
    L = codec.load()
    text = json.dumps(config).encode()
    handle, err = ctypes.c_void_p(), ctypes.create_string_buffer(256)
    rc = L.lc_codec_create(text, len(text), ctypes.byref(handle), err, 256)
    if rc != 0:
        assert not handle.value
        raise codec.CodecInitError(err.value.decode(), rc)
    L.lc_codec_free(handle)


def test_create_refuses_nothing_else():
    for op in model.OPS:
        assert model.init_error({"Op": op}) is None
        p = codec.Processor(Op=op)  # no SourceKey: it matches contents whose key is empty
        assert p.handle and p.counters() == dict.fromkeys(codec.COUNTERS, 0)
        assert codec.Processor(Op=op, SourceKey="", NewKey="", MD5Key="", NoKeyError=True, DecodeError=True, Unknown=[1]).handle
    handle, err = ctypes.c_void_p(), ctypes.create_string_buffer(256)
    assert codec.load().lc_codec_create(b"[]", 2, ctypes.byref(handle), err, 256) == LC_ERR_ARG and b"JSON object" in err.value


def test_argument_errors_that_need_no_device():
    L, p = codec.load(), codec.Processor(Op="md5")
    needed, out = ctypes.c_uint64(9), ctypes.c_void_p(1)
    word = (ctypes.c_uint64 * 8)()
    at = (ctypes.addressof(word) + 15) & ~15
    assert L.lc_codec_apply_device(None, at, at, 1, at, at, at, at, at, 16, ctypes.byref(needed), None) == LC_ERR_ARG and needed.value == 0
    assert L.lc_codec_apply_device(p.handle, None, None, 0, None, None, None, None, None, 0, ctypes.byref(needed), None) == 0  # n = 0 touches nothing
    for k in (1, 2, 4, 6, 7):
        args = [p.handle, at, at, 1, at, at, at, at, None, 0, ctypes.byref(needed), None]
        args[k] = None
        assert L.lc_codec_apply_device(*args) == LC_ERR_ARG, k
    assert L.lc_codec_apply_device(p.handle, at, at, 1, at, at, at, at, at + 8, 16, ctypes.byref(needed), None) == LC_ERR_ARG  # d_out: 16-byte aligned
    assert L.lc_codec_apply_host(None, at, at, 1, at, at, at, at, ctypes.byref(out)) == LC_ERR_ARG and not out.value
    assert L.lc_codec_apply_host(p.handle, at, at, 1, at, at, at, at, None) == LC_ERR_ARG
    assert L.lc_codec_apply_host(p.handle, None, at, 1, at, at, at, at, ctypes.byref(out)) == LC_ERR_ARG
    assert L.lc_codec_apply_host(p.handle, None, None, 0, None, None, at, None, ctypes.byref(out)) == 0 and not any(word)
    assert L.lc_codec_counters(None, word) == LC_ERR_ARG and L.lc_codec_process_logs_json(p.handle, None, 0, ctypes.byref(out)) == LC_ERR_ARG
    L.lc_codec_set_alarm_sink(None, None, None)
    L.lc_codec_free(None)
    L.lc_codec_free_string(None)
