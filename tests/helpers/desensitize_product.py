"""Loads tests/native/desens_double.cpp (built on first use into tests/_build/libdesens_double.so): the product's host code of
processor_desensitize_gpu with every search answered by the oracle's matcher and everything behind the search run by the __host__
instantiation of csrc/desens_vm.hpp; and the rules, corpora and fixture walk the CPU and the GPU suite share."""
import ctypes
import json
import os
import random

from helpers import plugin_double
from helpers.native_build import load_double, oracle_link
from loongcollector_amd.desensitize import GpuDesensitize

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONST, MD5 = 0, 1
CHANGED, GAVE_UP = 1, 2


def double():
    vp, cp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    return load_double("desens_double", ("desens_double.cpp", "processor_desensitize_gpu.cpp", "event_model.cpp"), {
        "dd_md5": (None, [cp, u32, cp]),
        "dd_rewrite_text": (vp, [cp, sz, i32]),
        "dd_fail_next_trips": (i32, [i32]),
        "dd_give_up_every": (i32, [i32]),
        "dd_apply_calls": (ctypes.c_uint64, []),
        "dd_process_json_rc": (vp, [vp, cp, cp, ctypes.POINTER(i32), ctypes.POINTER(i32), cp, sz]),
        "dd_free": (i32, [vp]),
        "dd_write_resident": (ctypes.c_uint64, [vp, vp, vp, u32, vp, vp, u32, vp, ctypes.POINTER(ctypes.c_double)]),
    }, extra=oracle_link())


def _b(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


class Engine(GpuDesensitize):
    """lc_desens_* of library L (the double by default): apply(values) -> (new value or None per value, flags, rounds)"""

    def __init__(self, method, before, content, replacing=b"", replacing_all=False, L=None):
        GpuDesensitize.__init__(self, method, before, content, replacing, replacing_all, lib=L or double())

    def apply(self, values):
        new, flags, stats = self.apply_host(values)
        return new, flags, stats["rounds"]


class Product(plugin_double.Product):
    """processor_desensitize_gpu of library L (the double by default).  process: (product, group JSON bytes) -> (rc, group JSON text)
    for a library that has no dd_process_json_rc (the real one goes through lc_group_from_json)"""
    PREFIX, ALARM_TEXT = "lc_desensitize", None

    def __init__(self, config, L=None, process=None):
        plugin_double.Product.__init__(self, config, L or double())
        self.key = config.get("SourceKey", "")
        self._process = process
        self.first_view_kept = None

    def process(self, group):
        """group: fixture dict -> (rc, the group afterwards as a dict)"""
        text = json.dumps(group).encode("utf-8")
        if self._process:
            rc, out = self._process(self, text)
            return rc, json.loads(out)
        rc, kept = ctypes.c_int(0), ctypes.c_int(0)
        err = ctypes.create_string_buffer(256)
        p = self.L.dd_process_json_rc(self.h, text, self.key.encode("utf-8"), ctypes.byref(rc), ctypes.byref(kept), err, 256)
        assert p, err.value
        try:
            out = ctypes.string_at(p).decode("utf-8")
        finally:
            self.L.dd_free(p)
        self.first_view_kept = bool(kept.value)
        return rc.value, json.loads(out)

    def rounds(self):
        return int(self.L.lc_desensitize_rounds(self.h))


# ---------------------------------------------------------------------------------------------- the rules of the issue's list
# (name, before, content, ReplacingString)
RULES = [
    ("pwd", "pwd=", "[^,]+", "********"),
    ("card", "card=", r"(\d{4}-)(?:\d{4}-){2}\d{4}", r"\2****-****-****"),
    ("word", r"\bkey\b", r"=\w+", "=?"),
    ("anchor", "^a", "b", "X"),
    ("empty", "(?:)", "x*", "-"),
    ("dollar", "end=", r"\w+$", "#"),
    ("newline", "msg=", ".+", "<m>"),
    ("edge", "(?:)", "S[a-z]*", "0123456789"),
    ("digest", "k=", "[a-z]*", "z"),
    ("threads", "k=", "[ab]*a[ab]{14}", "#"),   # no tagged DFA within the limits: the thread-list engine (LC_ENGINE_NFA)
    ("tables", "k=", r"\w*a\w{12};", "#"),      # a tagged DFA too large for LDS: the tables are read from global memory
]
RULE = {r[0]: r for r in RULES}

RULE_VALUES = {
    "pwd": [b"asf@@@324 FS2$%pwd,pwd=saf543#$@,,", b"pwd=a,pwd=b,pwd=c", b"no secret here", b"pwd=", b"pwd=,x", b"xpwd=tail-without-comma",
            b"\r\n\r\nasf@@\n\n@324 FS2$%pwd,pwd=saf543#$@,,", "pwd=密码密,中文 pwd=été,".encode("utf-8")],
    "card": [b"card=1234-5678-9012-3456 ok", b"card=1234-5678-9012-345", b"card=0000-1111-2222-3333;card=4444-5555-6666-7777", b"card", b"1234-5678"],
    "word": [b"key=abc", b"monkey=abc key=d", b"key=1 keys=2 key=3", b"akey=1", b"key", b"key=", b"key=a,key=b"],
    "anchor": [b"abab", b"ab", b"ba", b"abababab", b"a", b"b"],
    "empty": [b"", b"x", b"xx", b"ax", b"axxb", b"abc", b"xaxx", b"xxxxa"],
    "dollar": [b"end=abc", b"end=abc end=def", b"end=abc\n", b"end=a b", b"end=", b"x end=12"],
    "newline": [b"msg=one\ntwo", b"msg=\nmsg=b", b"msg=a\nmsg=b\nmsg=c", b"msg=", b"x\nmsg=tail", b"msg=a\n"],
    "edge": [b"..Sabc.", b"S", b"Sa.Sb.S", b"none"],
    "digest": [b"k=;", b"k=a;", b"k=abc;k=;k=zz", b"k=", b"xk=abc", b"k"],
    "threads": [b"k=" + b"ab" * 20 + b";", b"x k=aaaaaaaaaaaaaaaa k=bbbbbbbbbbbbbbbbbbbbbbbb", b"k=a", b"none", b"k=" + b"ba" * 8 + b" k=" + b"a" * 15,
                b"k=" + b"b" * 40 + b"a" + b"b" * 14 + b"bb k=ab"],
    "tables": [b"k=xxa123456789012; k=a123456789012;", b"k=a12345678901;", b"none", b"k=" + b"za" * 30 + b"0123456789ab;;"],
}

POSITIONS = (0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513)
CONTENT_SIZES = (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128, 1000)
MATCH_COUNTS = (0, 1, 2, 3, 63, 64, 65)
BATCH_SIZES = (0, 1, 63, 64, 65, 1000)


def edge_values():
    """rule "edge" (the cut is the whole match for both methods): the cut BEGINS on byte p, and separately ENDS on byte p; packed back
    to back these values start on every residue mod 16 (checked by the caller)"""
    out = []
    for p in POSITIONS:
        out.append(b"." * p + b"Sabc." + b"t" * (p % 7))  # begins on p
        out.append(b"." * p + b"Sab")                      # begins on p, ends with the value
        if p >= 1:
            k = min(p, 5)
            out.append(b"." * (p - k) + b"S" + b"a" * (k - 1) + b".tail")  # ends on p
            out.append(b"." * (p - k) + b"S" + b"a" * (k - 1))             # ends on p = the value's end
    for residue in range(16):  # a value with a cut on every residue of the first byte
        at = sum(map(len, out))
        out.append(b"." * ((residue - at - 1) % 16 + 1))
        out.append(b"Sx.")
    return out


def digest_values():
    """rule "digest" under md5: contents of every size of CONTENT_SIZES (0: a legal empty content, the MD5 of the empty string)"""
    return [b"head k=" + b"a" * size + b";tail" for size in CONTENT_SIZES] + [b"k=" + b"b" * size for size in CONTENT_SIZES]


def counted_values(rng=None):
    """rule "pwd": values with 0, 1, 2, 3, 63, 64 and 65 matches, every second one without any, 70 of them: more than one wavefront"""
    rng = rng or random.Random(11)
    out = []
    for i in range(70):
        if i % 2:
            out.append(b"nothing to see " * rng.randrange(1, 4))
        else:
            out.append(b"".join(b"pwd=%d," % rng.randrange(10 ** rng.randrange(1, 7)) for _ in range(MATCH_COUNTS[(i // 2) % len(MATCH_COUNTS)])) + b"end")
    return out


def random_batch(n=1 << 16, seed=20261019):
    """n values of 32..700 bytes with 0 to 4 secrets each for rule "pwd".  The filler holds no backtracking trap: the rule's pattern is a
    literal and one negated class, linear for every matcher (the CPU suite checks that the model never gives up on it)."""
    rng = random.Random(seed)
    alphabet = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 _-:;/=.@#[]\"'\t"
    out = []
    for _ in range(n):
        size = rng.randrange(32, 701)
        secrets = [b"pwd=" + bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, 17))) + b"," for _ in range(rng.randrange(0, 5))]
        body = bytearray(rng.choice(alphabet) for _ in range(max(size - sum(map(len, secrets)), 0)))
        cuts = sorted(rng.randrange(len(body) + 1) for _ in secrets)
        parts, at = [], 0
        for c, s in zip(cuts, secrets):
            parts += [bytes(body[at:c]), s]
            at = c
        parts.append(bytes(body[at:]))
        out.append(b"".join(parts)[:700].ljust(32, b"."))
    return out


_RANDOM = {}


def random_expected(method):
    """the model over the random batch, once per method and process (the CPU and the GPU suite share it) -> (values, new values);
    raises where the oracle gives up"""
    if method not in _RANDOM:
        from helpers import desensitize_model as model
        values = random_batch()
        rule = model.Rule(method, *RULE["pwd"][1:], True)
        _RANDOM[method] = (values, [rule.apply(v) for v in values])
    return _RANDOM[method]


# ---------------------------------------------------------------------------------------------- fixtures
def load_fixtures():
    with open(os.path.join(GOLDEN, "desensitize_unittest_vectors.json"), encoding="utf-8") as f:
        return json.load(f)
