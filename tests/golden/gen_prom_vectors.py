"""Writes tests/golden/prom_reference_outputs.json and prom_unittest_vectors.json: the output of the REFERENCE's OWN TextParser::ParseLine.

    python tests/golden/gen_prom_vectors.py          (needs the reference tree and a built oracle/_ref; CPU only)

core/prometheus/labels/TextParser.cpp is compiled, where it lies in the reference tree, into a TEMPORARY directory against
oracle/_ref/libref_models.so (the reference's own MetricEvent / MetricValue / PipelineEventGroup) and the existing stub headers, with a
small driver that hands ParseLine one line from an exactly sized, NUL-terminated heap copy and packs the MetricEvent it filled.
TextParser::Parse (never called) names two helpers of prometheus/Utils.cpp; the driver defines them empty so that the library links.
Per case: the line (latin-1 text), honor_timestamps, the defaults, ok / fail, and on success the name, the tags in order, the value as
a 16-digit hex bit pattern, seconds and nanoseconds.  Stored compactly: `honor` is left out when on, the time when it is the default,
and the 2 000 random cases are kept as their tokens and bit patterns alone (`random`: line i is form % (i % 7, i, token); that the
reference gave the name, the tag and the default time the form implies is asserted while the file is written).  `site` is this generator's own label of the HandleError site the case aims at
(the LC_PROM_FAIL_* name without the prefix); the reference itself only says ok or fail.
prom_unittest_vectors.json: every string literal handed to the parser in core/unittest/prometheus/TextParserUnittest.cpp's seven cases,
read as DATA and split into lines, each line with what the compiled reference gave (honor_timestamps on and off).  The expectation
text of that file is not read.
The inputs on which the reference's behaviour is UNDEFINED (a NaN timestamp: a cast of NaN; a timestamp outside int64 after the
multiplication -- except 2^63 itself, which the compiled reference fails on x86-64) are never handed to it: they form the separate
list `defined_only`, checked against include/lc_prom.h alone.
Only JSON is written; nothing compiled from the reference and none of its text is kept.  No test, build() or smoke() runs this file.
Seeded: the same cases come out every time."""
import ctypes
import json
import os
import random
import re
import struct
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("LC_REFERENCE_CORE", "/root/reference/core")
OUT = os.path.join(ROOT, "tests", "golden", "prom_reference_outputs.json")
OUT_UNIT = os.path.join(ROOT, "tests", "golden", "prom_unittest_vectors.json")
UNITTEST = os.path.join(REF, "unittest", "prometheus", "TextParserUnittest.cpp")
DEFAULT_SECS, DEFAULT_NANOS = 1700000000, 123000000
RANDOM_FORM = 'r%d{k="%d"} %s'  # (i % 7, i, token): the line of random case i

GLUE = r"""
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "models/MetricEvent.h"
#include "models/PipelineEventGroup.h"
#include "prometheus/labels/TextParser.h"
namespace logtail {
bool IsValidMetric(const StringView&) { return false; }
void SplitStringView(const std::string&, char, std::vector<StringView>&) {}
}
namespace {
void put32(std::string& o, uint32_t v) { o.append(reinterpret_cast<const char*>(&v), 4); }
void put64(std::string& o, uint64_t v) { o.append(reinterpret_cast<const char*>(&v), 8); }
void putText(std::string& o, logtail::StringView s) {
    put32(o, uint32_t(s.size()));
    o.append(s.data(), s.size());
}
}
extern "C" {
// -> malloc'ed: ok u8 | bits u64 | secs i64 | nanos u32 | has_nanos u8 | name | ntags u32 | (key, value)*; *out_len its size
char* tp_parse_line(const char* line, size_t n, int honor, unsigned long long def_secs, unsigned def_nanos, size_t* out_len) {
    logtail::PipelineEventGroup group(std::make_shared<logtail::SourceBuffer>());
    std::unique_ptr<logtail::MetricEvent> ev = group.CreateMetricEvent();
    char* copy = static_cast<char*>(std::malloc(n + 1));
    std::memcpy(copy, line, n);
    copy[n] = '\0';
    logtail::TextParser parser(honor != 0);
    parser.SetDefaultTimestamp(def_secs, def_nanos);
    const bool ok = parser.ParseLine(logtail::StringView(copy, n), *ev);
    std::string o;
    o.push_back(ok ? 1 : 0);
    uint64_t bits = 0;
    if (ok && ev->Is<logtail::UntypedSingleValue>()) std::memcpy(&bits, &ev->GetValue<logtail::UntypedSingleValue>()->mValue, 8);
    put64(o, bits);
    put64(o, uint64_t(int64_t(ev->GetTimestamp())));
    put32(o, ev->GetTimestampNanosecond() ? *ev->GetTimestampNanosecond() : 0);
    o.push_back(ev->GetTimestampNanosecond() ? 1 : 0);
    putText(o, ok ? ev->GetName() : logtail::StringView());
    put32(o, ok ? uint32_t(ev->TagsSize()) : 0);
    if (ok)
        for (auto it = ev->TagsBegin(); it != ev->TagsEnd(); ++it) {
            putText(o, it->first);
            putText(o, it->second);
        }
    char* out = static_cast<char*>(std::malloc(o.size()));
    std::memcpy(out, o.data(), o.size());
    *out_len = o.size();
    std::free(copy);
    return out;
}
}
"""


def build(tmp):
    for d in ("oracle", os.path.join("oracle", "ref_models")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, d)])
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    glue = os.path.join(tmp, "glue.cpp")
    with open(glue, "w") as f:
        f.write(GLUE)
    so = os.path.join(tmp, "libref_prom.so")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-w", "-include", "set", "-include", "memory", "-include", "unordered_set",
         "-I", os.path.join(ROOT, "oracle", "ref_models", "stubs"), "-I", os.path.join(ROOT, "tests", "refhdr"), "-I", REF, "-I", os.path.join(REF, "config"),
         "-idirafter", os.path.join(ROOT, "oracle", "ref_processor", "stubs"),  # (the boost headers StringTools.h names ...
         "-idirafter", os.path.join(ROOT, "oracle"),  # ... and the oracle header its boost/regex.hpp stands on)
         "-o", so, glue, os.path.join(REF, "prometheus", "labels", "TextParser.cpp"),
         "-Wl,-z,defs", "-Wl,-Bsymbolic", "-L" + ref_dir, "-lref_models", "-Wl,-rpath," + ref_dir])
    L = ctypes.CDLL(so)
    L.tp_parse_line.restype = ctypes.c_void_p
    L.tp_parse_line.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_uint, ctypes.POINTER(ctypes.c_size_t)]
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    return L, libc


def run(L, libc, line, honor):
    """-> {"ok": False} or {"ok": True, name, tags, bits, secs, nanos}; texts as latin-1"""
    n = ctypes.c_size_t(0)
    p = L.tp_parse_line(line, len(line), int(honor), DEFAULT_SECS, DEFAULT_NANOS, ctypes.byref(n))
    raw = ctypes.string_at(p, n.value)
    libc.free(p)
    ok, bits, secs, nanos, has = struct.unpack_from("<BQqIB", raw, 0)
    at = struct.calcsize("<BQqIB")

    def text():
        nonlocal at
        (k,) = struct.unpack_from("<I", raw, at)
        at += 4 + k
        return raw[at - k:at].decode("latin-1")
    if not ok:
        return {"ok": False}
    name = text()
    (ntags,) = struct.unpack_from("<I", raw, at)
    at += 4
    tags = [[text(), text()] for _ in range(ntags)]
    return {"ok": True, "name": name, "tags": tags, "bits": "%016x" % bits, "secs": secs, "nanos": nanos if has else None}


def cases():
    """-> [(name, line bytes, honor, site or None)]"""
    c = []

    def add(name, line, honor=True, site=None):
        c.append((name, line if isinstance(line, bytes) else line.encode("utf-8"), honor, site))
    # ---- every HandleError site, at least twice
    for i, ln in enumerate(["", "   ", "{a=\"b\"} 1", "9metric 1", "# HELP x y", "\xe9tat 1"]):
        add("site_name_%d" % i, ln, site="NAME")
    for i, ln in enumerate(["metric", "metric   ", " \tm:e_tric9 \t"]):
        add("site_name_end_%d" % i, ln, site="NAME_END")
    for i, ln in enumerate(["m{a", "m{a }", "m{a b=\"c\"} 1", "m{a:\"b\"} 1", "m{a\xc3\xa9=\"b\"} 1"]):
        add("site_equal_%d" % i, ln, site="EQUAL")
    for i, ln in enumerate(["m{", "m{ ", "m{9a=\"b\"} 1", "m{a=\"b\",,} 1", "m{\"a\"=\"b\"} 1", "m{a=\"b\", =\"c\"} 1"]):
        add("site_label_name_%d" % i, ln, site="LABEL_NAME")
    for i, ln in enumerate(["m{a=", "m{a= ", "m{a=b} 1", "m{a='b'} 1", "m{a==\"b\"} 1"]):
        add("site_quote_%d" % i, ln, site="QUOTE")
    for i, ln in enumerate(["m{a=\"b", "m{a=\"b\\\"} 1", "m{a=\"", "m{a=\"b\\", "m{a=\"\\"]):
        add("site_label_value_end_%d" % i, ln, site="LABEL_VALUE_END")
    for i, ln in enumerate(["m{a=\"b\"", "m{a=\"b\" ", "m{a=\"b\" c=\"d\"} 1", "m{a=\"b\"x} 1", "m{a=\"b\";} 1"]):
        add("site_label_value_next_%d" % i, ln, site="LABEL_VALUE_NEXT")
    for i, ln in enumerate(["m 1z", "m 1,2", "m}", "m 12_3", "m{a=\"b\"} 1}", "m 1\r", "m bar", "m 0b1"]):
        add("site_value_end_%d" % i, ln, site="VALUE_END")
    for i, ln in enumerate(["m{}", "m{} ", "m #", "m{a=\"b\"} # 1", "m +", "m 1e", "m 0x", "m infinit", "m nane", "m 1e309", "m .", "m -", "m 1.2.3", "m ee",
                            "m --1", "m 1e+", "m tya"]):
        add("site_value_%d" % i, ln, site="VALUE")
    for i, ln in enumerate(["m 1 1700000000000z", "m 1 bar", "m 1 17,5", "m 1 1700000000 000\r", "m 1 }"]):
        add("site_time_end_%d" % i, ln, site="TIME_END" if i != 3 else None)
    for i, ln in enumerate(["m 1 1e", "m 1 +", "m 1 0x", "m 1 1e999", "m 1 infinit", "m 1 ."]):
        add("site_timestamp_%d" % i, ln, site="TIMESTAMP")
    for i, ln in enumerate(["m 1 92233720368547758080000", "m 1 1e19", "m 1 9223372036854777856", "m 1 inf", "m 1 +Infinity"]):
        add("site_timestamp_overflow_%d" % i, ln, site="TIMESTAMP_OVERFLOW")
    for i, ln in enumerate(["m 1 999999999", "m 1 0", "m 1 -5", "m 1 -1700000000000", "m 1 999999999999", "m 1 1e8", "m 1 0.5"]):
        add("site_timestamp_small_%d" % i, ln, site="TIMESTAMP_SMALL")
    # ---- escapes: the meaning comes from the value's SECOND byte
    for i, v in enumerate(["a\\n", "n\\\\x", "\\\"", "an\\tb\\nc", "a\\\\n\\\"", "a\"", "xn\\q", "x\\\\\\n\\\"\\q", "x\"", "\\\\", "\\n", "\\\\\\\\", "\\nn\\n",
                           "ab\\\"cd\\\\ef\\ngh", "\\", "\\x", "n", "", "a", "a\\", "\\\"\\\"", "C:\\\\dir\\\\file", "line1\\nline2", "q\\\"uote\\\""]):
        add("escape_%d" % i, "m{a=\"%s\",b=\"plain\"} 1" % v)
    add("escape_last_byte_1", "m{a=\"x\\", site="LABEL_VALUE_END")
    add("escape_last_byte_2", "m{a=\"n\\n\\", site="LABEL_VALUE_END")
    add("escape_second_value", "m{a=\"plain\",b=\"x\\\\y\\nz\"} 1")
    add("utf8_value", "m{a=\"\u4e2d\u6587\",b=\"\u00e9\\n\u00e8\"} 1")
    add("utf8_value_2", "m{a=\"\u4e2d\\\\\u6587\"} 2")
    add("latin1_bytes", b"m{a=\"\xff\xfe\\n\x80\"} 3")
    # ---- label edge forms
    add("dup_labels", "m{a=\"1\",b=\"2\",a=\"3\"} 1")
    add("dup_labels_escaped", "m{a=\"1\",b=\"2\",a=\"x\\\\y\"} 1")
    add("name_label", "m{__name__=\"other\",a=\"1\"} 1")
    add("empty_braces", "m{} 1")
    add("blank_braces", "m{ } 1")
    add("blank_braces_tabs", "m\t{\t}\t1\t1700000000000")
    add("trailing_comma", "m{a=\"1\",} 1")
    add("trailing_comma_blank", "m{a=\"1\" , } 1")
    add("tabs_everywhere", "\t m\t{\ta\t=\t\"1\"\t,\tb\t=\t\"2\"\t}\t1.5\t1700000000123\t# x")
    add("blanks_around_equal", "m{a = \"1\" , b= \"2\",c =\"3\"} 1")
    add("colon_name", ":a:b{c=\"d\"} 1")
    add("underscore_names", "_m{_a=\"1\",_=\"2\",a9_=\"3\"} 1")
    add("value_right_behind_name_brace", "m{a=\"1\"}1")
    add("value_behind_name_no_labels", "m 1")
    add("many_labels_15", "m{%s} 1" % ",".join("l%d=\"v%d\"" % (k, k) for k in range(15)))
    add("many_labels_16", "m{%s} 1" % ",".join("l%d=\"v%d\"" % (k, k) for k in range(16)))
    add("many_labels_17", "m{%s} 1" % ",".join("l%d=\"v%d\"" % (k, k) for k in range(17)))
    add("many_labels_40_escaped_last", "m{%s,z=\"a\\nb\"} 1" % ",".join("l%d=\"v%d\"" % (k, k) for k in range(40)))
    # ---- value tokens the device decides
    two53 = 1 << 53
    for i, t in enumerate([str(two53 - 1), str(two53), str(two53 + 1), "1e-23", "1e-22", "1e22", "1e23", "9007199254740993", "0.1", ".5", "5.", "-0", "+0",
                           "0.0", "-0.0e5", "0e999", "-0e-999", "12345678901234567", "1234567890123456789", "123456789012345.67", "1.5e10", "9.9410452992e+10",
                           "1E5", "-1.25E-3", "+7", "007", "0.000001", "1e0", "9007199254740992e22", "9007199254740992e-22", "9007199254740991e23",
                           "0.9007199254740992e38", "123.456e20", "123.456e-20", "1.e2", ".1e1", "00000000000000000000001", "1." + "0" * 30, "3e+022", "3e-0022"]):
        add("value_%d" % i, "m %s" % t)
    for i, t in enumerate(["inf", "Inf", "INF", "+inf", "-inf", "-InF", "infinity", "+Infinity", "-INFINITY", "iNfInItY", "nan", "NaN", "NAN", "+nan", "-nan", "-NaN", "+nAn"]):
        add("special_%d" % i, "m %s" % t)
    # ---- value tokens the host decides
    for i, t in enumerate(["1e308", "1e309", "4.9e-324", "1e-320", "0x1A", "0x1e3", "0x", "1e", "+", "infinit", "nane", "2.2250738585072014e-308", "1.7976931348623157e308",
                           "1.7976931348623159e308", "0x1p-1", "0x.8", "-0x10", "0X1F", "1e-400", "infinityy", "nan1", "in", "na", "e5", "-e5", "i", "1ee5", "1e5e5", "1-2",
                           "179769313486231570000000000000000000000000000000000000000000", "0.30000000000000004", "2.5e-5"]):
        add("host_value_%d" % i, "m %s" % t)
    # ---- timestamps
    two31 = 1 << 31
    for i, t in enumerate([str(two31 - 1), str(two31), str(two31 + 1), "999999999", "1000000000", "1715829785083", "1715829785083.5", "1.7e12", "-1715829785083",
                           str(1 << 63), str((1 << 63) + 2048), str((1 << 63) - 1), "1715829785", "1715829785.25", "1e12", "1e9", "+1715829785083", "01715829785083",
                           "0x18F8A9C0000", str((1 << 53) - 1), str(1 << 53), str((1 << 53) + 1), "999999999999", "1000000000000", "2147483647.5", "2147483648.5"]):
        add("time_%d" % i, "m{a=\"b\"} 1 %s" % t)
    add("hash_behind_value", "m 1#comment")
    add("hash_behind_value_blank", "m 1 # 1715829785083")
    add("hash_behind_time", "m 1 1715829785083#x")
    add("text_behind_time", "m 1 1715829785083 whatever \"{")
    add("honor_off_bad_time", "m 1 bar", honor=False)
    add("honor_off_bad_time_2", "m 1 99x", honor=False)
    add("honor_off_good_time", "m 1 1715829785083", honor=False)
    add("honor_off_small_time", "m 1 5", honor=False)
    add("honor_off_bad_value", "m 1z 5", honor=False, site="VALUE_END")
    add("deferred_value_then_bad_time", "m 0x 17z", site="VALUE")
    add("deferred_value_ok_then_bad_time", "m 0x1A 17z", site="TIME_END")
    add("deferred_value_bad_then_bad_number_time", "m 0x 17x", site="VALUE")
    add("deferred_value_ok_then_small_time", "m 0x1A 17", site="TIMESTAMP_SMALL")
    add("deferred_both", "m 0x1A 1.7e12")
    add("long_name_70", "m" * 70 + "{a=\"b\"} 1")
    add("long_value_label_200", "m{a=\"%s\"} 1 1715829785083" % ("v" * 200))
    # ---- 2 000 random valid decimal tokens: 1 to 20 digits, exponents -30 to 30
    rng = random.Random(20261020)
    for i in range(2000):
        digits = "".join(rng.choice("0123456789") for _ in range(rng.randrange(1, 21)))
        if rng.random() < 0.5 and len(digits) > 1:
            at = rng.randrange(0, len(digits) + 1)
            digits = digits[:at] + "." + digits[at:]
        token = rng.choice(["", "", "-", "+"]) + digits
        if rng.random() < 0.7:
            token += rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randrange(0, 31))
        add("random_%d" % i, RANDOM_FORM % (i % 7, i, token))
    return c


def compact(entry, defaults):
    """what a reader can put back is left out: honor when it is on, the time of a parsed line when it is the default"""
    if entry.get("honor") is True:
        del entry["honor"]
    if entry["ok"] and (entry["secs"], entry["nanos"]) == (defaults["secs"], defaults["nanos"]):
        del entry["secs"], entry["nanos"]
    return entry


def defined_only():
    """inputs the compiled reference is never asked about (undefined there; include/lc_prom.h defines them)"""
    return [{"name": "nan_timestamp", "line": "m 1 nan", "honor": True, "status": "TIMESTAMP_NAN"},
            {"name": "nan_timestamp_signed", "line": "m{a=\"b\"} 2 -NaN", "honor": True, "status": "TIMESTAMP_NAN"},
            {"name": "timestamp_minus_inf", "line": "m 1 -inf", "honor": True, "status": "TIMESTAMP_SMALL"},
            {"name": "timestamp_minus_1e30", "line": "m 1 -1e30", "honor": True, "status": "TIMESTAMP_SMALL"}]


def unittest_lines():
    """the string literals of the seven cases' bodies, expectation lines (APSARA_TEST_*) left out, as lines -> [(case, line bytes)]"""
    src = open(UNITTEST, encoding="utf-8").read()
    out = []
    bodies = re.findall(r"void TextParserUnittest::(\w+)\(\)[^{]*\{(.*?)\nUNIT_TEST_CASE", src, re.S)
    literal = re.compile(r'R"([^()\s\\]{0,16})\((.*?)\)\1"|"((?:[^"\\\n]|\\.)*)"', re.S)
    for case, body in bodies:
        body = "\n".join(ln for ln in body.split("\n") if "APSARA_TEST" not in ln)
        for m in literal.finditer(body):
            if m.group(2) is not None:
                text = m.group(2)
            else:
                text = m.group(3).encode("utf-8").decode("unicode_escape").encode("latin-1").decode("utf-8", "replace")
            for ln in text.split("\n"):
                out.append((case, ln.encode("utf-8")))
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        L, libc = build(tmp)
        undefined = {d["line"] for d in defined_only()}
        ref = {"defaults": {"secs": DEFAULT_SECS, "nanos": DEFAULT_NANOS}, "cases": [], "random": {"form": RANDOM_FORM, "tokens": [], "bits": []},
               "defined_only": defined_only()}
        for name, line, honor, site in cases():
            text = line.decode("latin-1")
            assert text not in undefined, name
            entry = {"id": name, "line": text, "honor": honor}
            if site:
                entry["site"] = site
            entry.update(run(L, libc, line, honor))
            assert not (site and entry["ok"]), (name, "aimed at a failure site and parsed")
            if name.startswith("random_"):
                # stored as token and bits alone: everything else of the result is what the line's form says, checked here
                i = len(ref["random"]["tokens"])
                assert name == "random_%d" % i and text == RANDOM_FORM % (i % 7, i, text.rsplit(" ", 1)[1]) and honor
                assert entry["ok"] and entry["name"] == "r%d" % (i % 7) and entry["tags"] == [["k", str(i)]], name
                assert (entry["secs"], entry["nanos"]) == (DEFAULT_SECS, DEFAULT_NANOS), name
                ref["random"]["tokens"].append(text.rsplit(" ", 1)[1])
                ref["random"]["bits"].append(entry["bits"])
                continue
            ref["cases"].append(compact(entry, ref["defaults"]))
        n_random = len(ref["random"]["tokens"])
        ref["random"]["tokens"] = " ".join(ref["random"]["tokens"])
        ref["random"]["bits"] = "".join(ref["random"]["bits"])
        unit = {"defaults": ref["defaults"], "cases": []}
        seen = set()
        for case, line in unittest_lines():
            for honor in (True, False):
                if (case, line, honor) in seen or line.decode("latin-1") in undefined:
                    continue
                seen.add((case, line, honor))
                entry = {"case": case, "line": line.decode("latin-1"), "honor": honor}
                entry.update(run(L, libc, line, honor))
                unit["cases"].append(compact(entry, unit["defaults"]))
    for path, doc in ((OUT, ref), (OUT_UNIT, unit)):
        with open(path, "w") as f:
            json.dump(doc, f, separators=(",", ":"), ensure_ascii=True)
            f.write("\n")
    print("%d cases (%d ok) and %d random tokens, %d unit-test lines from %d cases" % (len(ref["cases"]), sum(e["ok"] for e in ref["cases"]), n_random, len(unit["cases"]),
                                                               len({e["case"] for e in unit["cases"]})))


if __name__ == "__main__":
    main()
