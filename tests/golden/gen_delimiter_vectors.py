"""Writes tests/golden/delimiter_reference_outputs.json: the output of the REFERENCE's OWN processor_parse_delimiter_native.

    python tests/golden/gen_delimiter_vectors.py          (needs the reference tree and a built oracle/_ref; CPU only)

ProcessorParseDelimiterNative.cpp + DelimiterModeFsmParser.cpp are compiled, where they lie in the reference tree, into a TEMPORARY
directory against oracle/_ref/libref_processor.so / libref_models.so (CommonParserOptions, ParamExtractor, Processor.cpp, the event
model, the agent shims and the fixture reader / writer are in there), driven over generated event groups, and what comes out is
recorded: per case the config, the input lines, the surviving events' contents in order, the four plugin counters and the alarm
texts; and for a list of configs what its Init answers (accepted or not, the alarm texts it raises).  The same run writes
tests/golden/delimiter_unittest_vectors.json: the cases of core/unittest/processor/ProcessorParseDelimiterNativeUnittest.cpp read as DATA
(each sub-case's config assignments, input and expected fixture JSON, asserted counters); where a case runs splitters or the merge
processor first, the group is recorded as the delimiter processor receives it (the reference's own splitters, from
oracle/_ref/libref_processor.so, make it), and every case's expectation is checked against the reference's own processor while it is
written.  Only the JSON is written; nothing compiled from the reference and none of its text is kept.  No test, build() or smoke() runs
this file.  Seeded: the same file comes out every time."""
import ctypes
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("LC_REFERENCE_CORE", "/root/reference/core")
OUT = os.path.join(ROOT, "tests", "golden", "delimiter_reference_outputs.json")
OUT_UNIT = os.path.join(ROOT, "tests", "golden", "delimiter_unittest_vectors.json")
UNITTEST = os.path.join(REF, "unittest", "processor", "ProcessorParseDelimiterNativeUnittest.cpp")

GLUE = r"""
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
// (everything the processor's header includes comes in first, untouched: only the class itself is opened up, for its counters)
#include "collection_pipeline/plugin/interface/Processor.h"
#include "models/LogEvent.h"
#include "parser/DelimiterModeFsmParser.h"
#include "plugin/processor/CommonParserOptions.h"
#define private public
#define protected public
#include "plugin/processor/ProcessorParseDelimiterNative.h"
#undef private
#undef protected
bool hdGroupFromJson(logtail::PipelineEventGroup& group, const std::string& json, std::string* error);
std::string hdGroupToJson(const logtail::PipelineEventGroup& group);
namespace {
struct Handle {
    logtail::CollectionPipelineContext ctx;
    logtail::ProcessorParseDelimiterNative proc;
};
}
extern "C" {
void* rd_create(const char* config_json) {
    Handle* h = new Handle;
    h->ctx.SetConfigName("test_config");
    h->proc.SetContext(h->ctx);
    Json::Value config = Json::Value::fromText(config_json);
    if (!h->proc.Init(config)) {
        delete h;
        return nullptr;
    }
    return h;
}
void rd_destroy(void* h) { delete static_cast<Handle*>(h); }
char* rd_process(void* h, const char* group_json) {
    std::vector<logtail::PipelineEventGroup> groups;
    groups.emplace_back(std::make_shared<logtail::SourceBuffer>());
    std::string error;
    if (!hdGroupFromJson(groups[0], group_json, &error)) return nullptr;
    static_cast<logtail::Processor&>(static_cast<Handle*>(h)->proc).Process(groups);
    return strdup(hdGroupToJson(groups[0]).c_str());
}
void rd_counters(void* h, unsigned long long out[4]) {
    auto& p = static_cast<Handle*>(h)->proc;
    out[0] = p.mDiscardedEventsTotal->GetValue();
    out[1] = p.mOutFailedEventsTotal->GetValue();
    out[2] = p.mOutKeyNotFoundEventsTotal->GetValue();
    out[3] = p.mOutSuccessfulEventsTotal->GetValue();
}
}
"""


def build(tmp):
    for d in ("oracle", os.path.join("oracle", "ref_models"), os.path.join("oracle", "ref_processor")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, d)])
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    glue = os.path.join(tmp, "glue.cpp")
    with open(glue, "w") as f:
        f.write(GLUE)
    so = os.path.join(tmp, "libref_delimiter.so")
    stubs = os.path.join(ROOT, "oracle", "ref_processor", "stubs")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-w", "-include", "set", "-include", "memory", "-I", stubs, "-I", os.path.join(ROOT, "oracle"),
         "-I", os.path.join(ROOT, "tests", "refhdr"), "-I", REF, "-I", os.path.join(REF, "config"), "-o", so, glue,
         os.path.join(REF, "plugin", "processor", "ProcessorParseDelimiterNative.cpp"), os.path.join(REF, "parser", "DelimiterModeFsmParser.cpp"),
         "-L" + ref_dir, "-lref_processor", "-lref_models", "-Wl,-rpath," + ref_dir, "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    L = ctypes.CDLL(so)
    L.rd_create.restype = ctypes.c_void_p
    L.rd_create.argtypes = [ctypes.c_char_p]
    L.rd_destroy.argtypes = [ctypes.c_void_p]
    L.rd_process.restype = ctypes.c_void_p
    L.rd_process.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    L.rd_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
    P = ctypes.CDLL(os.path.join(ref_dir, "libref_processor.so"))
    P.refp_take_alarms.restype = ctypes.c_void_p
    P.refp_free.argtypes = [ctypes.c_void_p]
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    return L, P, libc


PRE_KINDS = {"ProcessorSplitLogStringNative": "processor_split_string_native",
             "ProcessorSplitMultilineLogStringNative": "processor_split_multiline_log_string_native",
             "ProcessorMergeMultilineLogNative": "processor_merge_multiline_log_native"}
INIT_CONFIGS = [
    {"SourceKey": "content", "Separator": "\\t", "Keys": ["a"]},
    {"SourceKey": "content", "Separator": "@@@@", "Keys": ["a"]},
    {"SourceKey": "content", "Separator": "@@", "Quote": "'", "Keys": ["a"]},
    {"SourceKey": "content", "Separator": ",", "Quote": 3, "Keys": ["a"]},
    {"SourceKey": "content", "Separator": ",", "Quote": "", "Keys": ["a"]},
    {"SourceKey": "content", "Separator": ",", "Keys": ["a"], "OverflowedFieldsTreatment": "explode"},
    {"SourceKey": "content", "Separator": ",", "Keys": ["a"], "OverflowedFieldsTreatment": 1},
    {"SourceKey": "content", "Separator": ",", "Keys": ["a"], "AllowingShortenedFields": "yes"},
    {"SourceKey": "content", "Separator": ",", "Keys": ["a"], "KeepingSourceWhenParseFail": "yes", "CopingRawLog": 1, "RenamedSourceKey": 2},
    {"Separator": ",", "Keys": ["a"]},
    {"SourceKey": "", "Separator": ",", "Keys": ["a"]},
    {"SourceKey": 5, "Separator": ",", "Keys": ["a"]},
    {"SourceKey": "content", "Keys": ["a"]},
    {"SourceKey": "content", "Separator": "", "Keys": ["a"]},
    {"SourceKey": "content", "Separator": 1, "Keys": ["a"]},
    {"SourceKey": "content", "Separator": "@@@@@", "Keys": ["a"]},
    {"SourceKey": "content", "Separator": ",", "Quote": "''", "Keys": ["a"]},
    {"SourceKey": "content", "Separator": ","},
    {"SourceKey": "content", "Separator": ",", "Keys": "a"},
    {"SourceKey": "content", "Separator": ",", "Keys": []},
    {"SourceKey": "content", "Separator": ",", "Keys": ["a", 1]},
]


def _value(text):
    """a C++ literal of the unit test's config assignments as a JSON value"""
    text = text.strip()
    if text in ("true", "false"):
        return text == "true"
    if text == "Json::arrayValue":
        return []
    if text.startswith("'"):
        return ord(text[1:-1].encode().decode("unicode_escape"))       # (a char becomes an integer in a Json::Value)
    if text.startswith('"'):
        return text[1:-1].encode().decode("unicode_escape")
    return int(text)


def read_unittest():
    """-> [{name, config, pre: [(kind, config)], in: fixture text, expect: fixture text, asserted: {member: value}}], [init-only configs]"""
    import copy
    import re
    with open(UNITTEST, encoding="utf-8") as f:
        text = f.read()
    cases, init_only = [], []
    raw = {}
    config, delim_config, pre_vars, chain, group_in, name, sub, count = {}, None, {}, [], None, None, 0, None
    processed = False
    pos = 0
    token = re.compile(
        r'void ProcessorParseDelimiterNativeUnittest::(\w+)\(\)|std::string (inJson|expectJson) = R"\((.*?)\)";|Json::Value config;|'
        r'config\["(\w+)"\](?:\["(\w+)"\])? = ([^;]+);|config\["(\w+)"\]\.append\(("[^"]*")\);|'
        r'(ProcessorSplitLogStringNative|ProcessorSplitMultilineLogStringNative|ProcessorMergeMultilineLogNative) (\w+);|'
        r'FromJsonString\(inJson\)|Init\(config, mContext\)|(\w+)\.Process\((\w+)\)|APSARA_TEST_STREQ_FATAL\((?:CompactJson\(expectJson\)|"null")|'
        r'ProcessorParseDelimiterNative& (\w+) =|int count = (\d+);|APSARA_TEST_EQUAL_FATAL\(uint64_t\((\w+)\), (\w+)\.(m\w+)->GetValue\(\)\)', re.S)

    def close_function():
        if name and delim_config is not None and not processed and not any(c["name"].startswith(name) for c in cases):
            init_only.append({"name": name, "config": delim_config})

    for m in token.finditer(text):
        t = m.group(0)
        if m.group(1):
            close_function()
            name, sub, config, delim_config, pre_vars, chain, group_in, count, processed = m.group(1), 0, {}, None, {}, [], None, None, False
            raw = {}
        elif m.group(2):
            raw[m.group(2)] = m.group(3)
        elif t == "Json::Value config;":
            config = {}
        elif m.group(4):
            if m.group(5):
                config.setdefault(m.group(4), {})[m.group(5)] = _value(m.group(6))
            else:
                config[m.group(4)] = _value(m.group(6))
        elif m.group(7):
            config[m.group(7)].append(_value(m.group(8)))
        elif m.group(9):
            pre_vars[m.group(10)] = PRE_KINDS[m.group(9)]
        elif t == "FromJsonString(inJson)":
            group_in, chain = raw["inJson"], []
        elif t == "Init(config, mContext)":
            delim_config = copy.deepcopy(config)
        elif m.group(11):
            if m.group(11) in pre_vars:
                chain.append((pre_vars[m.group(11)], copy.deepcopy(config)))
            else:
                processed = True
        elif t.startswith("APSARA_TEST_STREQ_FATAL"):
            sub += 1
            expect = "{}" if '"null"' in t else raw["expectJson"]      # (an emptied group prints as null)
            cases.append({"name": "%s/%d" % (name, sub), "config": delim_config, "pre": chain, "in": group_in, "expect": expect,
                          "asserted": {}})
        elif m.group(13):
            pre_vars.pop(m.group(13), None)              # (the name now means the delimiter processor)
        elif m.group(14):
            count = int(m.group(14))
        elif m.group(15):
            v = count if m.group(15) == "count" else int(m.group(15))
            cases[-1]["asserted"][m.group(17)] = v
    close_function()
    return cases, init_only


def lines_for(S, q, rng, wide):
    """the ingredients of the issue's list for separator S and quote q"""
    out = [
        "x1%sy2%sz3" % (S, S),                                       # exact
        "only", "p%sq" % S,                                          # too few
        S.join("c%d" % i for i in range(5)),                         # too many
        "%s%s" % (S, S), "a%s%sc" % (S, S), "a%sb%s" % (S, S),       # empty columns, a trailing separator
        "  a%sb%sc  \r" % (S, S), " \r ", "", "   ", "a%s b %sc\r\r" % (S, S),   # blanks and \r
        "%sa%sb%s%sc%sd" % (q, S, q, S, S),                          # a quoted field with a separator
        "%she said %s%shi%s%s%s%sb%sc" % (q, q, q, q, q, q, S, S),   # doubled quotes
        "ab%sc%sd%se" % (q, S, S),                                   # a lone inner quote
        "%sabc%sd" % (q, S),                                         # an unterminated quote
        "%sab%sx%sc" % (q, q, S),                                    # data after a closing quote
        "%s%s%sb%sc" % (q, q, S, S),                                 # a quoted empty field
        "a%sb%sc%s%sd%s%se%s%s%sf%sg%s" % (S, S, S, q, q, q, q, S, q, S, q),   # overflow with quotes in it (the keep re-join)
        S[:1], S, S + S[:1], "a" + S[:-1] + "b" if len(S) > 1 else "a" + S,    # the separator itself, shorter than it, a partial one
    ]
    if wide:
        out.append(S.join("w%d" % i for i in range(40)))
        out.append(S.join("%sv%d%s" % (q, i, q) for i in range(23)))
    alphabet = ["a", "b", " ", S, S, q, "\r", S[:1]]
    for _ in range(3):
        out.append("".join(rng.choice(alphabet) for _ in range(rng.randint(1, 14))))
    return out


def main():
    rng = random.Random(20261016)
    cases = []
    seps = [(",", ['"', "'", ","]), ("|", ['"', "'", "|"]), ("\t", ['"', "'", "\t"]), ("||", ['"']), ("@@@@", ["'"])]
    modes = ["extend", "keep", "discard"]
    keeps = [(False, False), (False, True), (True, False), (True, True)]
    key_sets = [["a", "b", "c"], ["a", "content", "c"], ["a", "_", "c"]]
    n = 0
    # every separator / quote with every mode and AllowingShortenedFields; the source-key policy and the key sets rotate
    for S, quotes in seps:
        for q in quotes:
            for mode in modes:
                for short in (False, True):
                    kf, ks = keeps[n % 4]
                    config = {"SourceKey": "content", "Separator": "\\t" if S == "\t" and n % 2 else S, "Quote": q, "Keys": key_sets[(n // 2) % 3],
                              "AllowingShortenedFields": short, "OverflowedFieldsTreatment": mode, "KeepingSourceWhenParseFail": kf,
                              "KeepingSourceWhenParseSucceed": ks}
                    if n % 5 == 0:
                        config["RenamedSourceKey"] = "raw"
                    if n % 7 == 0:
                        config["CopingRawLog"] = True
                    cases.append((config, lines_for(S, q, rng, n % 11 == 0)))
                    n += 1
    # the whole policy cross on one separator, few lines
    for mode in modes:
        for short in (False, True):
            for kf, ks in keeps:
                for keys in key_sets:
                    config = {"SourceKey": "content", "Separator": ",", "Keys": keys, "AllowingShortenedFields": short,
                              "OverflowedFieldsTreatment": mode, "KeepingSourceWhenParseFail": kf, "KeepingSourceWhenParseSucceed": ks}
                    cases.append((config, ["1,2,3", "1,2", "1,2,3,4,5", '"1,1",2', 'a"b,c', "  ", '1,2,3,"4""4",5']))
    with tempfile.TemporaryDirectory() as tmp:
        L, P, libc = build(tmp)
        out_cases = []
        for config, lines in cases:
            h = L.rd_create(json.dumps(config).encode())
            assert h, config
            P.refp_free(P.refp_take_alarms())
            events = [{"contents": [["content", ln]], "timestamp": 1, "type": 1} for ln in lines]
            events.append({"contents": [["other", "x"]], "timestamp": 1, "type": 1})
            p = L.rd_process(h, json.dumps({"events": events}).encode())
            assert p
            got = json.loads(ctypes.string_at(p).decode("utf-8"), object_pairs_hook=list)
            libc.free(p)
            c = (ctypes.c_ulonglong * 4)()
            L.rd_counters(h, c)
            a = P.refp_take_alarms()
            alarms = [m for _, _, m in json.loads(ctypes.string_at(a).decode("utf-8"))]
            P.refp_free(a)
            L.rd_destroy(h)
            out_events = [dict(ev).get("contents", []) for ev in dict(got or []).get("events", [])]
            out_cases.append({"config": config, "lines": lines, "out": out_events, "counters": [int(x) for x in c], "alarms": alarms})
        # ---- what the reference's Init answers
        init = []
        for config in INIT_CONFIGS:
            P.refp_free(P.refp_take_alarms())
            h = L.rd_create(json.dumps(config).encode())
            a = P.refp_take_alarms()
            alarms = [m for _, _, m in json.loads(ctypes.string_at(a).decode("utf-8"))]
            P.refp_free(a)
            init.append({"config": config, "ok": bool(h), "alarms": alarms})
            if h:
                L.rd_destroy(h)
        # ---- the unit test's cases, as data
        P.refp_create_kind.restype = ctypes.c_void_p
        P.refp_create_kind.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        P.refp_process_chain4_json.restype = ctypes.c_void_p
        P.refp_process_chain4_json.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        unit_cases, init_only = read_unittest()
        unit_out = []
        for case in unit_cases:
            group = json.loads(case["in"], strict=False)
            if case["pre"]:
                err = ctypes.create_string_buffer(512)
                hs = [P.refp_create_kind(kind.encode(), json.dumps(cfg).encode(), err, 512) for kind, cfg in case["pre"]]
                assert all(hs), (case["name"], err.value)
                hs += [None] * (4 - len(hs))
                p = P.refp_process_chain4_json(hs[0], hs[1], hs[2], hs[3], json.dumps(group).encode(), err, 512)
                assert p, err.value
                group = json.loads(ctypes.string_at(p).decode("utf-8"), object_pairs_hook=list)
                P.refp_free(p)
                group = dict(group)
                group["events"] = [dict(ev) for ev in group.get("events", [])]
            for ev in group.get("events", []):
                ev.pop("fileOffset", None)               # (the splitters' positions: the unit test's expectations do not carry them)
                ev.pop("rawSize", None)
            for ev in group.get("events", []):           # contents as an ordered list of pairs (an object is applied in key order)
                c = ev.get("contents", {})
                ev["contents"] = [list(kv) for kv in (sorted(c.items()) if isinstance(c, dict) else c)]
            expect = json.loads(case["expect"], strict=False)
            # the cross-check: the reference's own processor on the recorded group gives the unit test's expectation
            h = L.rd_create(json.dumps(case["config"]).encode())
            assert h, case["name"]
            P.refp_free(P.refp_take_alarms())
            p = L.rd_process(h, json.dumps(group).encode())
            assert p, case["name"]
            got = json.loads(ctypes.string_at(p).decode("utf-8")) or {}
            libc.free(p)
            c = (ctypes.c_ulonglong * 4)()
            L.rd_counters(h, c)
            a = P.refp_take_alarms()
            alarms = [m for _, _, m in json.loads(ctypes.string_at(a).decode("utf-8"))]
            P.refp_free(a)
            L.rd_destroy(h)
            for ev in got.get("events", []) + expect.get("events", []):
                ev.setdefault("timestampNanosecond", 0)
            agrees = got.get("events", []) == expect.get("events", [])
            if not agrees:
                print("FINDING: %s: the reference's own output differs from the unit test's expectation" % case["name"], file=sys.stderr)
            unit_out.append({"name": case["name"], "config": case["config"], "chained_behind": [k for k, _ in case["pre"]], "in": group,
                             "expect": expect, "asserted": case["asserted"], "reference_counters": [int(x) for x in c],
                             "reference_alarms": alarms, "reference_agrees": agrees})
        unit_doc = {"_about": "the cases of core/unittest/processor/ProcessorParseDelimiterNativeUnittest.cpp as data (tests/golden/"
                              "gen_delimiter_vectors.py): config, the group as the delimiter processor receives it (contents as ordered pairs), "
                              "the expected group, the counters the test asserts (by member name); reference_counters / reference_alarms: "
                              "what the reference's own processor gave on that group when the file was written (discarded, out_failed, "
                              "out_key_not_found, out_successful); init_only: configs the test only initialises; init: what the reference's "
                              "own Init answers for a config -- accepted or not, and the alarm texts it raises",
                    "cases": unit_out, "init_only": init_only, "init": init}
        with open(OUT_UNIT, "w", encoding="utf-8") as f:
            json.dump(unit_doc, f, ensure_ascii=True, separators=(",", ":"))
            f.write("\n")
        print("%d unit-test sub-cases (%d functions) + %d init-only, %d bytes -> %s" % (
            len(unit_out), len({c["name"].split("/")[0] for c in unit_out}), len(init_only), os.path.getsize(OUT_UNIT),
            os.path.relpath(OUT_UNIT, ROOT)), file=sys.stderr)
    doc = {"_about": "output of the reference's own processor_parse_delimiter_native (tests/golden/gen_delimiter_vectors.py); every group "
                     "is its lines as {content: line} events plus one event {other: x}; out = the contents of the events left, in order; "
                     "counters = discarded, out_failed, out_key_not_found, out_successful; init = what the reference's Init answers for a "
                     "config: accepted or not, and the alarm texts it raises",
           "cases": out_cases}
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(doc, f, ensure_ascii=True, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d bytes -> %s" % (len(out_cases), os.path.getsize(OUT), os.path.relpath(OUT, ROOT)), file=sys.stderr)


if __name__ == "__main__":
    main()
