"""Writes tests/golden/apsara_reference_outputs.json and apsara_unittest_vectors.json: the output of the REFERENCE's OWN
processor_parse_apsara_native.

    python tests/golden/gen_apsara_vectors.py          (needs the reference tree and a built oracle/_ref; CPU only)

ProcessorParseApsaraNative.cpp, common/TimeUtil.cpp and common/Strptime.cpp are compiled, where they lie in the reference tree, into a
TEMPORARY directory against oracle/_ref/libref_processor.so / libref_models.so, with a small driver that also defines the two discard
flags (common/LogtailCommonFlags.cpp pulls in the whole agent).  The driver runs generated event groups through the processor under
TZ=UTC, CST-8 and EST5EDT,M3.2.0,M11.1.0 and what comes out is recorded: per case the config, the input lines, the events left
(contents in order, timestamp seconds and nanoseconds), the five plugin counters and the alarm texts.  The outputs are clock-free:
ilogtail_discard_old_data is off except in the discard cases, whose times lie decades in the past or in 2090; Timezone is resolved by
the reference against the wall clock of the run (`now` is recorded: a replay hands it to the product as its clock).
The same run writes apsara_unittest_vectors.json: the cases of core/unittest/processor/ProcessorParseApsaraNativeUnittest.cpp that are
written as inJson / expectJson pairs, read as DATA, each checked against the compiled reference while the file is written, and `init`:
configs with what the reference's Init answers.  Only JSON is written; nothing compiled from the reference and none of its text is
kept.  No test, build() or smoke() runs this file.  Seeded: the same cases come out every time."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("LC_REFERENCE_CORE", "/root/reference/core")
OUT = os.path.join(ROOT, "tests", "golden", "apsara_reference_outputs.json")
OUT_UNIT = os.path.join(ROOT, "tests", "golden", "apsara_unittest_vectors.json")
UNITTEST = os.path.join(REF, "unittest", "processor", "ProcessorParseApsaraNativeUnittest.cpp")
ZONES = ["UTC", "CST-8", "EST5EDT,M3.2.0,M11.1.0"]

GLUE = r"""
#include <cstdlib>
#include <cstring>
#include <strings.h>
#include <string>
#include <vector>
#include "collection_pipeline/plugin/interface/Processor.h"
#include "common/Flags.h"
#include "models/LogEvent.h"
#include "plugin/processor/CommonParserOptions.h"
#define private public
#define protected public
#include "plugin/processor/ProcessorParseApsaraNative.h"
#undef private
#undef protected
DEFINE_FLAG_BOOL(ilogtail_discard_old_data, "if discard the old data flag", true);
DEFINE_FLAG_INT32(ilogtail_discard_interval, "if the data is old than the interval, it will be discard", 43200);
bool hdGroupFromJson(logtail::PipelineEventGroup& group, const std::string& json, std::string* error);
std::string hdGroupToJson(const logtail::PipelineEventGroup& group);
// common/StringTools.cpp is not compiled (oracle/ref_processor/shims.cpp says why): the one function of it Strptime.cpp calls
namespace logtail {
int CStringNCaseInsensitiveCmp(const char* s1, const char* s2, size_t n) { return strncasecmp(s1, s2, n); }
}
namespace {
struct Handle {
    logtail::CollectionPipelineContext ctx;
    logtail::ProcessorParseApsaraNative proc;
};
}
extern "C" {
void ra_set_discard(int on) { FLAGS_ilogtail_discard_old_data = on != 0; }
void* ra_create(const char* config_json) {
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
void ra_destroy(void* h) { delete static_cast<Handle*>(h); }
int ra_zone_offset(void* h) { return static_cast<Handle*>(h)->proc.mLogTimeZoneOffsetSecond; }
char* ra_process(void* h, const char* group_json) {
    std::vector<logtail::PipelineEventGroup> groups;
    groups.emplace_back(std::make_shared<logtail::SourceBuffer>());
    std::string error;
    if (!hdGroupFromJson(groups[0], group_json, &error)) return nullptr;
    static_cast<logtail::Processor&>(static_cast<Handle*>(h)->proc).Process(groups);
    return strdup(hdGroupToJson(groups[0]).c_str());
}
void ra_counters(void* h, unsigned long long out[5]) {
    auto& p = static_cast<Handle*>(h)->proc;
    out[0] = p.mDiscardedEventsTotal->GetValue();
    out[1] = p.mOutFailedEventsTotal->GetValue();
    out[2] = p.mOutKeyNotFoundEventsTotal->GetValue();
    out[3] = p.mOutSuccessfulEventsTotal->GetValue();
    out[4] = p.mHistoryFailureTotal->GetValue();
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
    # what the three sources expect their includes to have brought along (a complete sls_logs::Log for SetLogTime, struct stat for
    # ReadUtmp, the logger macros): this file's own text, forced in front of every translation unit
    pre = os.path.join(tmp, "pre.h")
    with open(pre, "w") as f:
        f.write("#pragma once\n#include <sys/stat.h>\n#include <cstdint>\n"
                "namespace sls_logs { class Log { public: void set_time(uint32_t) {} void set_time_ns(uint32_t) {} }; }\n"
                '#include "logger/Logger.h"\n')
    so = os.path.join(tmp, "libref_apsara.so")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-w", "-include", "set", "-include", "memory", "-include", pre,
         "-I", os.path.join(ROOT, "oracle", "ref_processor", "stubs"), "-I", os.path.join(ROOT, "oracle"),
         "-I", os.path.join(ROOT, "tests", "refhdr"), "-I", REF, "-I", os.path.join(REF, "config"),
         "-idirafter", os.path.join(ROOT, "oracle", "ref_models", "stubs"),  # (gflags/gflags.h alone; its other stubs stay behind the real headers)
         "-o", so, glue, os.path.join(REF, "plugin", "processor", "ProcessorParseApsaraNative.cpp"),
         os.path.join(REF, "common", "TimeUtil.cpp"), os.path.join(REF, "common", "Strptime.cpp"),
         "-Wl,-z,defs", "-L" + ref_dir, "-lref_processor", "-lref_models", "-Wl,-rpath," + ref_dir, "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    L = ctypes.CDLL(so)
    L.ra_create.restype = ctypes.c_void_p
    L.ra_create.argtypes = [ctypes.c_char_p]
    L.ra_destroy.argtypes = [ctypes.c_void_p]
    L.ra_zone_offset.argtypes = [ctypes.c_void_p]
    L.ra_process.restype = ctypes.c_void_p
    L.ra_process.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    L.ra_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
    P = ctypes.CDLL(os.path.join(ref_dir, "libref_processor.so"))
    P.refp_take_alarms.restype = ctypes.c_void_p
    P.refp_free.argtypes = [ctypes.c_void_p]
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    return L, P, libc


UNIT_LINES_RE = re.compile(r'const char\* logLine\[\] = \{(.*?)\n    \};', re.S)


def unittest_lines():
    """the 31 lines of TestApsaraLogLineParser, read from the unit test as data"""
    with open(UNITTEST, encoding="utf-8") as f:
        text = f.read()
    body = UNIT_LINES_RE.search(text).group(1)
    lines = []
    for entry in re.split(r',\s*//\s*\d+\s*\n|\s*//\s*31\s*$', body):
        parts = re.findall(r'"((?:[^"\\]|\\.)*)"', entry)
        if parts or entry.strip():
            lines.append("".join(parts).encode().decode("unicode_escape"))
    assert len(lines) == 31, len(lines)
    return lines


def unittest_cases():
    """the test functions written as inJson / expectJson: -> [{name, config, in, expect}]"""
    with open(UNITTEST, encoding="utf-8") as f:
        text = f.read()
    cases = []
    token = re.compile(r'void ProcessorParseApsaraNativeUnittest::(\w+)\(\)|std::string (inJson|expectJson|outJson) = R"\((.*?)\)";|'
                       r'Json::Value config;|config\["(\w+)"\] = ([^;]+);|APSARA_TEST_STREQ_FATAL\(CompactJson\(expectJson\)', re.S)
    name, config, raw, sub = None, {}, {}, 0
    for m in token.finditer(text):
        t = m.group(0)
        if m.group(1):
            name, config, raw, sub = m.group(1), {}, {}, 0
        elif m.group(2):
            raw[m.group(2)] = m.group(3)
        elif t == "Json::Value config;":
            config = {}
        elif m.group(4):
            v = m.group(5).strip()
            config[m.group(4)] = v == "true" if v in ("true", "false") else v[1:-1].encode().decode("unicode_escape") if v.startswith('"') else int(v)
        elif t.startswith("APSARA_TEST_STREQ_FATAL") and "inJson" in raw and "expectJson" in raw:
            sub += 1
            cases.append({"name": "%s/%d" % (name, sub), "config": dict(config), "in": raw["inJson"], "expect": raw["expectJson"]})
    return cases


BASE4 = "\t[INFO]\t[385658]\t[src/core/worker.cpp:215]"
D = "[2013-03-13 18:05:09.493309]"


def case_lines(rng):
    """(name, [lines]) groups: the issue's list"""
    groups = []
    groups.append(("unit_lines", unittest_lines()))
    t = []
    for digits in ("1378972170", "1378972171093", "1378972170425093", "1378972170425093123"):
        t += ["[%s]\tA:B" % digits, "[%s]" % digits, "[%s]\t[INFO]\tk:v" % digits]
    t += ["[1x]\tA:B", "[1]\tA:B", "[1378972170 ]\tA:B", "[1378972170", "[2013-03-13 18:05:09.493309\tA:B", "[", "[]", "[]\tA:B", "x",
          "[2013-03-13 18:0]5:09]\tA:B", "[2013-03]\tA:B", "[1969-12-31 23:59:59.5]\tA:B", "[1970-01-01 00:00:00]\tA:B",
          "[1970-01-01 00:00:01]\tA:B", "[1901-01-01 00:00:01]\tA:B", "[2013-03-13 18:05:09.x]\tA:B", "[2013-03-13 18:05:09x123]\tA:B",
          "[2013-03-13 18:05:09]\tA:B", "[2013-03-13 18:05:09]5\tA:B", "[2013-03-13 18:05:09.1234567891]\tA:B",
          "[2013-03-13 18:05:09.123456789012]\tA:B", "[2013-03-13 18:05:09.5]\tA:B", "[2013-02-30 18:05:09.5]\tA:B",
          "[2013-13-13 18:05:09.5]\tA:B", "[2013-03-13 24:05:09]\tA:B", "[2013-03-13 18:05:61]\tA:B", "[2013-03-13T18:05:09]\tA:B",
          "[2013-03-10 02:30:00.25]\tA:B", "[2013-11-03 01:30:00.25]\tA:B", "[2090-06-01 12:00:00.000001]\tA:B", "[9999999999]\tA:B"]
    groups.append(("time_forms", t))
    groups.append(("cache_equal_seconds", [D + "\tn:%d" % i for i in range(3)] + ["[2013-03-13 18:05:10.1]\tn:3", "[2013-03-13 18:05:10.2]\tn:4",
                                           "[2013-03-13 18:05:10]\tn:5", "[2013-03-13 18:05:10", "[2013-03-13 18:05:10.7]\tn:6"]))
    groups.append(("cache_fail_and_epoch_between", [D + "\tn:0", "garbage", "[1378972170425093]\tn:1", "[2013-03-13 18:05:0x]\tn:2", D + "\tn:3",
                                                    "[2013-03-13 18:05:09.7]\tn:4"]))
    groups.append(("cache_observable_one_digit", [D + "\tn:0", "[2013-3-13 8:5:9.25]\tlonger:tail\tn:1", "[2013-3-13 8:5:9.25]\tlonger:tail\tn:2",
                                                  "[2013-3-13 8:5:9.75]\tlonger:tail\tn:3", "[2013-3-13 8:5:9.25]\tlonger:tailx\tn:4", D + "\tn:5",
                                                  D + "\tn:6"]))
    groups.append(("cache_observable_blanks", [D + "\tn:0", "[2013-03-13  18:05:09.25]\tn:1", "[2013-03-13  18:05:07.5]\tn:2",
                                               "[2013-03-13  18:05:0]\tn:3", "[2013-03-13   18:05:09.25]\tn:4", "[2013-03-13   18:05:09.5]\tn:5",
                                               "[2013-03-13          18:05:09]\tn:6", "[2013-03-13         x]\tn:7", D + "\tn:8",
                                               "[12013-03-13 18:05:09]\tn:9"]))
    groups.append(("cache_short_line_behind", [D + "\tn:0", "[2013-03-13 18:0]", "[2013-03-13]", "[2013-03-13 18:05:09]", "[2]", D + "\tn:1"]))
    b = []
    for n in (0, 1, 9, 10, 11, 12):
        b.append(D + "".join("\t[f%d]" % i for i in range(n)) + "\tk:v")
        b.append(D + "".join("\t[%s]" % ("A" * (i + 1) if i % 3 == 0 else str(i) if i % 3 == 1 else "a/b.c:%d" % i) for i in range(n)))
    b += [D + "\t[[INFO]]\t[a[b]\tk:v", D + "\t[INFO\t[12]\tk:v", D + "\t[INFO]\n[12]\tk:v", D + "\n[INFO]\t[12]\tk:v", D + "\t[]\t[]\t[]\tk:v",
          D + "\t[INFO]\t[WARN]\t[12]\t[13]\tk:v", D + "\t[a/b]\tk:v", D + "\t[a/b:]\tk:v", D + "\t[:a.b]\tk:v", D + "\t[a.b:1:2]\t[c/d:3]\tk:v",
          D + "\t[INFO]x\t[12]\tk:v", D + "\t[INFO]]\t[12]\tk:v", D + "\t[INFO]\t", D + "\t[INFO]\t\t[12]", D + "\nabc.d:e]\tk:v",
          D + "\nABC]\t[12]\tk:v", D + "\t[In.fo]\t[1a]\t[INFO]\t[7]\t[x/y]\t[z/w:1]\tk:v", "abc]\t[INFO]\tk:v"]
    groups.append(("base_fields", b))
    p = [D + BASE4, D + BASE4 + "\t", D + BASE4 + "\t:v", D + BASE4 + "\tk:", D + BASE4 + "\t:", D + BASE4 + "\tnocolon\tk:v", D + BASE4 + "\tk:v",
         D + BASE4 + "\tk:1\tk:2\tk:3", D + BASE4 + "\t__LEVEL__:x\tmicrotime:y\tcontent:z", D + BASE4 + "\tcontent:z\tk:v",
         D + BASE4 + "\t__FILE__:x\t__THREAD__:y\t__LINE__:z", D + "k:v\tk2:v2", D + " k:v", D + "\tk:v:w\t\t\tx::y", D + BASE4 + "k:v\tk2:v2",
         D + "\t[INFO]\tk:v\t[12]\tk2:v2", D + BASE4 + "\tk:v\n\tk2:v2\r", "[1378972170]k:v", "[1378972170]\t[E]k:v\tk2:v2"]
    groups.append(("pairs", p))
    groups.append(("pairs_wide", [D + BASE4 + "".join("\tk%d:v%d" % (i, i) for i in range(40)), D + BASE4 + "\tk:v",
                                  D + BASE4 + "".join("\tk%d:v%d" % (i, i) for i in range(300))]))
    pieces = ["[INFO]", "[12]", "[a/b.c:7]", "[]", "[x", "y]", "k:v", "key:", ":val", "plain", "a:b:c", "", "[W]", "[3/4]", "\n", "content:q"]
    times = [D, "[2013-03-13 18:05:09]", "[2013-03-13 18:05:10.5]", "[1378972170425093]", "[1378972171093]", "[2013-3-13 8:5:9.25]", "[bad]",
             "[2013-03-13  18:05:09.25]", "2013"]
    for g in range(4):
        lines = []
        for _ in range(20):
            n = rng.randrange(0, 9)
            seps = [rng.choice(["\t", "\t", "\t", "", " ", "\t\t"]) for _ in range(n)]
            lines.append(rng.choice(times) + "".join(s + rng.choice(pieces) for s in seps))
        groups.append(("random_%d" % g, lines))
    return groups


POLICY_LINES = [D + BASE4 + "\tk:v", "garbage", D + BASE4 + "\tcontent:z", "[1969-01-01 00:00:00]\tk:v", ""]
INIT_CONFIGS = [
    {"SourceKey": "content"},
    {"SourceKey": "content", "Timezone": "GMT+08:00"},
    {"SourceKey": "content", "Timezone": "GMT-05:30"},
    {"SourceKey": "content", "Timezone": ""},
    {"SourceKey": "content", "Timezone": "UTC"},
    {"SourceKey": "content", "Timezone": "GMT+8:00"},
    {"SourceKey": "content", "Timezone": "GMT+0a:00"},
    {"SourceKey": "content", "Timezone": 8},
    {"SourceKey": "content", "KeepingSourceWhenParseFail": "yes", "CopingRawLog": 1, "RenamedSourceKey": 2},
    {"Timezone": "GMT+08:00"},
    {"SourceKey": ""},
    {"SourceKey": 5},
]


def run(L, P, libc, config, lines, discard, extra_event=True):
    L.ra_set_discard(int(discard))
    h = L.ra_create(json.dumps(config).encode())
    assert h, config
    P.refp_free(P.refp_take_alarms())
    events = [{"contents": [["content", ln]], "timestamp": 1, "type": 1} for ln in lines]
    if extra_event:
        events.append({"contents": [["other", "x"]], "timestamp": 1, "type": 1})
    return finish(L, P, libc, h, {"events": events})


def finish(L, P, libc, h, group):
    p = L.ra_process(h, json.dumps(group).encode("latin-1"))
    assert p
    got = json.loads(ctypes.string_at(p).decode("latin-1"), object_pairs_hook=list)
    libc.free(p)
    c = (ctypes.c_ulonglong * 5)()
    L.ra_counters(h, c)
    a = P.refp_take_alarms()
    alarms = [m for _, _, m in json.loads(ctypes.string_at(a).decode("latin-1"))]
    P.refp_free(a)
    zone = L.ra_zone_offset(h)
    L.ra_destroy(h)
    out = []
    for ev in dict(got or []).get("events", []):
        ev = dict(ev)
        out.append({"contents": [list(kv) for kv in ev.get("contents", [])], "ts": ev.get("timestamp"), "ns": ev.get("timestampNanosecond", 0)})
    return {"out": out, "counters": [int(x) for x in c], "alarms": alarms, "zone_offset": zone}


def main():
    rng = random.Random(20261018)
    now = int(time.time())
    libc0 = ctypes.CDLL(None)
    cases = []
    base = {"SourceKey": "content"}
    for name, lines in case_lines(rng):
        cases.append({"name": name, "config": dict(base, KeepingSourceWhenParseFail=True), "discard": False, "lines": lines})
    cases.append({"name": "timezone_plus8", "config": dict(base, Timezone="GMT+08:00"), "discard": False, "lines": dict(case_lines(random.Random(1)))["time_forms"]})
    cases.append({"name": "timezone_minus0530", "config": dict(base, Timezone="GMT-05:30"), "discard": False, "lines": dict(case_lines(random.Random(1)))["cache_equal_seconds"]})
    old = ["[1000000000]\tk:v", "[1990-01-01 00:00:00.5]\tk:v", "[2090-06-01 12:00:00.000001]\tk:v", "garbage", "[2090-06-01 12:00:01]\t[INFO]\tk:v",
           "[1000000000123]\tk:v", "[1990-01-01 00:00:00.5]" + "\tpad:" + "x" * 1100]
    cases.append({"name": "discard_old", "config": dict(base), "discard": True, "lines": old})
    cases.append({"name": "discard_off_same_lines", "config": dict(base), "discard": False, "lines": old})
    cases.append({"name": "long_failure_alarm", "config": dict(base), "discard": False, "lines": ["bad" + "y" * 1100, "[2013-03-13 18:05:09" + "z" * 1100]})
    n = 0
    for kf in (False, True):
        for ks in (False, True):
            for renamed in (None, "rawLog", "content"):
                for coping in (False, True):
                    config = dict(base, KeepingSourceWhenParseFail=kf, KeepingSourceWhenParseSucceed=ks, CopingRawLog=coping)
                    if renamed:
                        config["RenamedSourceKey"] = renamed
                    cases.append({"name": "policy_%d" % n, "config": config, "discard": False, "lines": POLICY_LINES})
                    n += 1
    with tempfile.TemporaryDirectory() as tmp:
        L, P, libc = build(tmp)
        for case in cases:
            per_zone = {}
            # (the source-key policy and the pair count do not meet the zone: one zone is recorded for them)
            zones = ZONES[:1] if case["name"].startswith(("policy_", "pairs_wide", "long_")) else ZONES
            for tz in zones:
                os.environ["TZ"] = tz
                libc0.tzset()
                per_zone[tz] = run(L, P, libc, case["config"], case["lines"], case["discard"])
            first = per_zone[zones[0]]
            case["ref"] = {"*": first} if len(zones) > 1 and all(per_zone[z] == first for z in zones) else per_zone
        init = []
        os.environ["TZ"] = "UTC"
        libc0.tzset()
        for config in INIT_CONFIGS:
            P.refp_free(P.refp_take_alarms())
            h = L.ra_create(json.dumps(config).encode())
            a = P.refp_take_alarms()
            alarms = [m for _, _, m in json.loads(ctypes.string_at(a).decode("utf-8"))]
            P.refp_free(a)
            init.append({"config": config, "ok": bool(h), "alarms": alarms, "zone_offset": L.ra_zone_offset(h) if h else None})
            if h:
                L.ra_destroy(h)
        unit = []
        for case in unittest_cases():
            group = json.loads(case["in"], strict=False)
            for ev in group.get("events", []):
                c = ev.get("contents", {})
                ev["contents"] = [list(kv) for kv in (sorted(c.items()) if isinstance(c, dict) else c)]
            expect = json.loads(case["expect"], strict=False)
            per_zone = {}
            for tz in ZONES:
                os.environ["TZ"] = tz
                libc0.tzset()
                L.ra_set_discard(0)
                h = L.ra_create(json.dumps(case["config"]).encode())
                assert h, case["name"]
                P.refp_free(P.refp_take_alarms())
                per_zone[tz] = finish(L, P, libc, h, group)
            # the cross-check: under the zone the unit test's numbers were written for, the compiled reference gives its expectation
            want = [(sorted(ev.get("contents", {}).items()), ev.get("timestamp"), ev.get("timestampNanosecond", 0)) for ev in expect.get("events", [])]
            agrees = [z for z in ZONES if [(sorted(map(tuple, e["contents"])), e["ts"], e["ns"]) for e in per_zone[z]["out"]] == want]
            if not agrees:
                print("FINDING: %s: the reference's own output differs from the unit test's expectation under every zone" % case["name"], file=sys.stderr)
            first = per_zone[ZONES[0]]
            unit.append({"name": case["name"], "config": case["config"], "in": group, "expect": expect, "reference_agrees_under": agrees,
                         "ref": {"*": first} if all(per_zone[z] == first for z in ZONES) else per_zone})
    doc = {"_about": "output of the reference's own processor_parse_apsara_native (tests/golden/gen_apsara_vectors.py); every group is its "
                     "lines as {content: line} events plus one event {other: x}; ref[zone] (or ref['*'] when the zones agree): out = the "
                     "events left, in order (contents as ordered pairs, ts, ns); counters = discarded, out_failed, out_key_not_found, "
                     "out_successful, history_failure; alarms = the alarm texts; zone_offset = mLogTimeZoneOffsetSecond.  now = the wall "
                     "clock of the run (Timezone is resolved against it)",
           "now": now, "zones": ZONES, "cases": cases}
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(doc, f, ensure_ascii=True, separators=(",", ":"))
        f.write("\n")
    unit_doc = {"_about": "the inJson / expectJson cases of core/unittest/processor/ProcessorParseApsaraNativeUnittest.cpp as data "
                          "(tests/golden/gen_apsara_vectors.py): config, the group (contents as ordered pairs), the expected group, the zones "
                          "under which the compiled reference gave exactly that expectation, and ref = the compiled reference's own output "
                          "per zone; init = configs with what the reference's Init answers (accepted or not, alarm texts, zone offset "
                          "under TZ=UTC)",
                "now": now, "zones": ZONES, "cases": unit, "init": init}
    with open(OUT_UNIT, "w", encoding="utf-8") as f:
        json.dump(unit_doc, f, ensure_ascii=True, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d bytes -> %s; %d unit cases, %d bytes -> %s" % (len(cases), os.path.getsize(OUT), os.path.relpath(OUT, ROOT), len(unit),
                                                                      os.path.getsize(OUT_UNIT), os.path.relpath(OUT_UNIT, ROOT)), file=sys.stderr)


if __name__ == "__main__":
    main()
