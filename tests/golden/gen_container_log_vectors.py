"""Writes tests/golden/container_log_reference_outputs.json and container_log_unittest_vectors.json: the output of the REFERENCE's OWN
processor_parse_container_log_native.

    python tests/golden/gen_container_log_vectors.py          (needs the reference tree and a built oracle/_ref; CPU only)

ProcessorParseContainerLogNative.cpp is compiled, where it lies in the reference tree, into a TEMPORARY directory against
oracle/_ref/libref_processor.so / libref_models.so, with a small driver.  (oracle/ref_models stubs that class's header and defines its
two key constants for the event model's sake; here the reference's real header comes first on the include path and the library is
linked -Bsymbolic, so the processor uses its own.)  The driver sets the group's LOG_FORMAT itself -- FromJsonString cannot -- and, for
the chain cases, runs the reference's line splitter in front and its flag-mode merge behind.  AlarmManager::IsLowLevelAlarmValid, a
rate limiter that oracle/ref_processor answers with false, is answered with true, so that the alarm texts are recorded.
Per case: the config, the format, the input group, the events left (contents in order), the group's metadata, the three counters
(out_failed, parse_stdout_total, parse_stderr_total) and the alarm texts.
The same run writes container_log_unittest_vectors.json: every inJson / expectJson pair of
core/unittest/processor/ProcessorParseContainerLogNativeUnittest.cpp read as DATA, each run through the compiled reference while the file is
written (the two with-split tests as chains: split, this processor, flag-mode merge), and `init`: configs with the warnings the
reference's Init raises.
The inputs on which the reference THROWS (a "\\u" that std::stoul or to_bytes refuses) are never handed to it: they form the separate
list `defined_only`, checked against include/lc_container_log.h's definition alone.
Only JSON is written; nothing compiled from the reference and none of its text is kept.  No test, build() or smoke() runs this file.
Seeded: the same cases come out every time."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("LC_REFERENCE_CORE", "/root/reference/core")
OUT = os.path.join(ROOT, "tests", "golden", "container_log_reference_outputs.json")
OUT_UNIT = os.path.join(ROOT, "tests", "golden", "container_log_unittest_vectors.json")
UNITTEST = os.path.join(REF, "unittest", "processor", "ProcessorParseContainerLogNativeUnittest.cpp")

GLUE = r"""
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "collection_pipeline/plugin/interface/Processor.h"
#include "models/LogEvent.h"
#include "monitor/AlarmManager.h"
#define private public
#define protected public
#include "plugin/processor/inner/ProcessorParseContainerLogNative.h"
#undef private
#undef protected
#include "plugin/processor/inner/ProcessorMergeMultilineLogNative.h"
#include "plugin/processor/inner/ProcessorSplitLogStringNative.h"
bool hdGroupFromJson(logtail::PipelineEventGroup& group, const std::string& json, std::string* error);
std::string hdGroupToJson(const logtail::PipelineEventGroup& group);
namespace logtail {
bool AlarmManager::IsLowLevelAlarmValid() { return true; }
}
namespace {
struct Handle {
    logtail::CollectionPipelineContext ctx;
    logtail::ProcessorParseContainerLogNative proc;
    logtail::ProcessorSplitLogStringNative split;
    logtail::ProcessorMergeMultilineLogNative merge;
};
}
extern "C" {
void* rc_create(const char* config_json) {
    Handle* h = new Handle;
    h->ctx.SetConfigName("test_config");
    h->proc.SetContext(h->ctx);
    h->split.SetContext(h->ctx);
    h->merge.SetContext(h->ctx);
    if (!h->proc.Init(Json::Value::fromText(config_json)) || !h->split.Init(Json::Value::fromText("{}")) ||
        !h->merge.Init(Json::Value::fromText("{\"MergeType\":\"flag\",\"UnmatchedContentTreatment\":\"single_line\"}"))) {
        delete h;
        return nullptr;
    }
    return h;
}
void rc_destroy(void* h) { delete static_cast<Handle*>(h); }
// format: the LOG_FORMAT metadata (NULL: none).  chain: the line splitter in front, the flag-mode merge behind
char* rc_process(void* hv, const char* format, const char* group_json, int chain) {
    Handle* h = static_cast<Handle*>(hv);
    std::vector<logtail::PipelineEventGroup> groups;
    groups.emplace_back(std::make_shared<logtail::SourceBuffer>());
    std::string error;
    if (!hdGroupFromJson(groups[0], group_json, &error)) return nullptr;
    if (format) groups[0].SetMetadata(logtail::EventGroupMetaKey::LOG_FORMAT, std::string(format));
    if (chain) static_cast<logtail::Processor&>(h->split).Process(groups);
    static_cast<logtail::Processor&>(h->proc).Process(groups);
    if (chain) static_cast<logtail::Processor&>(h->merge).Process(groups);
    return strdup(hdGroupToJson(groups[0]).c_str());
}
void rc_counters(void* hv, unsigned long long out[3]) {
    auto& p = static_cast<Handle*>(hv)->proc;
    out[0] = p.mOutFailedEventsTotal->GetValue();
    out[1] = p.mParseStdoutTotal->GetValue();
    out[2] = p.mParseStderrTotal->GetValue();
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
    pre = os.path.join(tmp, "pre.h")
    with open(pre, "w") as f:
        f.write('#pragma once\n#include <sys/stat.h>\n#include <cstdint>\n#include <sstream>\n#include "logger/Logger.h"\n')
    so = os.path.join(tmp, "libref_container_log.so")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-w", "-include", "set", "-include", "memory", "-include", pre,
         "-I", os.path.join(ROOT, "oracle", "ref_processor", "stubs"), "-I", os.path.join(ROOT, "oracle"),
         "-I", os.path.join(ROOT, "tests", "refhdr"), "-I", REF, "-I", os.path.join(REF, "config"),
         "-idirafter", os.path.join(ROOT, "oracle", "ref_models", "stubs"),  # (behind the real headers: the real class's header wins)
         "-o", so, glue, os.path.join(REF, "plugin", "processor", "inner", "ProcessorParseContainerLogNative.cpp"),
         "-Wl,-z,defs", "-Wl,-Bsymbolic", "-L" + ref_dir, "-lref_processor", "-lref_models", "-Wl,-rpath," + ref_dir,
         "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    L = ctypes.CDLL(so)
    L.rc_create.restype = ctypes.c_void_p
    L.rc_create.argtypes = [ctypes.c_char_p]
    L.rc_destroy.argtypes = [ctypes.c_void_p]
    L.rc_process.restype = ctypes.c_void_p
    L.rc_process.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    L.rc_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
    P = ctypes.CDLL(os.path.join(ref_dir, "libref_processor.so"))
    P.refp_take_alarms.restype = ctypes.c_void_p
    P.refp_free.argtypes = [ctypes.c_void_p]
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    return L, P, libc


def run(L, P, libc, config, fmt, group, chain=False):
    """-> {out: events left (contents as ordered pairs), metadata, counters, alarms}"""
    P.refp_free(P.refp_take_alarms())
    h = L.rc_create(json.dumps(config).encode())
    assert h, config
    init_alarms = take_alarms(P)
    p = L.rc_process(h, fmt.encode() if fmt is not None else None, json.dumps(expand(group), ensure_ascii=False).encode("latin-1"), int(chain))
    assert p, group
    got = dict(json.loads(ctypes.string_at(p).decode("latin-1"), object_pairs_hook=list) or [])
    libc.free(p)
    c = (ctypes.c_ulonglong * 3)()
    L.rc_counters(h, c)
    alarms = take_alarms(P)
    L.rc_destroy(h)
    out = []
    for ev in got.get("events", []):
        ev = dict(ev)
        out.append([list(kv) for kv in ev.get("contents", [])] if ev.get("type") == 1 else {"content": ev.get("content"), "type": ev.get("type")})
    return {"out": out, "metadata": dict(got.get("metadata", [])), "counters": [int(x) for x in c], "alarms": alarms, "init_alarms": init_alarms}


def take_alarms(P):
    a = P.refp_take_alarms()
    alarms = [m for _, _, m in json.loads(ctypes.string_at(a).decode("latin-1"))]
    P.refp_free(a)
    return alarms


T = "2024-01-05T23:28:06.818486411+08:00"
DT = "2024-02-19T03:49:37.79Z"


def docker(log, stream="stdout", time=DT):
    return '{"log":"%s","stream":"%s","time":"%s"}' % (log, stream, time)


def log_last(log):
    return '{"stream":"stdout","time":"t","log":"%s"}' % log


CONTAINERD_LINES = [
    T + " stdout F hello", " stdout F x", "nospace", T + " stdout", T + " stdout ", T + " stdout P part", T + " stdout F full",
    T + " stdout PP 1", T + " stdout P", T + " stdout F ", T + " stdout F", T + " stderr F e", T + " stderr P p", T + " stdou F x",
    T + " stdoutx F x", T + " stdoux F x", T + " STDOUT F x", T + "  stdout F x", T + " stdout  F x", T + " stdout F  x", T + " stdout P  x",
    T + " stdout Px y", T + " stdout X y", T + " stdout\tF x", T + " stdout plain content with blanks", "", " ", "  ", "   ", "a b", "a b c",
    "a stdout", "a stdout b", "a stderr P", "a stderr P ", "a stderr P  ", "x" * 1030, T + " bad " + "y" * 1000, T + " stdout F " + "z" * 1000,
]
ESCAPES = ['\\"', "\\\\", "\\/", "\\b", "\\f", "\\n", "\\r", "\\t", "\\q", "\\u00e9", "\\ud83d", "\\ud83d\\ude00", "\\u0000", "\\u12G4",
           "\\u +1f", "\\u0x1f", "\\u0X1F", "\\uffff", "\\u-000", "\\u0xZZ", "\\u\t12", "\\u007f", "\\u0080", "\\u07ff", "\\u0800"]
DOCKER_LINES = (
    [docker("plain"), docker("plain\\n"), docker("a\\n\\n"), docker(""), docker("x", "stderr"), docker("x", "stdou"), docker("x", "stdoutx"),
     docker("x", ""), docker("x", "STDOUT")]
    + [docker("a" + e + "b") for e in ESCAPES] + [docker(e) for e in ESCAPES] + [docker("".join(ESCAPES[:9]) + "\\n")]
    + [log_last("a\\u1"), log_last("a\\u12"), log_last("a\\u123"), log_last("a\\u1234"), log_last("a\\u"), log_last("a\\"), log_last("a\\\\"),
       '{"stream":"stdout","time":"t","log":"a\\}', '{"stream":"stdout","time":"t","log":"a\\u00e9}', '{"stream":"stdout","time":"t","log":"a}']
    + ['{"lo":"x","stream":"stdout","time":"t"}', '{"logx":"x","stream":"stdout","time":"t"}', '{"log1":"x","stream":"stdout","time":"t"}',
       '{"log}', '{"lo}', '{"log"}', '{"stream}', '{"strea}', '{"time}', '{"tim}', '{"xyz":"x"}', '{"":"x"}',
       '{"log":"a","log":"b","stream":"stdout","time":"t"}', '{"log":"a","log":"b","stream":"stdout""time":"t"}',
       '{"log":"a\\nx","log":"b\\ty","stream":"stdout""time":"t"}', '{"log":"a\\nx","log":"plain","stream":"stdout""time":"t"}',
       '{"log":"plain","log":"b\\ty","stream":"stdout""time":"t"}', '{"stream":"stderr","stream":"stdout","log":"x""time":"t1""time":"t2"}',
       '{"log":"x","stream":"stdout","time":"t""log":"y\\n"}', '{"log":"x","stream":"stdout","time":"t","log":"y"}', "{}", "{ }", "{", "}", "",
       "x", "{}x}", "{}}", '{"log":"x"}', '{"log":"x","stream":"stdout"}', '{"log":"x","stream":"stdout",}', '{"log":"x",}',
       '{"stream":"stdout","time":"t",}', '{"log":"x","stream":"stdout","time":"t"} ', ' {"log":"x","stream":"stdout","time":"t"}',
       '{ "log" : "x" , "stream" : "stdout" , "time" : "t" }', '{  "log"  :  "x\\n"  ,  "stream"  :  "stderr"  ,  "time"  :  "t"  }',
       '{" log":"x","stream":"stdout","time":"t"}', '{"log" "x","stream":"stdout","time":"t"}', '{"log":x,"stream":"stdout","time":"t"}',
       '{\t"log":"x","stream":"stdout","time":"t"}', '{"log"\t:"x","stream":"stdout","time":"t"}', '{"log":\t"x","stream":"stdout","time":"t"}',
       '{"log":"x"\t,"stream":"stdout","time":"t"}', '{"log":"x",\t"stream":"stdout","time":"t"}', '{"log":"x","stream":"stdout","time":"t"\t}',
       '{"log":"x","stream":"std\\nout","time":"t"}', '{"log":"x","stream":"stdout","time":"t\\n"}', '{"log":"x","stream":"stdout\\\\","time":"t"}',
       '{"log":"a\\nb\\tc","stream":"std\\\\out","time":"t"}', '{"log":"a\\nb","stream":"stdxxx","time":"t"}', '{"log":"a\\nb","stream":"stdout","time":"t"',
       '{"log":"a\\nb","stream":"stdout","time":"t"}x', '{"log":"a\\nb","stream":"stdout" "time":"t"}', '{"log":"x" "stream":"stdout","time":"t"}',
       docker("q" * 1030, "bad"), '{"log":"' + "w\\n" * 350 + '","stream":"stdout","time":"t"', docker("v\\t" * 350)])
# the reference throws on these: never handed to it
DEFINED_ONLY = [
    {"name": "u_no_digit_G123", "line": docker("a\\uG123b")},
    {"name": "u_four_blanks", "line": docker("a\\u    b")},
    {"name": "u_sign_only", "line": docker("a\\u+xyzb")},
    {"name": "u_minus_001", "line": docker("a\\u-001b")},
    {"name": "u_minus_ffff", "line": docker("a\\u-fffb")},
    {"name": "u_quote_first", "line": docker('a\\u"123')},
    {"name": "u_throw_behind_a_rewrite", "line": docker("a\\nb\\uZZZZc")},
]
POLICY_CONTAINERD = ["t1 stdout F out", "t2 stderr F err", "garbage", "t3 stdout P part", "t4 bad F x"]
POLICY_DOCKER = [docker("out\\n", time="t1"), docker("err\\n", "stderr", "t2"), "garbage", docker("x", "bad", "t3"), '{"log":"a\\nb","stream":"std\\\\out","time":"t"}']


def group_of(lines, key="content", extra=True):
    """the compact form a case is stored in; expand() makes the group of it"""
    return {"key": key, "lines": lines, "extra": extra}


def expand(group):
    """{key, lines, extra} -> one log event {key: line} per line, and with extra one event {other: x} behind them"""
    if "lines" not in group:
        return group
    events = [{"contents": [[group["key"], ln]], "timestamp": 1, "type": 1} for ln in group["lines"]]
    if group["extra"]:
        events.append({"contents": [["other", "x"]], "timestamp": 1, "type": 1})
    return {"events": events}


def random_lines(rng, fmt, n):
    lines = []
    if fmt == "1":
        times = [T, "", "t", "2024", "x" * 40]
        sources = ["stdout", "stderr", "stdout", "stderr", "stdou", "stdoutx", "", "std out"]
        tags = ["P ", "F ", "P", "F", "PP ", "", " ", "P  ", "X ", "F\t"]
        for _ in range(n):
            parts = [rng.choice(times), rng.choice(sources), rng.choice(tags) + rng.choice(["", "c", "some content", " lead", "y" * rng.randrange(60)])]
            lines.append(rng.choice([" ", " ", " ", "  ", ""]).join(parts) if rng.random() < 0.3 else " ".join(parts))
    else:
        pieces = ["a", "bc", " ", "x" * 30, "\\n", "\\t", '\\"', "\\\\", "\\/", "\\b", "\\f", "\\r", "\\q", "\\u00e9", "\\ud83d", "\\u0041", "\\u 7f",
                  "\\u0x9", "\\u12G4", "\\uffff", "\\u0000", "{", "}", ",", ":"]
        for _ in range(n):
            log = "".join(rng.choice(pieces) for _ in range(rng.randrange(0, 12)))
            keys = [("log", log), ("stream", rng.choice(["stdout", "stderr", "stdout", "stdxx", ""])), ("time", rng.choice([DT, "t", ""]))]
            rng.shuffle(keys)
            if rng.random() < 0.15:
                keys.append(rng.choice([("log", "dup" + rng.choice(pieces)), ("stream", "stderr"), ("time", "t2")]))
            sp = lambda: rng.choice(["", "", "", " ", "  "])  # noqa: E731
            text = "{" + sp()
            for k, (name, val) in enumerate(keys):
                text += '"%s"%s:%s"%s"%s' % (name, sp(), sp(), val, sp())
                text += "," + sp() if k < 2 and k + 1 < len(keys) else ("," if rng.random() < 0.05 else "")
            text += "}"
            r = rng.random()
            if r < 0.05:
                text = text[:rng.randrange(len(text))]
            elif r < 0.08:
                text = text.replace('"', "'", 1)
            elif r < 0.11:
                text = text.replace(" ", "\t", 1)
            lines.append(text)
    return lines


def cases_list(rng):
    cases = []
    base = {}
    cases.append({"name": "containerd_lines", "config": base, "format": "1", "group": group_of(CONTAINERD_LINES)})
    cases.append({"name": "docker_lines", "config": base, "format": "2", "group": group_of(DOCKER_LINES)})
    cases.append({"name": "containerd_other_source_key", "config": {"SourceKey": "raw"}, "format": "1", "group": group_of(CONTAINERD_LINES[:16], "raw")})
    # (the source value stays beside the new keys: the reference's in-place rewrite of it is on record -- every second line that
    # holds a backslash, the long ones left out)
    rewritten = [ln for ln in DOCKER_LINES if "\\" in ln and len(ln) < 300][::2]
    cases.append({"name": "docker_other_source_key", "config": {"SourceKey": "raw"}, "format": "2", "group": group_of(rewritten, "raw")})
    cases.append({"name": "docker_other_source_key_discard_failed", "config": {"SourceKey": "raw", "KeepingSourceWhenParseFail": False}, "format": "2",
                  "group": group_of(rewritten[::3], "raw")})
    n = 0
    for ign_out in (False, True):
        for ign_err in (False, True):
            for keep in (False, True):
                for quiet in (False, True):
                    config = {"IgnoringStdout": ign_out, "IgnoringStderr": ign_err, "KeepingSourceWhenParseFail": keep, "IgnoreParseWarning": quiet}
                    cases.append({"name": "policy_containerd_%d" % n, "config": config, "format": "1", "group": group_of(POLICY_CONTAINERD, extra=False)})
                    cases.append({"name": "policy_docker_%d" % n, "config": config, "format": "2", "group": group_of(POLICY_DOCKER, extra=False)})
                    n += 1
    mixed = {"events": [{"content": "a raw event", "timestamp": 1, "type": 4}, {"contents": [["content", T + " stdout F one"]], "timestamp": 1, "type": 1},
                        {"contents": [["other", "x"]], "timestamp": 1, "type": 1}, {"contents": [], "timestamp": 1, "type": 1},
                        {"contents": [["content", T + " stdout P two"], ["keep", "me"]], "timestamp": 1, "type": 1}]}
    cases.append({"name": "non_log_events_and_no_key_containerd", "config": base, "format": "1", "group": mixed})
    mixed2 = json.loads(json.dumps(mixed))
    mixed2["events"][1]["contents"][0][1] = docker("one\\n")
    mixed2["events"][4]["contents"][0][1] = docker("two", "stderr")
    cases.append({"name": "non_log_events_and_no_key_docker", "config": base, "format": "2", "group": mixed2})
    for fmt, name in (("3", "unknown"), (None, "absent"), ("", "empty"), ("11", "eleven")):
        cases.append({"name": "format_%s" % name, "config": base, "format": fmt, "group": group_of(POLICY_CONTAINERD + POLICY_DOCKER)})
    cases.append({"name": "empty_group", "config": base, "format": "1", "group": {"events": []}})
    cases.append({"name": "random_containerd", "config": {}, "format": "1", "group": group_of(random_lines(rng, "1", 40))})
    cases.append({"name": "random_docker", "config": {"SourceKey": "raw"}, "format": "2", "group": group_of(random_lines(rng, "2", 40), "raw")})
    chain1 = "\n".join([T + " stdout P Exception i", T + " stdout P n thread", T + " stdout F  'main'", T + " stderr F dropped?", T + " stdout F single",
                        "garbage line", T + " stdout P tail without full"])
    cases.append({"name": "chain_containerd", "config": base, "format": "1", "chain": True, "group": group_of([chain1], extra=False)})
    cases.append({"name": "chain_containerd_ignoring_stderr", "config": {"IgnoringStderr": True}, "format": "1", "chain": True,
                  "group": group_of([chain1], extra=False)})
    chain2 = "\n".join([docker("Exception in thread\\n"), docker("    at a.b.c\\n"), docker("err\\n", "stderr"), "garbage", docker("no newline")])
    cases.append({"name": "chain_docker", "config": base, "format": "2", "chain": True, "group": group_of([chain2], extra=False)})
    return cases


INIT_CONFIGS = [
    {},
    {"SourceKey": "raw", "IgnoringStdout": True, "IgnoringStderr": True, "IgnoreParseWarning": True, "KeepingSourceWhenParseFail": False},
    {"SourceKey": 1},
    {"IgnoringStdout": "true", "IgnoringStderr": 1},
    {"IgnoreParseWarning": "yes", "KeepingSourceWhenParseFail": 0},
    {"SourceKey": ""},
]


def unittest_cases():
    """every inJson / expectJson pair, in file order: -> [{name, config, format, chain, in, expect}]"""
    with open(UNITTEST, encoding="utf-8") as f:
        text = f.read()
    token = re.compile(r'void ProcessorParseContainerLogNativeUnittest::(\w+)\(\)|(inJson|expectJson)\s*(?:=|<<)\s*R"\((.*?)\)"|Json::Value config;|'
                       r'config\["(\w+)"\] = ([^;]+);|LOG_FORMAT,\s*ProcessorParseContainerLogNative::(\w+)\)|APSARA_TEST_STREQ\(CompactJson\(expectJson', re.S)
    cases = []
    name, configs, raw, sub, fmt = None, [{}], {}, 0, None
    for m in token.finditer(text):
        t = m.group(0)
        if m.group(1):
            name, configs, raw, sub, fmt = m.group(1), [{}], {}, 0, None
        elif m.group(2):
            raw[m.group(2)] = m.group(3)
        elif t == "Json::Value config;":
            configs.append({})
        elif m.group(4):
            v = m.group(5).strip()
            if v in ("true", "false"):
                configs[-1][m.group(4)] = v == "true"
            elif v.startswith('"'):
                configs[-1][m.group(4)] = v[1:-1]
            elif re.fullmatch(r"-?\d+", v):
                configs[-1][m.group(4)] = int(v)
        elif m.group(6):
            fmt = "1" if m.group(6) == "CONTAINERD_TEXT" else "2"
        elif t.startswith("APSARA_TEST_STREQ") and "inJson" in raw and "expectJson" in raw:
            sub += 1
            chain = name.endswith("WithSplit")
            own = [c for c in configs if "IgnoringStdout" in c or "IgnoringStderr" in c or "KeepingSourceWhenParseFail" in c or "SourceKey" in c]
            config = own[-1] if own else {}
            cases.append({"name": "%s/%d" % (name, sub), "config": dict(config), "format": fmt, "chain": chain, "in": raw["inJson"],
                          "expect": raw["expectJson"]})
            raw = {}
    return cases


def main():
    rng = random.Random(20261019)
    cases = cases_list(rng)
    with tempfile.TemporaryDirectory() as tmp:
        L, P, libc = build(tmp)
        for case in cases:
            case["ref"] = run(L, P, libc, case["config"], case["format"], case["group"], case.get("chain", False))
            del case["ref"]["init_alarms"]
        init = []
        for config in INIT_CONFIGS:
            r = run(L, P, libc, config, "1", group_of([T + " stdout F x"], config["SourceKey"] if isinstance(config.get("SourceKey"), str) else "content"))
            init.append({"config": config, "alarms": r["init_alarms"], "out": r["out"], "counters": r["counters"]})
        unit = []
        for case in unittest_cases():
            group = json.loads(case["in"], strict=False)
            for ev in group.get("events", []):
                c = ev.get("contents", {})
                ev["contents"] = [list(kv) for kv in (sorted(c.items()) if isinstance(c, dict) else c)]
            expect = json.loads(case["expect"], strict=False)
            ref = run(L, P, libc, case["config"], case["format"], group, case["chain"])
            del ref["init_alarms"]
            # the cross-check: the compiled reference gives the unit test's expectation (the with-split tests run a fourth, regex-mode merge
            # behind the three recorded stages: not compared)
            want = [sorted(ev.get("contents", {}).items()) for ev in expect.get("events", [])]
            agrees = [sorted(map(tuple, e)) for e in ref["out"]] == want
            if not agrees and not case["chain"]:
                print("FINDING: %s: the reference's own output differs from the unit test's expectation" % case["name"], file=sys.stderr)
            unit.append({"name": case["name"], "config": case["config"], "format": case["format"], "chain": case["chain"], "in": group,
                         "reference_agrees": agrees, "ref": ref})
    doc = {"_about": "output of the reference's own processor_parse_container_log_native (tests/golden/gen_container_log_vectors.py).  Per case: "
                     "config, format (the group's LOG_FORMAT metadata; null: none), group (the input: events with contents as ordered pairs, or "
                     "{key, lines, extra}: one log event {key: line} per line and with extra one event {other: x} behind them), chain (true: "
                     "the reference's line splitter in front and its flag-mode merge behind), ref: out = the events left, in order (a log event "
                     "is its contents as ordered pairs); metadata "
                     "= the group's, as the fixture writer names it; counters = out_failed, parse_stdout_total, parse_stderr_total; alarms = "
                     "the alarm texts.  defined_only: lines on which the reference throws, never handed to it; include/lc_container_log.h "
                     "defines them as LC_CLOG_FAIL_JSON",
           "cases": cases, "defined_only": DEFINED_ONLY}
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(doc, f, ensure_ascii=True, separators=(",", ":"))
        f.write("\n")
    unit_doc = {"_about": "the inJson / expectJson pairs of core/unittest/processor/ProcessorParseContainerLogNativeUnittest.cpp as data "
                          "(tests/golden/gen_container_log_vectors.py): config, format, the group, whether the compiled "
                          "reference gave that expectation (chain cases: the unit test runs a fourth stage that is not recorded), and ref = "
                          "the compiled reference's own output; init = configs with the warnings the reference's Init raises",
                "cases": unit, "init": init}
    with open(OUT_UNIT, "w", encoding="utf-8") as f:
        json.dump(unit_doc, f, ensure_ascii=True, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d bytes -> %s; %d unit cases (%d agree), %d bytes -> %s" % (
        len(cases), os.path.getsize(OUT), os.path.relpath(OUT, ROOT), len(unit), sum(u["reference_agrees"] for u in unit),
        os.path.getsize(OUT_UNIT), os.path.relpath(OUT_UNIT, ROOT)), file=sys.stderr)


if __name__ == "__main__":
    main()
