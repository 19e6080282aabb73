"""Writes tests/golden/desensitize_unittest_vectors.json.  Run by hand, from the repository root, where the reference tree is at hand:

    python tests/golden/gen_desensitize_vectors.py /path/to/reference

It reads core/unittest/processor/ProcessorDesensitizeNativeUnittest.cpp AS DATA: every config (the GetCastSensWordConfig call and the
config[...] assignments behind it), every inJson and the stages run between them and the comparison -- the line splitter, the multiline
splitter and the regex-mode merge of the two chain tests are recorded as stages, and so are the three desensitize configs the Loggroup
test runs over one group.  What is stored per case: the configs, the input, the group as it reaches the first desensitize stage, and
the MODEL's output (tests/helpers/desensitize_model.py).  The unit test's expectation text is not kept; `unittest_agrees` says whether
the model's output equalled it, event for event, when this file was written.  Nothing under tests/ reads the reference tree.
How the stages in front are modelled: tests/golden/README_desensitize.md."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import desensitize_model as model  # noqa: E402
from oracle.multiline_oracle import MultilineOracle  # noqa: E402
from oracle.split_oracle import split_lines  # noqa: E402

DEFAULTS = ["cast1", "const", "********", "pwd=", "[^,]+", False]
CONFIG_KEYS = ["SourceKey", "Method", "ReplacingString", "ContentPatternBeforeReplacedString", "ReplacedContentPattern", "ReplacingAll"]
STAGE_KEYS = {"split": ["SplitChar"], "split_multiline": ["StartPattern", "UnmatchedContentTreatment"],
              "merge": ["StartPattern", "UnmatchedContentTreatment", "MergeType"]}

TOKEN = re.compile(
    r'void ProcessorDesensitizeNativeUnittest::(?P<test>\w+)\(\)'
    r'|Json::Value config = GetCastSensWordConfig\((?P<args>[^;]*)\);'
    r'|config\["(?P<key>\w+)"\] = (?P<value>[^;]*);'
    r'|inJson = R"\((?P<inj>.*?)\)";'
    r'|expectJson = R"\((?P<exp>.*?)\)";'
    r'|(?P<split>processorSplitLogStringNative\.Process\()'
    r'|(?P<msplit>processorSplitMultilineLogStringNative\.Process\()'
    r'|(?P<merge>processorMergeMultilineLogNative\.Process\()'
    r'|(?P<desens>processor(?:Instance)?\.Process\()'
    r'|(?P<judge>APSARA_TEST_STREQ_FATAL\(CompactJson\(expectJson\))', re.S)


def cxx_value(text):
    """a C++ argument: "string literal", std::string("..."), true / false"""
    text = text.strip()
    m = re.fullmatch(r'(?:std::string\()?"((?:[^"\\]|\\.)*)"\)?', text)
    if m:
        return re.sub(r"\\(.)", lambda q: {"n": "\n", "t": "\t", "r": "\r"}.get(q.group(1), q.group(1)), m.group(1))
    assert text in ("true", "false"), text
    return text == "true"


def split_args(text):
    out, depth, cur, quoted, i = [], 0, "", False, 0
    while i < len(text):
        c = text[i]
        if quoted:
            cur += c
            if c == "\\":
                cur += text[i + 1]
                i += 1
            elif c == '"':
                quoted = False
        elif c == '"':
            quoted = True
            cur += c
        elif c == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            depth += c == "("
            depth -= c == ")"
            cur += c
        i += 1
    if cur.strip():
        out.append(cur)
    return out


def make_config(args):
    values = list(DEFAULTS)
    for i, a in enumerate(split_args(args)):
        values[i] = cxx_value(a)
    config = dict(zip(CONFIG_KEYS, values))
    if config["ReplacingString"] == "":
        del config["ReplacingString"]
    return config


def events_of(group):
    """-> per event: type and the ordered contents"""
    return [{"type": ev.get("type"), "contents": sorted(ev.get("contents", {}).items())} for ev in group["events"]]


def cut_events(group, key, records_of):
    """a splitter / the merge: every log event's `key` value is cut into records (begin, length); each record is an event of its own
    that keeps the other contents"""
    out = []
    for ev in group["events"]:
        if ev.get("type") != 1 or key not in ev.get("contents", {}):
            out.append(ev)
            continue
        value = ev["contents"][key].encode("utf-8")
        for b, n in records_of(value):
            piece = dict(ev)
            piece["contents"] = dict(ev["contents"], **{key: value[b:b + n].decode("utf-8")})
            out.append(piece)
    return dict(group, events=out)


def run_stage(kind, config, group):
    key = config["SourceKey"]
    if kind == "split":
        return cut_events(group, key, lambda v: split_lines(v, ord(config.get("SplitChar", "\n"))))  # ("\n": the splitter's default)
    if kind == "split_multiline":
        ml = MultilineOracle(StartPattern=config["StartPattern"], UnmatchedContentTreatment=config["UnmatchedContentTreatment"])
        return cut_events(group, key, lambda v: [(b, n) for b, n, _ in ml.split(v)[0]])
    if kind == "merge":
        # the regex-mode merge over the events the line splitter left: the records the multiline rule cuts out of their lines joined
        # again, one event per record
        ml = MultilineOracle(StartPattern=config["StartPattern"], UnmatchedContentTreatment=config["UnmatchedContentTreatment"])
        logs = [ev for ev in group["events"] if ev.get("type") == 1 and key in ev.get("contents", {})]
        joined = "\n".join(ev["contents"][key] for ev in logs).encode("utf-8")
        merged = [dict(logs[0], contents=dict(logs[0]["contents"], **{key: joined[b:b + n].decode("utf-8")})) for b, n, _ in ml.split(joined)[0]]
        return dict(group, events=merged)
    raise AssertionError(kind)


def main(reference):
    path = os.path.join(reference, "core", "unittest", "processor", "ProcessorDesensitizeNativeUnittest.cpp")
    with open(path, encoding="utf-8") as f:
        text = f.read()
    text = text[text.index("void ProcessorDesensitizeNativeUnittest::TestMultipleLines()"):]
    cases, test, count = [], None, 0
    configs, stages, in_json, expect = [], [], None, None
    for m in TOKEN.finditer(text):
        if m.group("test"):
            test, count = m.group("test"), 0
            configs, stages = [], []
        elif m.group("args") is not None:
            configs.append(make_config(m.group("args")))
        elif m.group("key"):
            configs[-1][m.group("key")] = cxx_value(m.group("value"))
        elif m.group("inj") is not None:
            in_json = json.loads(m.group("inj"), strict=False)
        elif m.group("exp") is not None:
            expect = json.loads(m.group("exp"), strict=False)
        elif m.group("split"):
            stages.append(("split", len(configs) - 1))
        elif m.group("msplit"):
            stages.append(("split_multiline", len(configs) - 1))
        elif m.group("merge"):
            stages.append(("merge", len(configs) - 1))
        elif m.group("desens"):
            stages.append(("desensitize", len(configs) - 1))
        elif m.group("judge"):
            count += 1
            group, at_desensitize, recorded = in_json, None, []
            for kind, ci in stages:
                config = configs[ci]
                if kind == "desensitize":
                    if at_desensitize is None:
                        at_desensitize = group
                    own = {k: config[k] for k in CONFIG_KEYS if k in config}
                    group, counters = model.process_group(own, group, encoding="utf-8")
                    recorded.append({"kind": kind, "config": own, "counters": counters})
                else:
                    group = run_stage(kind, config, group)
                    recorded.append({"kind": kind, "config": {k: config[k] for k in ["SourceKey"] + STAGE_KEYS[kind] if k in config}})
            cases.append({"name": "%s#%d" % (test, count), "stages": recorded, "in": in_json, "at_desensitize": at_desensitize,
                          "out": events_of(group), "unittest_agrees": events_of(group) == events_of(expect)})
            configs, stages = [], []
    assert len(cases) >= 28, len(cases)  # every comparison of the unit test
    doc = {
        "source": "core/unittest/processor/ProcessorDesensitizeNativeUnittest.cpp read as data; outputs are the model's",
        "cases": cases,
        # handles whose behaviour is DEFINED here because the reference's is an error path of RE2 (include/lc_desensitize.h)
        "defined_only": [{"name": "rewrite_bad_escape",
                          "config": {"SourceKey": "cast1", "Method": "const", "ReplacingString": "\\x", "ContentPatternBeforeReplacedString": "pwd=",
                                     "ReplacedContentPattern": "[^,]+", "ReplacingAll": True},
                          "in": {"events": [{"type": 1, "timestamp": 1, "contents": {"cast1": "a pwd=secret, b"}}]},
                          "defined": "pass-through with an Init warning: values unchanged, counters as usual"}],
    }
    out = os.path.join(ROOT, "tests", "golden", "desensitize_unittest_vectors.json")
    with open(out, "w", encoding="utf-8") as f:
        json.dump(doc, f, ensure_ascii=True, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d cases, %d agree with the unit test" % (len(cases), sum(c["unittest_agrees"] for c in cases)))


if __name__ == "__main__":
    main(sys.argv[1])
