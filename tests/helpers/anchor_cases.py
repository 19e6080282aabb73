"""What the anchor tests share: the fixtures of tests/golden (anchor_unittest_vectors.json, anchor_model_vectors.json) as (label, config,
value, tail, rows) cases, seeded random values, the model's answer in the fixtures' form, and the stand-alone host program
(tests/native/anchor_host_check.cpp) as a child process.  `tail`: the bytes that follow the value in a packed buffer."""
import functools
import hashlib
import json
import os
import random
import subprocess

import numpy as np

from helpers import anchor_model

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@functools.lru_cache(maxsize=None)
def load_fixtures():
    with open(os.path.join(GOLDEN, "anchor_unittest_vectors.json"), encoding="utf-8") as f:
        unit = json.load(f)
    with open(os.path.join(GOLDEN, "anchor_model_vectors.json"), encoding="utf-8") as f:
        model = json.load(f)
    return unit, model


def config_of(pairs, **switches):
    """[(Start, Stop), ...] -> a configuration with the fields named f0, f1, ..."""
    return dict({"Anchors": [{"Start": s, "Stop": p, "FieldName": "f%d" % i} for i, (s, p) in enumerate(pairs)]}, **switches)


def rows_text(config, value):
    """the model's answer as the fixtures record it: b and e of every anchor, joined by blanks"""
    return " ".join("%d %d" % be for be in anchor_model.locate(config, value))


def rows_of(text, stride=None):
    """-> an int32 array [anchors][2]; stride: padded with (-1, -1) entries to that many"""
    out = np.array([int(x) for x in text.split()], np.int32).reshape(-1, 2)
    if stride is not None and len(out) < stride:
        out = np.concatenate([out, np.full((stride - len(out), 2), -1, np.int32)])
    return out


def random_values(symbols, seed, n, longest=24):
    """n seeded values over `symbols` (byte strings of any length), up to `longest` bytes"""
    rng, out = random.Random(seed), []
    for _ in range(n):
        target, value = rng.randint(0, longest), b""
        while True:
            s = symbols[rng.randrange(len(symbols))]
            if len(value) + len(s) > target:
                break
            value += s
        out.append(value)
    return out


def set_values(s):
    return random_values([x.encode("utf-8") for x in s["symbols"]], s["seed"], s["n"], s["longest"])


def with_tails(values):
    """every value with the bytes that follow it when the values lie back to back"""
    blob = b"".join(values)
    out, at = [], 0
    for v in values:
        at += len(v)
        out.append((v, blob[at:at + 40]))
    return out


def outcome_shares(config, values):
    """per anchor the share of the values on which it gives a field, no start, no stop"""
    shares = []
    for k in range(len(config["Anchors"])):
        got = [anchor_model.locate(config, v)[k][0] for v in values]
        n = float(len(values))
        shares.append({"field": sum(1 for b in got if b >= 0) / n, "no_start": got.count(anchor_model.NO_START) / n,
                       "no_stop": got.count(anchor_model.NO_STOP) / n})
    return shares


CODE = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"


def digest(values, rows):
    """what a random set records of its values and of the model's answers: a SHA-256 of each list (every entry behind its length), and two
    characters per value (12 bits of a SHA-256 of its rows text) that say WHICH value differs"""
    def sha(items):
        h = hashlib.sha256()
        for x in items:
            h.update(b"%d:" % len(x) + x)
        return h.hexdigest()

    def code(r):
        d = hashlib.sha256(r.encode()).digest()
        return CODE[d[0] & 63] + CODE[d[1] & 63]
    return {"values_sha256": sha(values), "rows_sha256": sha([r.encode() for r in rows]), "codes": "".join(code(r) for r in rows)}


@functools.lru_cache(maxsize=None)
def all_cases():
    """every fixture case -> [(label, config, value bytes, tail bytes, rows text: recorded for the unit and named cases, the model's for
    the random sets)]"""
    unit, model = load_fixtures()
    out = [("unit:" + e["case"], e["run_config"], e["value"].encode("utf-8"), b"", e["rows"]) for e in unit["cases"] if "rows" in e]
    out += [("named:" + e["name"], e["config"], e["value"].encode("utf-8"), e.get("tail", "").encode("utf-8"), e["rows"]) for e in model["named"]]
    for s in model["random"]:  # (values from the set's seed, rows from the model; tests/test_anchor_model.py holds both to the digests)
        out += [("random:%s:%d" % (s["name"], i), s["config"], v, t, rows_text(s["config"], v)) for i, (v, t) in enumerate(with_tails(set_values(s)))]
    return out


def cases_by_config(cases):
    """-> [(config, [case, ...])], the cases of one configuration together, in first-seen order"""
    groups = {}
    for c in cases:
        groups.setdefault(json.dumps(c[1], sort_keys=True), (c[1], []))[1].append(c)
    return list(groups.values())


def build_host_check(out_dir, sanitize=False, source=None):
    """tests/native/anchor_host_check.cpp -> an executable in out_dir; source: a mutated copy's program (in its own tree)"""
    exe = os.path.join(str(out_dir), "anchor_host_check_asan" if sanitize else "anchor_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-w"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd + ["-o", exe, source or os.path.join(ROOT, "tests", "native", "anchor_host_check.cpp")])
    return exe


def run_host_check(exe, triples):
    """triples: [(config, value, tail)] -> the program's answers in the fixtures' form (rows text)"""
    payload = []
    for config, value, tail in triples:
        c = anchor_model.init(config)
        needles = [x for a in c["Anchors"] for x in (a["Start"], a["Stop"])]
        payload.append(b"%d %d %d\n" % (len(c["Anchors"]), len(value), len(tail)) + b" ".join(b"%d" % len(x) for x in needles) + b"\n" +
                       b"".join(needles) + value + tail + b"\n")
    r = subprocess.run([exe], input=b"".join(payload), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode("utf-8", "replace")[-2000:])
    out = r.stdout.decode().split("\n")[:-1]
    assert len(out) == len(triples)
    return out
