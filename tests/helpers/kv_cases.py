"""What the key-value tests share: the fixtures of tests/golden (kv_unittest_vectors.json, kv_model_vectors.json) as (label, config,
value, rows) cases, seeded random values, the model's answer in the ABI's form, and the stand-alone host program
(tests/native/kv_host_check.cpp) as a child process."""
import functools
import hashlib
import json
import os
import random
import subprocess

import numpy as np

from helpers import kv_model

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PANIC = "P"


@functools.lru_cache(maxsize=None)
def load_fixtures():
    with open(os.path.join(GOLDEN, "kv_unittest_vectors.json"), encoding="utf-8") as f:
        unit = json.load(f)
    with open(os.path.join(GOLDEN, "kv_model_vectors.json"), encoding="utf-8") as f:
        model = json.load(f)
    return unit, model


def symbols(config):
    c = kv_model.init(config)
    return [b"a", b"b", b" ", b"\\", b"\"", b"'", c["Delimiter"], c["Separator"], c["Quote"]]


def rows_text(config, value):
    """the model's answer as the fixtures record it: "P", or the rows' integers joined by blanks"""
    status, pairs = kv_model.split(config, value)
    return PANIC if status == "panic" else " ".join(str(x) for _, _, _, spans in pairs for x in spans)


def rows_of(text):
    """-> None for a panic value, else an int32 array [npairs][4]"""
    if text == PANIC:
        return None
    return np.array([int(x) for x in text.split()], np.int32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def all_cases():
    """every fixture case -> [(label, config, value bytes, rows text: recorded for the unit and named cases, the model's for the random sets)]"""
    unit, model = load_fixtures()
    out = [("unit:" + e["case"], e["config"], e["value"].encode("utf-8"), e["rows"]) for e in unit["cases"]]
    out += [("named:" + e["name"], e["config"], e["value"].encode("utf-8"), e["rows"]) for e in model["named"]]
    for s in model["random"]:  # (values from the set's seed, rows from the model; tests/test_kv_model.py holds both to the set's digests)
        values = random_values(s["config"], s["seed"], s["n"], s["longest"])
        out += [("random:%s:%d" % (s["name"], i), s["config"], v, rows_text(s["config"], v)) for i, v in enumerate(values)]
    return out


CODE = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"


def digest(values, rows):
    """what a random set records of its values and of the model's answers: a SHA-256 of each list (every entry behind its length), and two
    characters per value (12 bits of a SHA-256 of its rows text; "!!" for a value the reference panics on) that say WHICH value differs"""
    def sha(items):
        h = hashlib.sha256()
        for x in items:
            h.update(b"%d:" % len(x) + x)
        return h.hexdigest()
    def code(r):
        if r == PANIC:
            return "!!"
        d = hashlib.sha256(r.encode()).digest()
        return CODE[d[0] & 63] + CODE[d[1] & 63]
    return {"values_sha256": sha(values), "rows_sha256": sha([r.encode() for r in rows]), "codes": "".join(code(r) for r in rows)}


def cases_by_config(cases):
    """-> [(config, [case, ...])], the cases of one configuration together, in first-seen order"""
    groups = {}
    for c in cases:
        groups.setdefault(json.dumps(c[1], sort_keys=True), (c[1], []))[1].append(c)
    return list(groups.values())


def random_values(config, seed, n, longest=24):
    """n seeded values over the nine-symbol alphabet of `config`, up to `longest` bytes"""
    rng, syms, out = random.Random(seed), symbols(config), []
    for _ in range(n):
        target, value = rng.randint(0, longest), b""
        while True:
            s = syms[rng.randrange(9)]
            if len(value) + len(s) > target:
                break
            value += s
        out.append(value)
    return out


def needles(config):
    c = kv_model.init(config)
    return c["Delimiter"], c["Separator"], c["Quote"]


def build_host_check(out_dir, sanitize=False, source=None, include_first=None):
    """tests/native/kv_host_check.cpp -> an executable in out_dir; source / include_first: a mutated copy's program and tree"""
    exe = os.path.join(str(out_dir), "kv_host_check_asan" if sanitize else "kv_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-w"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd + ["-I", os.path.join(ROOT, "include"), "-o", exe, source or os.path.join(ROOT, "tests", "native", "kv_host_check.cpp")])
    return exe


def run_host_check(exe, pairs):
    """pairs: [(config, value)] -> the program's answers in the fixtures' form (rows text)"""
    payload = []
    for config, value in pairs:
        d, s, q = needles(config)
        payload.append(b"%d %d %d %d\n" % (len(d), len(s), len(q), len(value)) + d + s + q + value + b"\n")
    r = subprocess.run([exe], input=b"".join(payload), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode("utf-8", "replace")[-2000:])
    out = []
    for line in r.stdout.decode().split("\n")[:-1]:
        f = line.split()
        out.append(PANIC if f[0] == "1" else " ".join(f[2:]))
        assert f[0] == "1" or int(f[1]) * 4 == len(f) - 2, line
    assert len(out) == len(pairs)
    return out
