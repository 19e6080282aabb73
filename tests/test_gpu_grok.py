"""Grok on the device, through the C ABI of include/lc_grok.h: the reference's own parse vectors
(processor_grok_test.go:119-373), the regex-module golden vectors, random values against the Grok oracle, many matches per
value (FindNextMatch), the extra-row overflow protocol and the device-resident entry point."""
import json
import os
import random

import numpy as np
import pytest

from loongcollector_amd import binding as B
from loongcollector_amd.grok import Grok, GrokInitError
from oracle.grok_oracle import GrokOracle
from tests.helpers.grok_device_rows import device_rows as _device_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert B.device_count() >= 1
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "grok_golden.json"), encoding="utf-8") as f:
        return json.load(f)


def test_reference_parse_vectors_through_process_logs(torch_dev, golden):
    ran = 0
    for r in golden["reference"]:
        try:
            g = Grok(**r["config"])
        except GrokInitError:
            continue   # a Match entry no device engine can run yet (reported in DESIGN.md); Init fails loudly
        ran += 1
        got = g.process_logs([[tuple(kv) for kv in log] for log in r["in"]])
        assert [[list(kv) for kv in log] for log in got] == r["out"], r["cite"]
    assert ran == len(golden["reference"])


def test_regex_module_golden_vectors(torch_dev, golden):
    checked = skipped = 0
    for c in golden["regex"]:
        try:
            g = Grok(**c["config"])
        except GrokInitError:
            skipped += 1
            continue
        values = [v.encode("latin-1") for v, _ in c["subs"]]
        pattern, fields = g.match_host(values)
        for (val, want), p, f in zip(c["subs"], pattern, fields):
            checked += 1
            assert [[k, v.decode("latin-1")] for k, v in f] == want, (c["config"]["Match"], val)
            assert (p >= 0) == bool(want)
    assert checked >= 300 and skipped == 0


def _random_values(rng, n):
    words = [b"GET", b"10.0.0.1", b"192.168.001.77", b"-3.5", b"err", b"2024-01-04T14:36:10Z", b"x=1", b"k=", b"[a]", b"\"q s\"",
             b"abc_9", b"::1", b"7", b"ERROR", b"info:", b"/p/a?x=1", b"\xe4\xbd\xa0\xe5\xa5\xbd", b""]
    out = []
    for _ in range(n):
        k = rng.randint(0, 9)
        out.append(rng.choice([b" ", b"  ", b"\t", b","]).join(rng.choice(words) for _ in range(k)))
    return out


@pytest.mark.parametrize("match", [
    ["%{IPV4:ip}"],
    ["%{LOGLEVEL:level}:? %{GREEDYDATA:msg}", "(?P<k>\\w+)=(?P<v>\\S*)", "%{INT:n}"],
    ["%{TIMESTAMP_ISO8601:ts}", "%{WORD:a} %{WORD:b}", "%{NOTSPACE:first}"],
    ["(?P<x>\\d+)|(?P<x>[a-z]+)_(?P<y>\\d)"],
])
def test_random_values_against_the_oracle(torch_dev, match):
    rng = random.Random(99)
    values = _random_values(rng, 3000)
    g = Grok(Match=match)
    o = GrokOracle(match)
    pattern, fields = g.match_host(values)
    nmulti = 0
    for v, p, f in zip(values, pattern, fields):
        res, want = o.process_value(v)
        assert f == want, (match, v)
        assert (p >= 0) == (res == 0)
        nmulti += len(want) > len(g.columns(int(p))) if p >= 0 else 0
    if match == ["%{IPV4:ip}"]:
        assert nmulti > 50   # several matches per value really happen (FindNextMatch path)


MONGO_PATTERNS = {  # example_config/processor_grok_patterns/mongodb:2-4, verbatim
    "MONGO_QUERY": r"\{ (?<={ ).*(?= } ntoreturn:) \}",
    "MONGO_SLOWQUERY": r"%{WORD} %{MONGO_WORDDASH:database}\.%{MONGO_WORDDASH:collection} %{WORD}: %{MONGO_QUERY:query} %{WORD}:%{NONNEGINT:ntoreturn} "
                       r"%{WORD}:%{NONNEGINT:ntoskip} %{WORD}:%{NONNEGINT:nscanned}.*nreturned:%{NONNEGINT:nreturned}..+ (?<duration>[0-9]+)ms",
    "MONGO_WORDDASH": r"\b[\w-]+\b",
}


def test_the_library_patterns_with_multi_byte_lookarounds(torch_dev):
    """MONGO_SLOWQUERY / MONGO_QUERY (mongodb:2-3) failed Init through round 4: "(?<={ )" is decided by the literal in front of it,
    "(?= } ntoreturn:)" is a window the rest of the entry does not decide (the word behind the query is any %{WORD}) -- a product of
    the automaton with the window's chain.  Slow-query lines, near misses and nested braces, on the device against the Grok oracle."""
    rng = random.Random(7)
    match = ["%{MONGO_SLOWQUERY}", "%{MONGO_QUERY:q}"]
    g = Grok(Match=match, CustomPatterns=MONGO_PATTERNS)
    o = GrokOracle(match, custom_patterns=MONGO_PATTERNS)
    values = []
    for k in range(600):
        q = rng.choice([b"a: 1", b"_id: { $gt: 5 }", b"x: { y: { z: 1 } }, w: 2", b"", b"name: \"ab } cd\""])
        word = rng.choice([b"ntoreturn", b"ntoreturn", b"ntoreturns", b"limit"])
        tail = b" ntoskip:%d nscanned:%d keyUpdates:0 locks(micros) r:%d nreturned:%d reslen:20 %dms" % (
            rng.randint(0, 9), rng.randint(0, 99999), rng.randint(1, 999), rng.randint(0, 50), rng.randint(1, 9000))
        line = b"query db-%d.coll_%d query: { " % (k % 7, k % 5) + q + b" } " + word + b":%d" % rng.randint(0, 100) + tail
        if k % 11 == 0:
            line = line.replace(b" } ntoreturn:", b" }ntoreturn:")
        if k % 13 == 0:
            line = b"junk " + line + b" trailing"
        if k % 7 == 3:   # the slow-query format broken behind the query: only the second entry (the query alone) can match
            line = line.replace(b" nreturned:", b" returned:")
        values.append(line)
    pattern, fields = g.match_host(values)
    won = [0, 0]
    for v, p, f in zip(values, pattern, fields):
        res, want = o.process_value(v)
        assert f == want, v
        assert (p >= 0) == (res == 0)
        if p >= 0:
            won[int(p)] += 1
    assert won[0] > 200 and won[1] > 30, won


def test_device_resident_entry_and_extra_row_overflow(torch_dev):
    torch = torch_dev
    dev = torch.device("cuda:0")
    g = Grok(Match=["%{WORD:w}"])
    o = GrokOracle(["%{WORD:w}"])
    values = [b"a b c d e f g h", b"", b"one", b"x y"] * 64
    n = len(values)
    data = np.frombuffer(b"".join(values) + b"\0" * 16, dtype=np.uint8)
    length = np.array([len(v) for v in values], dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(length[:-1])]).astype(np.uint32)
    d_data = torch.from_numpy(data.copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev)
    d_len = torch.from_numpy(length.view(np.int32).copy()).to(dev)
    row = g.row_ints
    d_pattern = torch.empty(n, dtype=torch.int32, device=dev)
    d_first = torch.empty((n, row), dtype=torch.int32, device=dev)
    d_nextra = torch.zeros(1, dtype=torch.int32, device=dev)
    d_scratch = torch.empty(g.scratch_bytes(n), dtype=torch.uint8, device=dev)
    small = torch.empty((8, row + 2), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):   # LC_ERR_OVERFLOW: 8 rows cannot hold the further matches
        g.match_device(d_data, d_off, d_len, n, d_pattern, d_first, small, d_nextra, d_scratch)
    need = int(d_nextra.cpu()[0])
    assert need == sum(max(0, len(v.split()) - 1) for v in values)
    d_extra = torch.empty((need, row + 2), dtype=torch.int32, device=dev)
    g.match_device(d_data, d_off, d_len, n, d_pattern, d_first, d_extra, d_nextra, d_scratch)
    pattern, first, extra = d_pattern.cpu().numpy(), d_first.cpu().numpy(), d_extra.cpu().numpy()
    rows = {}
    for r in extra:
        rows.setdefault(int(r[0]), []).append(r)
    for i, v in enumerate(values):
        _, want = o.process_value(v)
        if not want:
            assert pattern[i] == -1
            continue
        got = [v[first[i][2]:first[i][3]]] + [v[r[4]:r[5]] for r in sorted(rows.get(i, []), key=lambda r: r[1])]
        assert got == [w for _, w in want]


def test_config3_supported_patterns_on_generated_lines(torch_dev, golden_dir):
    """BASELINE.json configs[2]: the whole 50-entry Match list of the example_config, first match wins, against the oracle --
    on random values and on 3 000 lines of the synthetic corpus tools/grok_bench.py measures (every family of formats,
    IPv4 and IPv6, 26..4096 bytes, 5 % junk)."""
    from loongcollector_amd.grok_corpus import grok_lines
    with open(os.path.join(golden_dir, "grok_config3.json"), encoding="utf-8") as f:
        cfg = json.load(f)
    ok = []
    for m in cfg["match"]:
        try:
            Grok(Match=[m], CustomPatterns=cfg["custom_patterns"], AnchoredFirst=False)
            ok.append(m)
        except GrokInitError:
            pass
    assert len(ok) == 50, len(ok)
    g = Grok(Match=ok, CustomPatterns=cfg["custom_patterns"])
    o = GrokOracle(ok, custom_patterns=cfg["custom_patterns"])
    rng = random.Random(3)
    values = _random_values(rng, 400) + [
        b"Mar 16 00:01:25 evita CRON[1713]: (root) CMD (run-parts /etc/cron.hourly)",
        b"%ASA-4-106023: Deny tcp src outside:10.1.1.1/1234 dst inside:10.2.2.2/80 by access-group \"acl\" [0x0, 0x0]",
        b"%ASA-6-302010: 5 in use, 10 most used",
        b"%ASA-1-104001: (Primary) Switching to ACTIVE - reason",
        b"    at com.example.Foo.bar(Foo.java:42)",
    ] + grok_lines(3000)
    pattern, fields = g.match_host(values)      # (right after Init: the warm-up thread has hardly delivered an anchored search yet)
    hits, winners = 0, set()
    for v, p, f in zip(values, pattern, fields):
        res, want = o.process_value(v)
        assert p != -2, v
        assert f == want, v
        hits += p >= 0
        winners.add(int(p))
    assert hits >= 2800 and len(winners) >= 15
    # the same list with every anchored search in place (tried first on each value, tables in L2), and with none at all
    B.launched_kernels()
    pattern2, fields2 = g.wait_ready().match_host(values)
    assert "tdfa_l2_kernel" in B.launched_kernels()
    assert list(pattern2) == list(pattern) and fields2 == fields
    g0 = Grok(Match=ok, CustomPatterns=cfg["custom_patterns"], AnchoredFirst=False)
    pattern0, fields0 = g0.match_host(values)
    assert list(pattern0) == list(pattern) and fields0 == fields


def test_sixteen_runner_threads_share_device_batches(torch_dev, golden_dir):
    """core/runner/ProcessorRunner.cpp:138-142: one group per call, synchronous, from process_thread_count threads on ONE plugin
    instance.  Sixteen threads, twelve 250-value groups each (different sizes at the ends), through lc_grok_match_host: every group's
    pattern ids and fields equal what the same group gives alone (and a third of them, the oracle); the groups did travel together
    (csrc/group_combiner.hpp) -- far fewer batches than groups, a batch of at least eight groups seen."""
    import threading
    from loongcollector_amd.grok_corpus import grok_lines
    with open(os.path.join(golden_dir, "grok_config3.json"), encoding="utf-8") as f:
        cfg = json.load(f)
    g = Grok(Match=cfg["match"], CustomPatterns=cfg["custom_patterns"]).wait_ready()
    o = GrokOracle(cfg["match"], custom_patterns=cfg["custom_patterns"])
    lines = grok_lines(2400)
    rng = random.Random(11)
    groups = []
    at = 0
    while at < len(lines):
        n = rng.choice([1, 7, 250, 250, 250, 250, 400])
        groups.append(lines[at:at + n])
        at += n
    alone = [g.match_host(gr) for gr in groups]
    for k in range(0, len(groups), 3):
        for v, f in zip(groups[k], alone[k][1]):
            assert f == o.process_value(v)[1], v
    before = g.combiner_stats()
    T, rounds = 16, 12
    errors = []
    barrier = threading.Barrier(T)

    def runner(t):
        try:
            barrier.wait()
            for r in range(rounds):
                k = (t * 5 + r * 7) % len(groups)
                pattern, fields = g.match_host(groups[k])
                if list(pattern) != list(alone[k][0]) or fields != alone[k][1]:
                    errors.append((t, r, k))
        except Exception as e:   # noqa: BLE001
            errors.append((t, repr(e)))
        finally:
            B.load().lc_thread_release()

    threads = [threading.Thread(target=runner, args=(t,)) for t in range(T)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[:5]
    st = g.combiner_stats()
    n_groups, n_batches = st["groups"] - before["groups"], st["batches"] - before["batches"]
    assert n_groups == T * rounds
    assert n_batches <= n_groups // 3, st            # (sixteen Python threads: the interpreter lock staggers their calls)
    assert st["largest_batch_groups"] >= 8, st


def test_relaxed_screens_on_the_device(torch_dev, golden_dir):
    """lc_regex_screen_device (dfa_screen_kernel: one value per lane, the yes/no DFA's table in L2) against the same tables
    walked on the CPU, and against the oracle: a value the pattern matches somewhere is never rejected.  Whole list and a
    listed subset; lengths 26..4096, unaligned starts."""
    from loongcollector_amd.grok_corpus import grok_lines
    from oracle.oracle import ORX_NO_MOD_M, ORX_NO_MOD_S, ORX_REGEXP2, OracleRegex
    from tests.helpers.table_interp import TdfaInterp
    from tests.test_grok_host import GROK_SYNTAX
    with open(os.path.join(golden_dir, "grok_config3.json"), encoding="utf-8") as f:
        cfg = json.load(f)
    lib = Grok(CustomPatterns=cfg["custom_patterns"])
    values = grok_lines(600) + [b"", b"x"]
    length = np.array([len(v) for v in values], dtype=np.uint32)
    off = np.zeros(len(values), dtype=np.uint32)
    off[1:] = np.cumsum(length[:-1], dtype=np.uint64).astype(np.uint32)
    data = np.frombuffer(b"".join(values) + b"\0" * 32, dtype=np.uint8).copy()
    dev = torch_dev.device("cuda:0")
    d_data = torch_dev.from_numpy(data).to(dev)
    d_off = torch_dev.from_numpy(off.view(np.int32)).to(dev)
    d_len = torch_dev.from_numpy(length.view(np.int32)).to(dev)
    subset = np.arange(0, len(values), 3, dtype=np.uint32)
    d_subset = torch_dev.from_numpy(subset.view(np.int32)).to(dev)
    rejected_total = big = 0
    for name in ("COMMONAPACHELOG", "SYSLOGLINE", "CISCOFW106001", "CISCOFW302013_302014_302015_302016", "SHOREWALL", "TOMCATLOG"):
        pat = lib.denormalize("%{" + name + "}").encode("utf-8")
        scr = B.GpuRegex.compile_screen(pat, syntax_flags=GROK_SYNTAX & ~B.LC_SYNTAX_SEARCH, max_states=20000,
                                        max_table_bytes=2 << 20, relaxed=True)
        assert scr is not None, name
        big += scr.info()["states"] > 100        # (950 - 17 000 states as built; 120 - 300 once minimised)
        it = TdfaInterp(scr)
        want = np.array([it.fullmatch(v) is not None for v in values])
        for lines, d_lines in ((np.arange(len(values)), None), (subset, d_subset)):
            d_out = torch_dev.full((len(values),), -1, dtype=torch_dev.int32, device=dev)
            d_count = torch_dev.zeros((1,), dtype=torch_dev.int32, device=dev)
            scr.screen_device(d_data, d_off, d_len, len(lines), d_out, d_count, d_lines=d_lines,
                              stream=torch_dev.cuda.current_stream().cuda_stream)
            torch_dev.cuda.synchronize()
            k = int(d_count[0])
            got = np.sort(d_out.cpu().numpy()[:k])
            assert np.array_equal(got, lines[want[lines]]), (name, k, int(want[lines].sum()))
        o = OracleRegex(pat, ORX_NO_MOD_S | ORX_NO_MOD_M | ORX_REGEXP2)
        for v, w in zip(values[::5], want[::5]):
            assert w or o.search(v) is None, (name, v)
        rejected_total += int((~want).sum())
    assert big >= 5 and rejected_total > 2500 and "dfa_screen_kernel" in B.launched_kernels()


@pytest.mark.parametrize("name", ["HTTPD_ERRORLOG", "HAPROXYHTTP", "SYSLOGPAMSESSION", "NAGIOSLOGLINE"])
def test_wide_table_patterns_against_the_oracle(torch_dev, golden_dir, name):
    """> 64 byte classes (4-word class masks), > 64 / > 128 capture slots (NS=128 / NS=320 kernels), run captures:
    tests/helpers/wide_patterns.py"""
    from tests.helpers.wide_patterns import wide_values
    with open(os.path.join(golden_dir, "grok_config3.json"), encoding="utf-8") as f:
        cfg3 = json.load(f)
    match = ["%{" + name + "}"]
    g = Grok(Match=match, CustomPatterns=cfg3["custom_patterns"])
    assert g.engine(0) == B.LC_ENGINE_NFA
    o = GrokOracle(match, custom_patterns=cfg3["custom_patterns"])
    values = wide_values(mutations=12)
    pattern, fields = g.match_host(values)
    matched = 0
    for v, p, f in zip(values, pattern, fields):
        res, want = o.process_value(v)
        assert p != -2, v
        assert [(k, bytes(x)) for k, x in f] == [(k, bytes(x)) for k, x in want], (name, v)
        matched += bool(want)
    assert matched >= 5


def test_values_that_need_more_than_64_threads_are_decided(torch_dev, golden_dir):
    """CISCOFW305011 on an IPv6 address peaks at 71 live NFA threads: the second-chance kernel (two threads per lane) has
    to decide those values -- none may come back as -2, and the fields must be the oracle's."""
    from loongcollector_amd.grok_corpus import grok_lines
    with open(os.path.join(golden_dir, "grok_config3.json"), encoding="utf-8") as f:
        cfg3 = json.load(f)
    match = ["%{CISCOFW305011}"]
    g = Grok(Match=match, CustomPatterns=cfg3["custom_patterns"])
    o = GrokOracle(match, custom_patterns=cfg3["custom_patterns"])
    values = [v for v in grok_lines(40000) if v.startswith(b"Built dynamic")][:600]   # (one line in 48 is this format)
    pattern, fields = g.match_host(values)
    assert (np.asarray(pattern) != -2).all()
    hit = 0
    for v, p, f in zip(values, pattern, fields):
        _, want = o.process_value(v)
        assert [(k, bytes(x)) for k, x in f] == [(k, bytes(x)) for k, x in want], v
        hit += bool(want)
    assert hit >= 500


@pytest.mark.parametrize("match", [
    ["%{IPV4:ip}"],                                                      # many matches per value: rounds far beyond the queue
    ["%{LOGLEVEL:level}:? %{GREEDYDATA:msg}", "(?P<k>\\w+)=(?P<v>\\S*)", "%{INT:n}"],
    ["%{TIMESTAMP_ISO8601:ts}", "%{WORD:a} %{WORD:b}", "%{NOTSPACE:first}"],
    ["(?P<x>\\d+)|(?P<x>[a-z]+)_(?P<y>\\d)"],
    ["%{WORD:w}"] * 3 + ["%{GREEDYDATA:all}"],                           # later entries shadowed by an earlier one, a catch-all
])
def test_speculative_and_sequential_paths_agree(torch_dev, match):
    """The default path evaluates every (entry, value) pair that passes the screens at once and takes the first contributing
    entry afterwards; the sequential path walks the list (processor_grok.go:148-194 literally).  Same pattern ids, first rows
    and further matches on every value, and both equal the oracle."""
    rng = random.Random(5)
    values = _random_values(rng, 2500) + [b"", b" ", b"a" * 5000]
    spec = Grok(Match=match)
    seq = Grok(Match=match, Speculative=False)
    p1, f1, x1, s1 = _device_rows(torch_dev, spec, values)
    p2, f2, x2, s2 = _device_rows(torch_dev, seq, values)
    assert s1["speculative"] and not s2["speculative"]
    assert np.array_equal(p1, p2) and np.array_equal(f1, f2) and np.array_equal(x1, x2)
    # a second batch: the entries have learned how many rounds to queue ahead -- still the same rows, and (unless an entry
    # needs more rounds than can be queued) exactly FOUR host synchronisations: candidates per entry, round 0's counts, the remainder
    # screens' survivors, the end (round 4: the two in the middle replaced ~400 launches over lists that turn out empty)
    p3, f3, x3, s3 = _device_rows(torch_dev, spec, values)
    assert np.array_equal(p1, p3) and np.array_equal(f1, f3) and np.array_equal(x1, x3)
    # (round 5: THREE when no slot's remainder passes its entry's screen -- the host reads the survivors together with the results)
    assert s3["host_syncs"] <= 8, s3      # (an entry with dozens of matches per value goes on in stretches of rounds)
    assert s3["host_syncs"] in (3, 4) or s3["deferred_entries"] > 0, s3
    if match[0] != "%{IPV4:ip}":          # (up to 36 addresses per value there)
        assert s3["host_syncs"] in (3, 4), s3
    assert s2["host_syncs"] > s3["host_syncs"]
    o = GrokOracle(match)
    pattern, fields = spec.match_host(values)
    assert np.array_equal(np.asarray(pattern), p1)
    for v, p, f in zip(values[::7], pattern[::7], fields[::7]):
        res, want = o.process_value(v)
        assert f == want and (p >= 0) == (res == 0), (match, v)


def test_large_batch_prefix_screen_first_branch(torch_dev, golden_dir):
    """Sequential path, 'prefix screen first' branch (an entry that has both screens runs the prefix screen first only above
    PrefixScreenAbove carriers): forced with a low threshold on > 70 000 values, compared with the default path fed the same
    values in 4 Ki-value slices and with the oracle on a strided sample."""
    from loongcollector_amd.grok_corpus import grok_lines
    with open(os.path.join(golden_dir, "grok_config3.json"), encoding="utf-8") as f:
        cfg = json.load(f)
    match = ["%{SYSLOGLINE}", "%{CISCOFW106015}", "%{CISCOFW302013_302014_302015_302016}", "%{COMMONAPACHELOG}"]
    values = grok_lines(72000)
    kw = dict(Match=match, CustomPatterns=cfg["custom_patterns"], AnchoredFirst=False)
    g_prefix = Grok(Speculative=False, PrefixScreenAbove=1000, **kw)
    g_plain = Grok(Speculative=False, **kw)      # threshold 65536: most entries skip their prefix screen
    g_spec = Grok(**kw)
    pa, fa, xa, _ = _device_rows(torch_dev, g_prefix, values)
    pb, fb, xb, _ = _device_rows(torch_dev, g_plain, values)
    assert np.array_equal(pa, pb) and np.array_equal(fa, fb) and np.array_equal(xa, xb)
    ps, fs, xs = [], [], []
    for lo in range(0, len(values), 4096):
        p, f, x, st = _device_rows(torch_dev, g_spec, values[lo:lo + 4096])
        x = x.copy()
        if len(x):
            x[:, 0] += lo
        ps.append(p)
        fs.append(f)
        xs.append(x)
    assert np.array_equal(pa, np.concatenate(ps)) and np.array_equal(fa, np.concatenate(fs))
    assert np.array_equal(xa, np.concatenate([x for x in xs if len(x)] or [xa[:0]]))
    assert (pa >= 0).sum() > 5000 and (pa <= -2).sum() == 0
    o = GrokOracle(match, custom_patterns=cfg["custom_patterns"])
    idx = list(range(0, len(values), 24))
    ph, fh = g_prefix.match_host([values[i] for i in idx])
    assert np.array_equal(np.asarray(ph), pa[idx])
    for i, p, f in zip(idx, ph, fh):
        res, want = o.process_value(values[i])
        assert (p >= 0) == (res == 0) and f == want, values[i]


def test_plan_knobs_and_histories_do_not_change_a_result(torch_dev, golden_dir, monkeypatch):
    """Round 5's plan decides by an entry's HISTORY which kernel is its first chance (nfa_wide_kernel for an entry whose values needed
    more than 64 threads in recent batches) and whether its search rounds behind the first match are queued ahead, unscreened; it
    queues phase 2c's launches round-robin; and it runs the literal index over the remainders in front of the remainder screens.
    None of that may change a row: the 50-entry list of configs[2] on corpus lines -- every knob forced on, every knob off, and the
    default three batches in a row (no history, history, history) -- gives the rows of the sequential walk, and the oracle's fields."""
    from loongcollector_amd.grok_corpus import grok_lines
    with open(os.path.join(golden_dir, "grok_config3.json"), encoding="utf-8") as f:
        cfg = json.load(f)
    values = grok_lines(2500) + [b"", b"x" * 4096]
    seq = Grok(Match=cfg["match"], CustomPatterns=cfg["custom_patterns"], Speculative=False).wait_ready()
    want = _device_rows(torch_dev, seq, values)
    # (the history rules are about the thread-list kernels: this handle keeps the lazy automata out of their way; they get their turn below)
    spec = Grok(Match=cfg["match"], CustomPatterns=cfg["custom_patterns"], LazyTdfa=False).wait_ready()

    def same(got, what):
        assert np.array_equal(got[0], want[0]), what
        assert np.array_equal(got[1], want[1]), what
        assert np.array_equal(got[2], want[2]), what

    for k in range(3):   # batch 0 has no history; 1 and 2 go wide first / queue rounds ahead where batch 0 saw reason to
        B.launched_kernels()
        same(_device_rows(torch_dev, spec, values), "default, batch %d" % k)
    assert "nfa_wide_kernel:first" in B.launched_kernels()          # (CISCOFW formats on IPv6 addresses overflow 64 threads)
    forced = {"LC_GROK_WIDE_FIRST": "2", "LC_GROK_EARLY_ROUNDS": "2"}
    off = {"LC_GROK_WIDE_FIRST": "0", "LC_GROK_EARLY_ROUNDS": "0", "LC_GROK_REMAINDER_LITERAL": "0", "LC_GROK_REMAINDER_WON": "0",
           "LC_GROK_FUSED_ROUND0": "0", "LC_GROK_SCREEN_SCALED": "0", "LC_GROK_FLAT": "0", "LC_GROK_SCREEN_TRANSPOSED": "0", "LC_GROK_LITERAL_LDS": "0"}
    # (round 6) the remainder screens queued ahead of the host's read of round 0's counts: with the search rounds forced ahead (the
    # entries then leave the launch through its skip mask)
    ahead_rounds = {"LC_GROK_EARLY_ROUNDS": "2"}
    ahead_levels = {"LC_GROK_FLAT": "0"}   # (shadowed entries wait for the entries of level 0: not in the launch either)
    for knobs in (forced, off, ahead_rounds, ahead_levels):
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        fresh = Grok(Match=cfg["match"], CustomPatterns=cfg["custom_patterns"]).wait_ready()
        same(_device_rows(torch_dev, fresh, values), knobs)
        same(_device_rows(torch_dev, fresh, values), knobs)
        for k in knobs:
            monkeypatch.delenv(k)
    # Round 6: the LAZY automata in front of the entries that do not determinise (include/lc_grok.h).  Batches behind a settled trainer
    # -- the automata grow from batch to batch --, then the same handle with LC_LAZY_TDFA=0 (the thread-list kernels alone) and on again.
    lazy = Grok(Match=cfg["match"], CustomPatterns=cfg["custom_patterns"]).wait_ready()
    for k in range(4):
        B.launched_kernels()
        same(_device_rows(torch_dev, lazy, values), "lazy automata, batch %d" % k)
        assert lazy.lazy_settle(120000)
    st = lazy.lazy_stats()
    assert st["automata_in_use"] >= 30 and st["values_kept"] > 0 and st["batches_taken"] >= 1, st
    B.launched_kernels()
    same(_device_rows(torch_dev, lazy, values), "lazy automata, settled")
    assert "tdfa_l2_kernel:wave:lazy" in B.launched_kernels()
    monkeypatch.setenv("LC_LAZY_TDFA", "0")
    B.launched_kernels()
    same(_device_rows(torch_dev, lazy, values), "LC_LAZY_TDFA=0")
    assert "lazy" not in B.launched_kernels()
    monkeypatch.delenv("LC_LAZY_TDFA")
    same(_device_rows(torch_dev, lazy, values), "LC_LAZY_TDFA back on")
    o = GrokOracle(cfg["match"], custom_patterns=cfg["custom_patterns"])
    pattern, fields = spec.match_host(values)
    assert np.array_equal(np.asarray(pattern), want[0])
    pattern_l, fields_l = lazy.match_host(values)
    assert list(pattern_l) == list(pattern) and fields_l == fields
    for v, p, f in zip(values[::5], pattern[::5], fields[::5]):
        res, exp = o.process_value(v)
        assert f == exp and (p >= 0) == (res == 0), v
