"""The LAUNCH around the depth-first decide walk (gpu_runtime.hip launchDecide; nfa_decide_kernel.hpp nfa_decide_plan_kernel and the
worker loop of nfa_decide_kernel) on the device: every outcome of the planner, the walk without the memo on either side of its step
budget, and both give-up exits of the scratch.  The walk itself is pinned by tests/test_gpu_decide.py; here the question is who gets the
memo, who walks under LC_DECIDE_BUDGET, who finds no room -- and that nothing else of a launch changes with it.

Which outcome a launch takes depends on the pool (LC_DECIDE_POOL_MB, read once per process), so the launches at the pool's minimum of
8 MiB run in ONE child process (tests/helpers/decide_child.py); the parent reruns three of them at the default 256 MiB, where every
value has the memo.  Cases, the restated planner and the step counts: tests/helpers/decide_launch_cases.py, each of its conditions
checked on the CPU by tests/test_decide_launch_model.py.  Every launch goes through LC_ENGINE_DECIDE over listed rows, with every status
byte pre-filled with LC_OVERFLOW (unlisted rows and guards included), and is compared in four ways: rows against OracleRegex, or
exactly LC_GAVE_UP with a row of -1; lc_decide_stats against the exact (listed, given up) pair; unlisted rows untouched;
nfa_decide_kernel among the launched kernels.

Time (MI355X, the first measured run): the child 3.9 s wall -- 1.6 s imports, 1.9 s launches, oracle and processor; no launch above
0.25 s (the three 200 000-step walks of c, side by side: 1.1 us per step), f 0.03 s per launch, g 0.15 s per group -- and the parent's
four launches 0.3 s.  Three times the child's 3.9 s is 12 s; CHILD_TIMEOUT is 45 s, because the start of an interpreter with torch on
a machine that has not loaded it yet is not something the factor of three was measured on.  A launch at the real bound of 2^22 steps
was measured at 5.4 s (decided at 2^22 steps, LC_GAVE_UP at 2^22 + 1) and is left out for its time."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests.helpers import decide_child as dc
from tests.helpers import decide_launch_cases as dl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 45


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def child():
    """the one child process: LC_DECIDE_POOL_MB=8, LC_LAZY_TDFA=0.  A child that faults, aborts or runs out of time fails the tests with
    its stderr; nothing is started afterwards."""
    env = dict(os.environ)
    for k in ("LC_DECIDE_BUDGET", "LC_NFA_NO_DECIDE", "LC_NFA_DFS", "LC_NFA_NO_WIDE", "LC_NFA_WIDE_FIRST", "LC_NFA_GLOBAL_KB", "LC_HOST_ZEROCOPY"):
        env.pop(k, None)
    env.update(LC_DECIDE_POOL_MB="8", LC_LAZY_TDFA="0")
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, "-c", "from tests.helpers.decide_child import main; main()"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, "the child ended with status %d\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print("decide launch child: %.1f s wall, of which imports %.1f s, launches, oracle and processor %.1f s" % (
        wall, res["seconds"]["imports"], res["seconds"]["work"]))
    for r in res["launches"]:
        print("  %-16s %-26s %3d workers  stats %-14s %.3f s" % (r["launch"], r["branch"], r["workers"], tuple(r["stats"]), r["seconds"]))
    for r in res["processor"]:
        print("  g, keep source %-5s stats %-14s %.3f s" % (r["keep_fail"], tuple(r["stats"]), r["seconds"]))
    return res


def test_the_launches_at_the_smallest_pool(child):
    """Launches a to f with an 8 MiB pool.
    a  200 values of (a|aa)*b, budget 1000: all have the memo (a walk without it would stop at step 1001), workers take several values.
    b  128 values of 4096 bytes: 22 workers keep the memo (128 x 372 900 bytes do not fit), budget 1000 < 2L: all decided.
    c  three values of 100 000 bytes walk WITHOUT the memo beside three short ones that still have it: with budget S = 200 142 the value
       that takes S steps is decided and the one that takes S + 1 is LC_GAVE_UP -- the kernel counts steps as the model does; with
       S + 1 and with the variable unset (2^22) nothing is given up.
    d  a search resumed 60 bytes before the end of a 100 000-byte value: 61 frames, the memo fits (303 steps; 3843 without it, more
       than the budget); the same value from 0 walks without the memo and gives up at step 1001.
    e  a value whose frame stack alone (9 MB) exceeds the pool: one worker with the whole pool, exactly that value LC_GAVE_UP, the ten
       others decided (a plan of no workers gave them all up).
    f  524 272 + 5 one-byte values: the list holds 524 272; exactly five rows, whichever, are LC_GAVE_UP with a row of -1, stats
       (524 272, 5); with 524 272 values none."""
    records = child["launches"]
    assert [r["launch"] for r in records] == list(dc.CHILD_LAUNCHES)
    bad = dc.bad_launches(records)
    assert not bad, "%d of %d launches differ; first: %s" % (len(bad), len(records), bad[0])
    by = {r["launch"]: r for r in records}
    assert [tuple(by[k]["stats"]) for k in dc.CHILD_LAUNCHES] == [
        (200, 0), (128, 0), (6, 1), (6, 0), (6, 0), (1, 0), (1, 1), (11, 1), (524272, 5), (524272, 0)]
    assert [by[k]["gave_up_rows"] for k in dc.CHILD_LAUNCHES] == [0, 0, 1, 0, 0, 0, 1, 1, 5, 0]
    assert [(by[k]["branch"], by[k]["workers"]) for k in ("a", "b", "c, budget S", "d, from 0", "e", "f, list + 5")] == [
        ("memo for all", 128), ("fewer workers", 22), ("no memo", 4), ("no memo", 1), ("one worker", 1), ("memo for all + list full", 128)]


def test_the_parse_processor_counts_what_the_decide_launch_gives_up(child):
    """g: processor_parse_regex_gpu, `_Engine: nfa`, six values the thread-list kernels overflow on; four of 40 000 to 100 001 bytes walk
    without the memo, and the budget lies on the last step of the first: two give up.  They are parse failures AND counted as
    complexity-exceeded, nothing is undecided; events and counters are ProcessorOracle's with those two values made to fail."""
    assert [r["keep_fail"] for r in child["processor"]] == [True, False]
    for r in child["processor"]:
        assert r["ran"] and tuple(r["stats"]) == (6, 2), r
        assert r["events_equal"] and r["events"] == r["want_events"], r
        c, o = r["counters"], r["oracle"]
        assert (c["complexity_exceeded_events_total"], c["undecided_events_total"]) == (2, 0), r
        assert (c["discarded_events_total"], c["out_failed_events_total"], c["out_successful_events_total"]) == (
            o["discarded"], o["out_failed"], o["out_successful"]), r
        assert c["out_failed_events_total"] == 4 and r["parsed"] == 2, r


def test_the_same_launches_at_the_default_pool(torch_dev, monkeypatch):
    """256 MiB (LC_DECIDE_POOL_MB unset in this process): a, b and the three long values of c have the memo, every value is decided as
    the oracle says, stats (n, 0) -- with the budget unset, and a once more with LC_DECIDE_BUDGET=1000: the knob does not touch the
    memo walk's budget (7n steps would fit either way; the point is that nothing else moved)."""
    assert "LC_DECIDE_POOL_MB" not in os.environ
    monkeypatch.delenv("LC_DECIDE_BUDGET", raising=False)
    L = dl.launches()
    records = [dc.run(torch_dev, L[name], dl.POOL_DEFAULT, budget=None) for name in ("a", "b", "c-long")]
    records.append(dc.run(torch_dev, L["a"], dl.POOL_DEFAULT, budget=1000))
    for r in records:
        print("  %-16s %-26s %3d workers  stats %-14s %.3f s" % (r["launch"], r["branch"], r["workers"], tuple(r["stats"]), r["seconds"]))
    bad = dc.bad_launches(records)
    assert not bad, "%d of %d launches differ; first: %s" % (len(bad), len(records), bad[0])
    assert [tuple(r["stats"]) for r in records] == [(200, 0), (128, 0), (3, 0), (200, 0)]
    assert [r["branch"] for r in records] == ["memo for all"] * 4 and not any(r["gave_up_rows"] for r in records)
    assert "LC_DECIDE_BUDGET" not in os.environ
