"""Test-only: the launches of tests/test_gpu_decide_launch.py.  run() is one guarded LC_ENGINE_DECIDE launch of a case of
tests/helpers/decide_launch_cases.py and its comparison; main() is the body of the ONE child process with LC_DECIDE_POOL_MB=8 (read once
per process): launches a to f at the pool's minimum, then the parse processor on values the thread-list kernels overflow on (g), and one
JSON object on stdout: per launch the number of rows that differ from the expectation and the first, lc_decide_stats against the exact
pair, whether nfa_decide_kernel was among the launched kernels, the planner's branch by the restated arithmetic, and the wall time.
Not part of the product."""
import json
import os
import sys
import time

import numpy as np

T0 = time.perf_counter()

UNLISTED_FRONT, UNLISTED_BACK = 1, 2      # rows of the batch no launch lists: they must keep what they held


def set_budget(budget):
    """LC_DECIDE_BUDGET is read per launch"""
    if budget is None:
        os.environ.pop("LC_DECIDE_BUDGET", None)
    else:
        os.environ["LC_DECIDE_BUDGET"] = str(budget)


_compiled = {}


def compiled(pattern, flags):
    from loongcollector_amd import binding as B
    if (pattern, flags) not in _compiled:
        _compiled[(pattern, flags)] = B.GpuRegex(pattern, syntax_flags=flags, engine=B.LC_ENGINE_NFA)
    return _compiled[(pattern, flags)]


def run(torch, launch, pool, budget="its own"):
    """One launch through LC_ENGINE_DECIDE over the rows d_lines lists (the launch's values; a row in front of them and two behind are
    not listed), every status byte -- guards and unlisted rows included -- pre-filled with LC_OVERFLOW, the capture rows with their
    sentinel.  -> the record main() prints: rows that differ from cases.expected(), the stats pair, the kernel names, the seconds."""
    from loongcollector_amd import binding as B
    from tests.helpers import decide_launch_cases as dl
    from tests.helpers.chunk_edge_launch import decide_stats
    from tests.helpers.guarded_launch import CAPS_SENTINEL, GuardedResults
    dev = torch.device("cuda:0")
    budget = launch.budget if budget == "its own" else budget
    exp_caps, exp_status, want_stats, pl = dl.expected(launch, pool, budget)
    rx = compiled(launch.pattern, launch.flags)
    n = len(launch.values)
    rows = [b"b"] * UNLISTED_FRONT + list(launch.values) + [b"b"] * UNLISTED_BACK
    N = len(rows)
    listed = np.arange(UNLISTED_FRONT, UNLISTED_FRONT + n)
    data, off, length = dl.pack(rows)
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).to(dev)
    d_data = torch.from_numpy(data.copy()).to(dev)
    d_off, d_len, d_lines = i32(off), i32(length), i32(listed)
    d_from = None
    if launch.frm is not None:
        frm = np.zeros(N, np.uint32)
        frm[listed] = launch.frm
        d_from = i32(frm)
    assert exp_caps.shape[1] == 2 * rx.groups
    res = GuardedResults(torch, N, rx.groups, 0, B.LC_OVERFLOW)
    set_budget(budget)
    torch.cuda.synchronize()
    B.launched_kernels()
    t0 = time.perf_counter()
    try:
        rx.match_device_from(d_data, d_off, d_len, n, res.d_caps, res.d_status, d_lines=d_lines, d_from=d_from,
                             stream=torch.cuda.current_stream().cuda_stream, engine=B.LC_ENGINE_DECIDE)
        torch.cuda.synchronize()
    finally:
        set_budget(None)
    seconds = time.perf_counter() - t0
    names = B.launched_kernels().split(", ")
    stats = decide_stats()
    caps, status = res.read(launch.name)
    untouched = (status == B.LC_OVERFLOW) & (caps == CAPS_SENTINEL).all(axis=1)
    took = np.zeros(N, bool)
    took[listed] = True
    got_caps, got_status = caps[listed], status[listed]
    wrong = (got_status != exp_status) | (got_caps != exp_caps).any(axis=1)
    # the values the list had no room for: exactly `dropped` rows, whichever lost the race, read LC_GAVE_UP with a row of -1
    dropped = wrong & (got_status == B.LC_GAVE_UP) & (got_caps == -1).all(axis=1) if pl.dropped else np.zeros(n, bool)
    bad = np.nonzero(wrong & ~dropped)[0]
    first = None
    if bad.size:
        i = int(bad[0])
        first = "value %d of %d bytes: expected status %d row %s, actual status %d row %s" % (
            i, len(launch.values[i]), int(exp_status[i]), exp_caps[i].tolist(), int(got_status[i]), got_caps[i].tolist())
    return {"launch": launch.name, "differ": int(bad.size), "first": first, "dropped": int(dropped.sum()), "want_dropped": pl.dropped,
            "unlisted_touched": int((~untouched[~took]).sum()), "stats": list(stats), "want_stats": list(want_stats),
            "gave_up_rows": int((got_status == B.LC_GAVE_UP).sum()), "ran": "nfa_decide_kernel" in names, "kernels": names,
            "branch": pl.branch, "workers": pl.workers, "seconds": round(seconds, 3)}


def bad_launches(records):
    """the records a test fails on"""
    return [r for r in records if r["differ"] or r["unlisted_touched"] or r["dropped"] != r["want_dropped"] or r["stats"] != r["want_stats"]
            or not r["ran"]]


def run_processor(keep_fail):
    """g: processor_parse_regex_gpu behind the NFA engine on six values that all overflow the thread-list kernels; under the budget two
    of the long ones give up.  The expectation: ProcessorOracle with exactly those two values made to fail."""
    from loongcollector_amd import binding as B
    from loongcollector_amd.processor import EventGroup, Processor
    from oracle.processor_oracle import LogEventModel, ProcessorOracle
    from tests.helpers import decide_launch_cases as dl
    from tests.helpers.chunk_edge_launch import decide_stats
    g_long = dl.G_LONG
    vals = [dl.w_over(341, 200, match=True), g_long[0], g_long[1], dl.w_over(330), g_long[2], g_long[3]]
    gives_up = [2, 4]
    assert [dl.plain_steps(dl.W, 0, v, 0) > dl.G_BUDGET for v in g_long] == [False, True, True, False]
    cfg = {"SourceKey": "content", "Regex": dl.W.decode(), "Keys": ["head", "tail"], "KeepingSourceWhenParseFail": keep_fail, "_Engine": "nfa"}
    marker = lambda i: b"\x01given up %d\x01" % i
    po = ProcessorOracle({k: v for k, v in cfg.items() if k != "_Engine"})
    out = po.process_group([LogEventModel([("content", marker(i) if i in gives_up else v)]) for i, v in enumerate(vals)])
    back = {marker(i).decode(): vals[i].decode() for i in gives_up}
    want = [[(k, back.get(v.decode(), v.decode())) for k, v in ev.live()] for ev in out]
    p, g = Processor(cfg), EventGroup({"events": [{"contents": [["content", v.decode()]], "timestamp": 1, "type": 1} for v in vals]})
    set_budget(dl.G_BUDGET)
    B.launched_kernels()
    t0 = time.perf_counter()
    try:
        p.process(g)
    finally:
        set_budget(None)
    seconds = time.perf_counter() - t0
    names = B.launched_kernels().split(", ")
    c = p.counters()
    got = [[tuple(kv) for kv in ev] for ev in g.contents()]
    return {"keep_fail": keep_fail, "events_equal": got == want, "events": len(got), "want_events": len(want),
            "parsed": sum(1 for ev in got if dict(ev).get("head") is not None),
            "counters": {k: int(c[k]) for k in ("discarded_events_total", "out_failed_events_total", "out_successful_events_total",
                                                "complexity_exceeded_events_total", "undecided_events_total")},
            "oracle": {k: int(po.counters[k]) for k in ("discarded", "out_failed", "out_successful")},
            "stats": list(decide_stats()), "ran": "nfa_decide_kernel" in names, "kernels": names, "seconds": round(seconds, 3)}


CHILD_LAUNCHES = ("a", "b", "c, budget S", "c, budget S + 1", "c, budget unset", "d, from L - 60", "d, from 0", "e", "f, list + 5", "f, list")


def main():
    assert os.environ.get("LC_DECIDE_POOL_MB") == "8" and os.environ.get("LC_LAZY_TDFA") == "0"
    import torch
    from tests.helpers import decide_launch_cases as dl
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")
    t_imports = time.perf_counter() - T0
    L = dl.launches()
    out = {"launches": [run(torch, L[name], dl.POOL_SMALL) for name in CHILD_LAUNCHES]}
    out["processor"] = [run_processor(keep_fail) for keep_fail in (True, False)]
    out["seconds"] = {"imports": round(t_imports, 2), "work": round(time.perf_counter() - T0 - t_imports, 2)}
    sys.stdout.write(json.dumps(out) + "\n")
