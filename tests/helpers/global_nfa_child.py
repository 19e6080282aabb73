"""Test-only: the body of the ONE child process of tests/test_gpu_chunk_edges.py test_global_memory_nfa_kernel_in_a_process_of_its_own.
LC_NFA_GLOBAL_KB is read once per process; with LC_NFA_GLOBAL_KB=0 in the environment every non-empty batch takes
nfa_match_kernel<..., GLOBAL=true> (the program stays in global memory, LDS holds the scratch alone).  main() runs rows `nfa` and
`nfa-atomic` of the instantiation table in both input forms, the resumed searches, and the result edges on `log`, then rows `nfa-ns64`,
`nfa-ns128` and `nfa-ns320` (the slot-by-slot capture transfer with 4 and 10 tag words, the accumulation registers) in both forms, family
`alog` of row `nfa-atomic-edges` and row `achain-kept64` (the atomic instantiation's commit pass and its hand-off to nfa_decide_kernel,
with lc_decide_stats exact) in both forms, compares with the
oracle's rows behind sentinels, and prints one JSON object: per launch the number of values that differ and the first, the kernel
names, and where the time went.  Not part of the product."""
import json
import os
import sys
import time

T0 = time.perf_counter()


def main():
    assert os.environ.get("LC_NFA_GLOBAL_KB") == "0" and os.environ.get("LC_LAZY_TDFA") == "0"
    import numpy as np
    import torch
    from tests.helpers import chunk_edges as ce
    from tests.helpers.chunk_edge_launch import cut, decide_stats, differing, launch, make_batches, rows
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")
    t_imports = time.perf_counter() - T0
    batches = make_batches(torch)
    out = {"launches": [], "kernels": []}

    def note(row, where, names, batch, caps, status, exp_caps, exp_status, listed=None):
        n, first = differing(batch, caps, status, exp_caps, exp_status, where, listed)
        out["launches"].append({"launch": where, "differ": n, "first": first, "ran": row.kernel in names})
        out["kernels"] = sorted(set(out["kernels"]) | set(names))

    for row in (r for r in ce.ROWS if r.id in ("nfa", "nfa-atomic", "nfa-atomic-edges", "achain-kept64") + tuple(ce.NS_ROWS)):
        assert row.env == {"LC_LAZY_TDFA": "0"} and not row.dfs and not row.min_n
        for family in (("alog",) if row.id == "nfa-atomic-edges" else row.families):
            rx = ce.compile_row(row, family)
            batch = batches(family, row.walk)
            c, o = batch["corpus"], batch["oracle"]
            for form in ("len", "sep"):
                caps, status, names = launch(torch, row, rx, batch, form)
                note(row, "%s, %s, %s form" % (row.id, family, form), names, batch, caps, status, batch["caps"], batch["status"])
                if (row.id, family) in ce.DECIDES:      # the values sent on: exactly the overflow variants, none given up, no wide kernel
                    sent = (sum(c.family.overflows(k) for k in c.cases), 0)
                    out["launches"][-1]["ran"] = (row.kernel in names and "nfa_decide_kernel" in names and decide_stats() == sent
                                                  and not [x for x in names if x.startswith("nfa_wide")])
            if c.family.search:
                frm = c.frm()
                exp_caps, exp_status = rows(c.family, [o.search(k.line, int(f)) for k, f in zip(c.cases, frm)], batch["G"])
                for form in ("len", "sep"):
                    caps, status, names = launch(torch, row, rx, batch, form, frm=frm)
                    note(row, "%s, %s, resumed, %s form" % (row.id, family, form), names, batch, caps, status, exp_caps, exp_status)
            if family != "log":
                continue
            # the result edges, as test_result_edges asks them of every row
            N, G = batch["n"], batch["G"]
            cuts = (513, 515)
            subset = np.random.default_rng(7).permutation(N)[:cuts[1]]

            def edge(where, ngroups=G, listed=None, **kw):
                caps, status, names = launch(torch, row, rx, batch, ngroups=ngroups, **kw)
                note(row, "%s, log, %s" % (row.id, where), names, batch, caps, status, cut(batch["caps"], ngroups), batch["status"], listed)

            for shift in (0, 1, 2, 3):
                for ngroups in (0, 1, G, G + 3):
                    edge("table %d bytes off, %d groups" % (4 * shift, ngroups), ngroups=ngroups, form="len" if shift % 2 else "sep", caps_shift=shift)
            for k, n in enumerate(cuts):
                edge("%d values" % n, form="len", caps_shift=k % 2, n=n, listed=range(n))
            edge("a permuted subset of %d" % len(subset), form="len", n=len(subset), lines=subset, listed=subset)
            edge("a permuted subset of %d, separator form" % len(subset), form="sep", caps_shift=1, n=len(subset), lines=subset, listed=subset)
            edge("%d of %d values by the count on the device" % (cuts[0], N), form="sep", n=N, nlines=cuts[0], listed=range(cuts[0]))
            edge("%d of the subset by the count on the device" % cuts[0], form="len", n=len(subset), lines=subset, nlines=cuts[0], listed=subset[:cuts[0]])
    out["seconds"] = {"imports": round(t_imports, 2), "work": round(time.perf_counter() - T0 - t_imports, 2)}
    sys.stdout.write(json.dumps(out) + "\n")
