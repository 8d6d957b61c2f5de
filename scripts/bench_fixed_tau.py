"""Throughput of the fixed-tau chain (dsm_ctx_gibbs_update_fixed_tau) -> profiles/fixed_tau_bench.json.

    python scripts/bench_fixed_tau.py [--out profiles/fixed_tau_bench.json] [--iters 200] [--reps 7]

Per shape: 200 iterations with pool = 0 and pool = 1, and dsm_ctx_gibbs_update on the same table in the same process for scale (the
full iteration is the only thing there is to compare against).  HIP events around the call (it returns with its stream drained), a
warm-up call, median of --reps.  tau is the generating one, so the table holds as many words as its strains form (W is recorded).
A pooled call pays its set-up -- sorting the words, the pooling pass, loading the scratch chain -- inside the timed bracket.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(10000, 64, 3), (10000, 64, 5), (10000, 64, 8), (10000, 4, 5)]          # V, S, G


def timed(fn, reps):
    import torch
    fn()                                                                 # warm-up
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [float(x) for x in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixed_tau_bench.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch                                                         # before the library: one HIP runtime per process, torch's
    from desman_amd import _lib
    from desman_amd.synth import synth_counts
    from oracle import cbind
    rows = []
    for V, S, G in CASES:
        counts, tau_true, gamma_true = synth_counts(V, S, G, seed=V + S + G)
        tau = cbind.idx_to_onehot(tau_true)
        eta = 0.96 * np.eye(4) + 0.01
        ctx = _lib.Context(0)
        ctx.set_counts(counts)

        def start():
            ctx.set_state(tau, np.ascontiguousarray(gamma_true), eta)
            ctx.seed(7)

        start()
        W = ctx.debug_fixtau_pool()["W"]
        row = dict(V=V, S=S, G=G, W=W, iters=a.iters, stats_spec=ctx.stats_spec())
        for name, fn in (("fixed_tau_pool0", lambda: ctx.gibbs_update_fixed_tau(a.iters, pool=0)),
                         ("fixed_tau_pool1", lambda: ctx.gibbs_update_fixed_tau(a.iters, pool=1)),
                         ("gibbs_update", lambda: ctx.gibbs_update(a.iters))):
            start()
            ms, every = timed(fn, a.reps)
            row[name] = dict(event_ms_median=ms, event_ms_all=every, us_per_iter=1e3 * ms / a.iters)
            print("V=%d S=%d G=%d W=%d %-16s %8.3f ms / %d iterations = %7.2f us per iteration" % (V, S, G, W, name, ms, a.iters, 1e3 * ms / a.iters),
                  flush=True)
        rows.append(row)
        ctx.close()
    out = dict(what="dsm_ctx_gibbs_update_fixed_tau, pool 0 / 1, against dsm_ctx_gibbs_update on the same table in the same process",
               device=torch.cuda.get_device_name(0),
               timing="HIP events around the call, warm-up call, median of reps; a pooled call's set-up is inside the bracket",
               not_measured=["where the auto rule (pool iff W < V) stops paying", "tables whose words are all distinct (W = V)",
                             "fix_eta = 1", "a target: nothing exists to compare against but the full iteration above"],
               cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
