"""Cost of the partly held chain (dsm_ctx_gibbs_update_held_tau, dsm_ctx_sample_tau_held) -> profiles/held_tau_bench.json.

    python scripts/bench_held_tau.py [--out profiles/held_tau_bench.json] [--iters 200] [--sweeps 50] [--reps 7]

At V = 10 000, S = 64 and (G, n_held) in {(8, 7), (8, 4), (5, 4), (12, 11)}, in one process: the held iteration, dsm_ctx_gibbs_update and
the fixed-tau call with pool = 0 on the same table (us per iteration over --iters iterations), and the held sweep alone against the
full sweep alone (us per sweep over --sweeps calls of dsm_ctx_sample_tau_held / dsm_ctx_sample_tau, each of which returns with its
stream drained: the figure includes the call's launch and read-back).  HIP events around the calls, one warm-up call, median of --reps.
There is no target; the file records what came out.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, S = 10000, 64
CASES = [(8, 7), (8, 4), (5, 4), (12, 11)]                                # G, n_held


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "held_tau_bench.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch                                                         # before the library: one HIP runtime per process, torch's
    from desman_amd import _lib
    from desman_amd.synth import synth_counts
    from oracle import cbind
    rows = []
    for G, n_held in CASES:
        counts, tau_true, gamma_true = synth_counts(V, S, G, seed=V + S + G)
        tau = cbind.idx_to_onehot(tau_true)
        eta = 0.96 * np.eye(4) + 0.01
        ctx = _lib.Context(0)
        ctx.set_counts(counts)

        def start():
            ctx.set_state(tau, np.ascontiguousarray(gamma_true), eta)
            ctx.seed(7)

        def sweeps(fn):
            for _ in range(a.sweeps):
                fn()

        start()
        row = dict(V=V, S=S, G=G, n_held=n_held, iters=a.iters, sweeps=a.sweeps, stats_spec=ctx.stats_spec())
        for name, fn, n in (("held_tau", lambda: ctx.gibbs_update_held_tau(a.iters, n_held), a.iters),
                            ("gibbs_update", lambda: ctx.gibbs_update(a.iters), a.iters),
                            ("fixed_tau_pool0", lambda: ctx.gibbs_update_fixed_tau(a.iters, pool=0), a.iters),
                            ("sweep_held", lambda: sweeps(lambda: ctx.sample_tau_held(n_held)), a.sweeps),
                            ("sweep_full", lambda: sweeps(ctx.sample_tau), a.sweeps)):
            start()
            ms, every = timed(fn, a.reps)
            row[name] = dict(event_ms_median=ms, event_ms_all=every, us_per_unit=1e3 * ms / n)
            print("G=%d n_held=%d %-16s %8.3f ms / %d = %7.2f us" % (G, n_held, name, ms, n, 1e3 * ms / n), flush=True)
        rows.append(row)
        ctx.close()
    out = dict(what="dsm_ctx_gibbs_update_held_tau against dsm_ctx_gibbs_update and dsm_ctx_gibbs_update_fixed_tau(pool = 0), us per iteration; "
                    "dsm_ctx_sample_tau_held against dsm_ctx_sample_tau, us per call; same table, same process",
               device=torch.cuda.get_device_name(0),
               timing="HIP events around the call(s), one warm-up call, median of reps; the single-sweep calls each drain their stream",
               not_measured=["the held sweep kernel in isolation by kernel trace", "G > 12", "over-fitted free haplotypes (near-ties)",
                             "a target: there is none"],
               cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
