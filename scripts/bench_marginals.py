#!/usr/bin/env python3
"""Cost of the device pass behind `desman --marginals` (dsm_ctx_trace_rb_marginals, L = floor(sqrt(n))) on the traces of n = 200 stored
iterations of a chain started at the generating state, at V = 10 000, S = 64, G = 8 and V = 1000, S = 16, G = 5, next to the n
iterations of dsm_ctx_gibbs_update that wrote those traces, in the same process: the yardstick -- the pass evaluates the 4 G candidates
of a position in plain fp64 where the sweep screens most of them in fp32.  Timing: HIP events around the whole call (it launches on the
context's stream and returns with that stream drained, so a sample holds the scratch allocations, the one kernel and the result
copies), after a warm-up call, median of --reps.  At the large table the chain then runs 500 iterations and the script reports what the
feature buys: the median, over the cells whose Tau_MCSE is not zero, of Tau_rb_MCSE / Tau_MCSE (both by batch means, L = 22) -- and the
same for a copy of that table at 2 % of its depth after a burn-in of 500, because the table itself is so deep that nothing flips.  Not
measured: the kernel alone (no profiler run), S > 64 (the instantiations with two and more samples per lane of a 64-lane group), the
host-side numpy of desman_amd/marginals.py.

    python scripts/bench_marginals.py [--reps 7] [--out profiles/marginals_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(10000, 64, 8, 200), (1000, 16, 5, 200)]
N_LONG = 500
THIN = 0.02                 # the depth of the thinned copy of the large table, as a share of its own


def _timed(fn, reps):
    import torch
    fn()                                                                     # warm-up
    ms, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        ms.append(e0.elapsed_time(e1))
    return dict(event_ms_median=float(np.median(ms)), event_ms_all=[float(x) for x in ms], wall_ms_median=float(np.median(wall)) * 1e3)


def _mcse_ratio(ctx):
    """N_LONG more iterations of the chain, then both Monte Carlo standard errors by batch means (L = floor(sqrt(N_LONG))) and the
    median of their ratio over the cells whose Tau_MCSE is not zero"""
    from desman_amd import diagnose, marginals
    ctx.gibbs_update(N_LONG)
    L = diagnose.default_batch_len(N_LONG)
    plain = diagnose.tau_diagnostics(ctx.trace_batch_stats(L, want=("sum", "bsq")))
    rb = marginals.rb_marginals(ctx.trace_rb_marginals(L))
    moved = plain["mcse"] > 0
    ratio = rb["mcse"][moved] / plain["mcse"][moved]
    cells = marginals.calls(rb["p"], ctx.get_star()["tau"])
    return dict(L=L, n_used=rb["N"], cells=int(moved.size), cells_with_nonzero_Tau_MCSE=int(moved.sum()),
                median_rb_mcse_over_mcse=float(np.median(ratio)) if moved.any() else None,
                quartiles_rb_mcse_over_mcse=[float(x) for x in np.percentile(ratio, (25, 75))] if moved.any() else None,
                cells_Tau_MCSE_zero_but_rb_MCSE_not=int(((plain["mcse"] == 0) & (rb["mcse"] > 0)).sum()),
                max_abs_mean_difference=float(np.abs(rb["p"] - plain["p"]).max()), summary=marginals.summary(cells, rb["dead"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from desman_amd import _lib, diagnose, marginals
    from desman_amd.synth import synth_counts
    rows = []
    for k, (V, S, G, n) in enumerate(CASES):
        counts, tau_true, gamma_true = synth_counts(V, S, G, seed=V + S)
        eta = 0.96 * np.eye(4) + 0.01
        onehot = np.zeros((V, G, 4), dtype=np.int64)
        np.put_along_axis(onehot, tau_true.astype(np.int64)[..., None], 1, axis=2)
        ctx = _lib.Context(0)
        ctx.set_counts(counts)
        ctx.set_state(onehot, gamma_true, eta)
        ctx.seed(11, ctr_seed=12345)
        L = diagnose.default_batch_len(n)
        row = dict(V=V, S=S, G=G, n=n, L=L, tiling=list(_lib.rbtau_debug_path(S, G)))
        # the yardstick first (it writes the traces): n Gibbs iterations from the generating state
        row["gibbs_update"] = _timed(lambda: ctx.gibbs_update(n), min(a.reps, 3))
        r = _timed(lambda: ctx.trace_rb_marginals(L), a.reps)
        used = ctx.trace_rb_marginals(L)
        assert np.isfinite(used["sum"]).all() and np.isfinite(used["bsq"]).all()
        r["n_used"] = used["N"]
        r["ms_per_used_iteration"] = r["event_ms_median"] / used["N"]
        row["trace_rb_marginals"] = r
        row["dead"] = used["dead"]
        row["gibbs_ms_per_iteration"] = row["gibbs_update"]["event_ms_median"] / n
        row["ratio_to_one_gibbs_iteration"] = r["ms_per_used_iteration"] / row["gibbs_ms_per_iteration"]
        if k == 0:
            row["after_%d_iterations" % N_LONG] = _mcse_ratio(ctx)
        ctx.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    # the large table is so deep that no base of it flips in 500 iterations (every Tau_MCSE is 0): the same table at 2 % of its depth,
    # where cells do move, says what the feature buys where there is something to buy
    V, S, G, _ = CASES[0]
    counts, tau_true, gamma_true = synth_counts(V, S, G, seed=V + S, depth_scale=THIN)
    onehot = np.zeros((V, G, 4), dtype=np.int64)
    np.put_along_axis(onehot, tau_true.astype(np.int64)[..., None], 1, axis=2)
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    ctx.set_state(onehot, gamma_true, 0.96 * np.eye(4) + 0.01)
    ctx.seed(11, ctr_seed=12345)
    ctx.gibbs_update(N_LONG)                                                 # burn-in from the generating state
    row = dict(V=V, S=S, G=G, depth_scale=THIN)
    row["after_%d_more_iterations" % N_LONG] = _mcse_ratio(ctx)
    ctx.close()
    rows.append(row)
    print(json.dumps(row), flush=True)
    out = dict(command="python scripts/bench_marginals.py --reps %d" % a.reps, device=torch.cuda.get_device_name(0),
               timing="HIP events around the whole call (scratch allocations, the kernel, result copies), warm-up call, median of reps "
                      "(gibbs_update: at most 3 reps)",
               not_measured="the kernel alone, S > 64, the numpy of desman_amd/marginals.py",
               cases=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
