#!/usr/bin/env python3
"""Cost of the device pass behind `desman --predictive` (dsm_ctx_trace_predictive) at N = 1000 positions, S = 64, G = 6 and G = 8 with
n_used = 50 stored iterations, next to what the library could already do for the same numbers: a Python loop of n_used
Context.assign_tau calls on the same resident table, one per stored (gamma_t, eta_t).  The new call evaluates the same
n_used N 4^G states and leaves out the marginals, the arg-max, the per-call uploads, allocations and result copies and the rebuilding
of each position's cell list, so it should not be slower; the ratio loop / call is recorded either way.  Timing: HIP events around the
whole call resp. the whole loop (scratch allocations, kernels, result copies included), after a warm-up, median of --reps.  Not
measured: the kernel alone (no profiler run), other shapes, the host-side numpy of desman_amd/predictive.py.

    python scripts/bench_predictive.py [--reps 7] [--out profiles/predictive_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(1000, 64, 6, 50), (1000, 64, 8, 50)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from desman_amd import _lib
    from desman_amd.synth import synth_counts
    rows = []
    for (N, S, G, n) in CASES:
        rs = np.random.RandomState(N + G)
        counts, tau_true, gamma_true = synth_counts(N, S, G, seed=N + S, depth_scale=0.1)
        eta = 0.96 * np.eye(4) + 0.01
        onehot = np.zeros((N, G, 4), dtype=np.int64)
        np.put_along_axis(onehot, tau_true.astype(np.int64)[..., None], 1, axis=2)
        ctx = _lib.Context(0)
        ctx.set_counts(counts)
        ctx.set_state(onehot, gamma_true, eta)
        ctx.debug_set_trace(np.broadcast_to(tau_true.astype(np.int64), (n, N, G)).copy())
        gam = gamma_true[None] * rs.uniform(0.95, 1.05, size=(n, S, G))
        gam /= gam.sum(axis=2, keepdims=True)
        etas = np.ascontiguousarray(np.broadcast_to(eta, (n, 4, 4)))
        ctx.debug_set_param_trace(gam, etas)
        states = float(n) * N * 4.0 ** G
        row = dict(N=N, S=S, G=G, n_used=n, states=states, nonzero_cells_per_position=float((counts > 0).sum()) / N)

        def loop():
            return np.stack([ctx.assign_tau(gam[t], etas[t])["logz"] for t in range(n)])
        row["trace_predictive"] = _timed(lambda: ctx.trace_predictive(), a.reps)
        row["assign_tau_loop"] = _timed(loop, a.reps)
        for k in ("trace_predictive", "assign_tau_loop"):
            row[k]["states_per_s"] = states / (row[k]["event_ms_median"] * 1e-3)
        row["ratio_loop_over_call"] = row["assign_tau_loop"]["event_ms_median"] / row["trace_predictive"]["event_ms_median"]
        got = ctx.trace_predictive(want=("logz_it",))["logz_it"]
        row["logz_bits_equal_to_assign_tau"] = bool(got.tobytes() == loop().tobytes())
        assert np.isfinite(got).all()
        ctx.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(command="python scripts/bench_predictive.py --reps %d" % a.reps, device=torch.cuda.get_device_name(0),
               timing="HIP events around the whole call / the whole loop of n_used Context.assign_tau calls (allocations, uploads, kernels, "
                      "result copies), warm-up, median of reps",
               not_measured="the kernel alone, other shapes, the numpy of desman_amd/predictive.py", cases=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
