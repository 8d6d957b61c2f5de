#!/usr/bin/env python3
"""Cost of the device pass behind `desman --check --check-reps` (dsm_ctx_trace_ppc) at R = 20 replicates over 50 used iterations, on
planted traces near one state at V = 10 000, S = 64, G = 8 and V = 1000, S = 16, G = 5, next to two yardsticks in the same process:
dsm_ctx_trace_fit_stats over the same 50 iterations, and one Gibbs iteration of the same table (the mean of 50).  Timing: HIP events
around the whole call (scratch allocations, every launch, result copies), after one warm-up call, median of --reps.  Not measured: the
kernel alone (no profiler run), other R or iteration counts, S > 64 (the instantiations with two and more samples per lane), the
host-side numpy of desman_amd/check.py.

    python scripts/bench_check_reps.py [--reps 7] [--out profiles/check_reps_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_check import _timed  # noqa: E402

CASES = [(10000, 64, 8), (1000, 16, 5)]
N_USED, R = 50, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from desman_amd import _lib
    from desman_amd.synth import synth_counts
    rows = []
    for (V, S, G) in CASES:
        n = N_USED
        rs = np.random.RandomState(V + G)
        counts, tau_true, gamma_true = synth_counts(V, S, G, seed=V + S)
        eta = 0.96 * np.eye(4) + 0.01
        base = tau_true.astype(np.int64)
        onehot = np.zeros((V, G, 4), dtype=np.int64)
        np.put_along_axis(onehot, base[..., None], 1, axis=2)
        ctx = _lib.Context(0)
        ctx.set_counts(counts)
        ctx.set_state(onehot, gamma_true, eta)
        ctx.seed(11, ctr_seed=12345)
        N = counts.sum(axis=2)
        row = dict(V=V, S=S, G=G, n_used=n, R=R, cell_draws=float((N > 0).sum()) * n * R, mean_reads_per_cell=float(N.mean()))
        # the yardstick first (it writes the traces): n Gibbs iterations from the generating state
        g = _timed(lambda: ctx.gibbs_update(n), a.reps)
        row["gibbs_iteration"] = dict(event_ms_median=g["event_ms_median"] / n, event_ms_all=[x / n for x in g["event_ms_all"]])
        trace = np.broadcast_to(base, (n, V, G)).copy()                      # a chain near its MAP state: 2 % of the cells moved per iteration
        cells = rs.randint(0, trace.size, size=trace.size // 50)
        flat = trace.reshape(-1)
        flat[cells] = (flat[cells] + rs.randint(1, 4, size=cells.size)) % 4
        ctx.debug_set_trace(trace)
        gam = gamma_true[None] * rs.uniform(0.95, 1.05, size=(n, S, G))
        gam /= gam.sum(axis=2, keepdims=True)
        ctx.debug_set_param_trace(gam, np.broadcast_to(eta, (n, 4, 4)))
        row["path"] = ctx.ppc_debug_path(n, R)
        row["share_of_cells_read_by_read"] = float((N[N > 0] <= row["path"]["C"]).mean())
        row["trace_fit_stats"] = _timed(lambda: ctx.trace_fit_stats(want=("sample", "position")), a.reps)
        row["trace_ppc"] = _timed(lambda: ctx.trace_ppc(R), a.reps)
        ms = row["trace_ppc"]["event_ms_median"]
        row["trace_ppc"]["cell_draws_per_s"] = row["cell_draws"] / (ms * 1e-3)
        row["ms_per_iteration_replicate"] = ms / (n * R)
        row["ratio_to_fit_stats_per_iteration_replicate"] = ms / (n * R) / (row["trace_fit_stats"]["event_ms_median"] / n)
        row["ratio_to_gibbs_iteration_per_iteration_replicate"] = ms / (n * R) / row["gibbs_iteration"]["event_ms_median"]
        got = ctx.trace_ppc(R)
        assert np.isfinite(got["rep_sample"]).all() and np.isfinite(got["rep_position"]).all()
        ctx.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(command="python scripts/bench_check_reps.py --reps %d" % a.reps, device=torch.cuda.get_device_name(0),
               timing="HIP events around the whole call (scratch allocations, every launch, result copies), one warm-up call, median of "
                      "reps; gibbs_iteration: a call of 50 iterations divided by 50",
               not_measured="the kernel alone, other R and iteration counts, S > 64, the numpy of desman_amd/check.py",
               cases=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
