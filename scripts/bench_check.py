#!/usr/bin/env python3
"""Cost of the device pass behind `desman --check` (dsm_ctx_trace_fit_stats) on planted traces of n = 500 stored iterations near one
state at V = 10 000, S = 64, G = 8 and V = 50 000, S = 96, G = 12, once with all three outputs and once with `sample` and `position`
only, next to n iterations of dsm_ctx_gibbs_update at the same shape in the same process: the yardstick -- the pass evaluates one
mixture per cell and iteration where the sweep evaluates 4 G candidates.  Timing: HIP events around the whole call (it launches on the
context's stream and returns with that stream drained, so a sample holds the scratch allocations, the three or four kernels and the
result copies), after a warm-up call, median of --reps.  Not measured: the kernel alone (no profiler run), other iteration counts,
S > 128 (the instantiations with four and eight samples per lane), the host-side numpy of desman_amd/check.py.

    python scripts/bench_check.py [--reps 7] [--out profiles/check_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(10000, 64, 8, 500), (50000, 96, 12, 500)]


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
    for (V, S, G, n) in CASES:
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
        row = dict(V=V, S=S, G=G, n=n, cell_iterations=float(V) * S * n)
        # the yardstick first (it writes the traces): n Gibbs iterations from the generating state
        row["gibbs_update"] = _timed(lambda: ctx.gibbs_update(n), min(a.reps, 3))
        trace = np.broadcast_to(base, (n, V, G)).copy()                      # a chain near its MAP state: 2 % of the cells moved per iteration
        cells = rs.randint(0, trace.size, size=trace.size // 50)
        flat = trace.reshape(-1)
        flat[cells] = (flat[cells] + rs.randint(1, 4, size=cells.size)) % 4
        del cells
        ctx.debug_set_trace(trace)
        del trace
        gam = gamma_true[None] * rs.uniform(0.95, 1.05, size=(n, S, G))
        gam /= gam.sum(axis=2, keepdims=True)
        ctx.debug_set_param_trace(gam, np.broadcast_to(eta, (n, 4, 4)))
        row["path"] = ctx.fit_debug_path()
        for name, want in (("all_outputs", ("sample", "position", "cell")), ("sample_position", ("sample", "position"))):
            r = _timed(lambda: ctx.trace_fit_stats(want=want), a.reps)
            r["cell_iterations_per_s"] = row["cell_iterations"] / (r["event_ms_median"] * 1e-3)
            row[name] = r
        row["ratio_to_gibbs_update"] = row["all_outputs"]["event_ms_median"] / row["gibbs_update"]["event_ms_median"]
        full = ctx.trace_fit_stats()
        assert np.isfinite(full["sample"]).all() and np.isfinite(full["position"]).all()
        row["mean_X_over_E"] = float(full["sample"][:, 0].sum() / full["sample"][:, 2].sum())
        ctx.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(command="python scripts/bench_check.py --reps %d" % a.reps, device=torch.cuda.get_device_name(0),
               timing="HIP events around the whole call (scratch allocations, kernels, result copies), warm-up call, median of reps "
                      "(gibbs_update: at most 3 reps)",
               not_measured="the kernel alone, other iteration counts, S > 128, the numpy of desman_amd/check.py",
               cases=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
