#!/usr/bin/env python3
"""Cost of the device pass behind `desman --marginal-pairs` (dsm_ctx_trace_rb_pairs, L = floor(sqrt(n))) on the traces of n = 40 stored
iterations of a chain started at the generating state, at V = 10 000, S = 64, G = 8 and V = 1000, S = 16, G = 5, per used iteration,
next to one pair pass of the chain (dsm_ctx_sample_tau_pairs) on the same resident table in the same process: the yardstick -- it forms
the same sixteen totals per position and pair, plus a draw, minus the accumulation.  Timing: HIP events around the whole call (it
launches on the context's stream and returns with that stream drained, so a sample of the reduction holds the scratch allocations, the
launches and the result copies -- joint is V P 128 bytes; the events lie on the default stream, not on the context's, so the interval is
in effect the host time of the blocking call bracketed by events, and wall_ms_median next to it is the check), after a warm-up call,
median of --reps.  The reduction is timed three times:
both outputs, same_batch alone (no joint traffic and no copy of it), joint alone.  Not measured: the kernel alone (no profiler run),
S > 64, G > 8, the host-side numpy of desman_amd/marginals.py.

    python scripts/bench_marginal_pairs.py [--reps 7] [--out profiles/marginal_pairs_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(10000, 64, 8, 40), (1000, 16, 5, 40)]


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
    from desman_amd import _lib, diagnose
    from desman_amd.synth import synth_counts
    rows = []
    for V, S, G, n in CASES:
        counts, tau_true, gamma_true = synth_counts(V, S, G, seed=V + S)
        eta = 0.96 * np.eye(4) + 0.01
        onehot = np.zeros((V, G, 4), dtype=np.int64)
        np.put_along_axis(onehot, tau_true.astype(np.int64)[..., None], 1, axis=2)
        ctx = _lib.Context(0)
        ctx.set_counts(counts)
        ctx.set_state(onehot, gamma_true, eta)
        ctx.seed(11, ctr_seed=12345)
        ctx.gibbs_update(n)                                                  # writes the traces the reduction reads
        L = diagnose.default_batch_len(n)
        row = dict(V=V, S=S, G=G, P=G * (G - 1) // 2, n=n, L=L, tiling=list(_lib.rbpair_debug_path(S, G)))
        used = ctx.trace_rb_pairs(L)
        assert np.isfinite(used["joint"]).all() and np.isfinite(used["same_batch"]).all()
        row["n_used"], row["dead"] = used["N"], used["dead"]
        for name, want in (("both", ("joint", "same_batch")), ("same_batch_only", ("same_batch",)), ("joint_only", ("joint",))):
            r = _timed(lambda: ctx.trace_rb_pairs(L, want=want), a.reps)
            r["ms_per_used_iteration"] = r["event_ms_median"] / used["N"]
            row["trace_rb_pairs_" + name] = r
        it = [1000]

        def pair_pass():
            it[0] += 1
            ctx.sample_tau_pairs(it[0])
        row["sample_tau_pairs"] = _timed(pair_pass, a.reps)                  # the yardstick last: it moves the resident tau
        one = row["sample_tau_pairs"]["event_ms_median"]
        row["ratio_to_one_pair_pass"] = {k: row["trace_rb_pairs_" + k]["ms_per_used_iteration"] / one for k in ("both", "same_batch_only", "joint_only")}
        ctx.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(command="python scripts/bench_marginal_pairs.py --reps %d" % a.reps, device=torch.cuda.get_device_name(0),
               timing="HIP events on the default stream around the whole blocking call (scratch allocations, the launches on the "
                      "context's own stream, result copies): in effect host time bracketed by events; warm-up call, median of reps",
               not_measured="the kernel alone, S > 64, G > 8, the numpy of desman_amd/marginals.py",
               cases=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
