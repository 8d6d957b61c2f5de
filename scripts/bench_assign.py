#!/usr/bin/env python3
"""Throughput of the exact joint assignment (dsm_ctx_assign_tau) on the synthetic generator: positions/s, states/s and the
achieved fp64-log rate (logarithms actually issued = non-zero count cells x states) at N = 10 000, S = 64, G in {4, 6, 8} and
N = 1 000, G = 10.  Timing: HIP events on the default stream (the library's launches of this call run there) around the
context form, which has the counts resident -- so a sample holds the three launches, the parameter upload and the result
copies, not the count upload; after a warm-up call, median of --reps.  The CPU comparator is the numpy restatement of
tests/test_assign_cpu.py on one core at a size it finishes.

    python scripts/bench_assign.py [--reps 7] [--out profiles/assign_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [(10000, 64, 4), (10000, 64, 6), (10000, 64, 8), (1000, 64, 10)]
# the tau sweep's own rate (profiles/r06_kernel_stats.csv): 8.2e7 logarithms in 34 us, most of them screened in fp32
SWEEP_LOGS_PER_S = 8.2e7 / 34e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--draw", action="store_true", help="time the call with the posterior draw as well")
    a = ap.parse_args()
    import torch
    from desman_amd import _lib
    from desman_amd.synth import synth_counts
    rows = []
    for (N, S, G) in CASES:
        counts, _, gamma = synth_counts(N, S, G, seed=100 + G)
        gamma = np.ascontiguousarray(gamma)
        eta = 0.96 * np.eye(4) + 0.01
        ctx = _lib.Context(0)
        ctx.set_counts(counts)
        seed = 1 if a.draw else None
        ctx.assign_tau(gamma, eta, seed=seed)                                # warm-up
        ms, wall = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            res = ctx.assign_tau(gamma, eta, seed=seed)
            e1.record()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            ms.append(e0.elapsed_time(e1))
        ctx.close()
        t = float(np.median(ms)) * 1e-3
        nz = int((counts > 0).sum())
        logs = float(nz) * 4.0 ** G
        rows.append(dict(N=N, S=S, G=G, states_per_position=4 ** G, nonzero_cells=nz, zero_fraction=float((counts == 0).mean()),
                         event_ms_median=t * 1e3, event_ms_all=[float(x) for x in ms], wall_ms_median=float(np.median(wall)) * 1e3,
                         positions_per_s=N / t, states_per_s=N * 4.0 ** G / t, fp64_logs_per_s=logs / t,
                         share_conf_below_099=float((res["conf"] < 0.99).mean())))
        print(json.dumps(rows[-1]), flush=True)
    # CPU comparator: the numpy restatement, one core, a size it finishes
    from test_assign_cpu import assign_numpy
    Nc, Sc, Gc = 200, 64, 6
    counts, _, gamma = synth_counts(Nc, Sc, Gc, seed=100 + Gc)
    t0 = time.perf_counter()
    assign_numpy(counts, np.ascontiguousarray(gamma), 0.96 * np.eye(4) + 0.01)
    tc = time.perf_counter() - t0
    cpu = dict(what="numpy restatement (tests/test_assign_cpu.py: assign_numpy), one process, BLAS threads as the environment sets them",
               N=Nc, S=Sc, G=Gc, seconds=tc, states_per_s=Nc * 4.0 ** Gc / tc)
    out = dict(command="python scripts/bench_assign.py --reps %d%s" % (a.reps, " --draw" if a.draw else ""), device=torch.cuda.get_device_name(0),
               timing="HIP events around Context.assign_tau (counts resident), warm-up call, median of reps", cases=rows, cpu=cpu,
               tau_sweep_logs_per_s=SWEEP_LOGS_PER_S)
    print(json.dumps(dict(cpu=cpu)))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
