#!/usr/bin/env python3
"""Cost of the trace reduction behind `desman --diagnose` (dsm_ctx_trace_batch_stats, L = floor(sqrt(n))) on planted traces of n = 500
stored iterations near one state at V = 10 000, G = 8 and V = 50 000, G = 12, next to dsm_ctx_get_tau_sum_perm at the same shapes in
the same process: the yardstick, a call of the parent commit that reads the same trace with the same mapping.  Timing: HIP events around
the whole call (it launches on the context's stream and returns with that stream drained, so a sample holds the outputs' memsets, the
kernel, the result copies and the scratch allocations of the call), after a warm-up call, median of --reps.  Not measured: the kernel
alone (no profiler run), other batch lengths, relabelled (non-identity) rows, the host-side numpy of desman_amd/diagnose.py.

    python scripts/bench_diagnose.py [--reps 7] [--out profiles/diagnose_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(10000, 8, 500), (50000, 12, 500)]


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
    from desman_amd.synth import random_state
    rows = []
    for (V, G, n) in CASES:
        rs = np.random.RandomState(V + G)
        S = 2
        ctx = _lib.Context(0)
        ctx.set_counts(rs.randint(0, 30, size=(V, S, 4)).astype(np.int64))
        tau, gamma, eta = random_state(V, S, G, seed=1)
        ctx.set_state(tau, gamma, eta)
        base = np.argmax(tau, axis=2)
        trace = np.broadcast_to(base, (n, V, G)).copy()                      # a chain near its MAP state: 2 % of the cells moved per iteration
        cells = rs.randint(0, trace.size, size=trace.size // 50)
        flat = trace.reshape(-1)
        flat[cells] = (flat[cells] + rs.randint(1, 4, size=cells.size)) % 4
        del cells
        ctx.debug_set_trace(trace)
        del trace
        L = diagnose.default_batch_len(n)
        B, N, skip = diagnose.batch_range(n, L)
        ident = np.tile(np.arange(G, dtype=np.uint8), (n, 1))
        row = dict(V=V, G=G, n=n, L=L, B=B, N=N, trace_bytes=8.0 * n * V,
                   result_bytes=dict(trace_batch_stats=(3 * 32 + 4) * V * G, tau_sum_perm=32 * V * G))
        for name, fn in (("tau_sum_perm", lambda: ctx.get_tau_sum_perm(ident)), ("trace_batch_stats", lambda: ctx.trace_batch_stats(L)),
                         ("trace_batch_stats_sum_only", lambda: ctx.trace_batch_stats(L, want=("sum",)))):
            row[name] = _timed(fn, a.reps)
        row["ratio_to_tau_sum_perm"] = row["trace_batch_stats"]["event_ms_median"] / row["tau_sum_perm"]["event_ms_median"]
        assert np.array_equal(ctx.trace_batch_stats(L, want=("sum",))["sum"], ctx.get_tau_sum_perm(ident[skip:], it0=skip))
        ctx.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(command="python scripts/bench_diagnose.py --reps %d" % a.reps, device=torch.cuda.get_device_name(0),
               timing="HIP events around the whole call (memsets, kernel, result copies, scratch allocations), warm-up call, median of reps",
               not_measured="the kernel alone, other batch lengths, non-identity perm rows, the numpy of desman_amd/diagnose.py",
               cases=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
