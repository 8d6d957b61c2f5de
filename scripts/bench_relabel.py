#!/usr/bin/env python3
"""Cost of the trace reductions behind `desman --relabel` (dsm_ctx_trace_snd in its STAR and SELF modes, dsm_ctx_get_tau_sum_perm) on
planted traces of n = 500 stored iterations at V = 10 000, G = 8 and V = 50 000, G = 12, next to what the same numbers cost through
the host today: get_tau_at (one [V][G][4] int64 tensor per iteration) plus the numpy compSND, timed for 5 iterations and scaled to
n -- an extrapolation, stated as such.  Timing: HIP events around the call (it launches on the context's stream and returns with that
stream drained, so a sample holds the output's memset, the kernel, the result copy and the scratch allocations of the call), after a
warm-up call, median of --reps.  The trace is read once per call: 8 n V bytes.

    python scripts/bench_relabel.py [--reps 7] [--out profiles/relabel_bench.json]
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
HBM_BYTES_PER_S = 8.0e12            # MI355X peak


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
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
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
        trace_bytes = 8.0 * n * V
        row = dict(V=V, G=G, n=n, trace_bytes=trace_bytes)
        ident = np.tile(np.arange(G, dtype=np.uint8), (n, 1))
        for name, fn in (("snd_star", lambda: ctx.trace_snd(_lib.SND_STAR)), ("snd_self", lambda: ctx.trace_snd(_lib.SND_SELF)),
                         ("tau_sum_perm", lambda: ctx.get_tau_sum_perm(ident))):
            r = _timed(fn, a.reps)
            r["trace_bytes_per_s"] = trace_bytes / (r["event_ms_median"] * 1e-3)
            r["share_of_hbm_peak"] = r["trace_bytes_per_s"] / HBM_BYTES_PER_S
            row[name] = r
        # the host path: what a caller has to do without these calls
        smp = HaploSNP_Sampler.__new__(HaploSNP_Sampler)
        star = ctx.get_star()["tau"]
        k = 5
        t0 = time.perf_counter()
        for it in range(k):
            smp.compSND(ctx.get_tau_at(it), star)
        th = time.perf_counter() - t0
        row["host_path"] = dict(what="get_tau_at + numpy compSND against tau_star, %d iterations timed, scaled to n (extrapolated)" % k,
                                seconds_measured=th, iterations_measured=k, seconds_extrapolated_n=th * n / k,
                                bytes_through_host_n=8.0 * 4 * V * G * n)
        assert np.array_equal(ctx.trace_snd(_lib.SND_STAR, it0=0, n_it=1)[0], smp.compSND(ctx.get_tau_at(0), star))
        ctx.close()
        del trace
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(command="python scripts/bench_relabel.py --reps %d" % a.reps, device=torch.cuda.get_device_name(0),
               timing="HIP events around the whole call (memset, kernel, result copy, scratch allocations), warm-up call, median of reps",
               hbm_peak_bytes_per_s=HBM_BYTES_PER_S, cases=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
