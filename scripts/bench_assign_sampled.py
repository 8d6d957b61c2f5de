#!/usr/bin/env python3
"""Time of the sampled joint assignment (dsm_ctx_assign_tau_sampled) at the command line's defaults (B = 20, T = 100) on the synthetic
generator, N = 10 000, S = 64, G in {6, 8, 10, 12, 16}, and -- in the same process -- of the exact call (dsm_ctx_assign_tau) at the
shapes of scripts/bench_assign.py (N = 10 000 at G = 6 and 8, N = 1 000 at G = 10), with their ratio per position.  Timing as in
scripts/bench_assign.py: HIP events on the default stream around the context form (counts resident: a sample holds the launch, the
parameter upload and the result copies), after a warm-up call, median of --reps.  With --pairs E every sampled shape is timed twice in
the same run, without pair moves and with a pair pass after every E-th sweep (dsm_ctx_assign_tau_sampled_pairs); the row then holds
both times, their ratio and the ratio the arithmetic predicts, 1 + 2 (G - 1) / E.

    python scripts/bench_assign_sampled.py [--reps 7] [--pairs E] [--out profiles/assign_sampled_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SAMPLED, S = 10000, 64
SAMPLED_G = (6, 8, 10, 12, 16)
EXACT = ((10000, 6), (10000, 8), (1000, 10))       # (N, G) of DESIGN.md sec. 8a


def timed(call, reps):
    """median and all HIP-event times (ms) of call() after one warm-up, and the last result"""
    import torch
    res = call()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        res = call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(float(e0.elapsed_time(e1)))
    return float(np.median(ms)), ms, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--burn", type=int, default=None)
    ap.add_argument("--kept", type=int, default=None)
    ap.add_argument("--pairs", type=int, default=0, metavar="E", help="also time the call with a pair pass after every E-th sweep")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from desman_amd import _lib
    from desman_amd.synth import synth_counts
    B = _lib.SAMPLED_BURN if a.burn is None else a.burn
    T = _lib.SAMPLED_KEPT if a.kept is None else a.kept
    eta = 0.96 * np.eye(4) + 0.01
    exact_ms = {}
    rows = []
    for (N, G) in EXACT:
        counts, _, gamma = synth_counts(N, S, G, seed=100 + G)
        gamma = np.ascontiguousarray(gamma)
        ctx = _lib.Context(0)
        ctx.set_counts(counts)
        med, ms, _ = timed(lambda: ctx.assign_tau(gamma, eta), a.reps)
        ctx.close()
        exact_ms[G] = med / N
        rows.append(dict(form="exact", N=N, S=S, G=G, event_ms_median=med, event_ms_all=ms, ms_per_position=med / N, positions_per_s=N / (med * 1e-3)))
        print(json.dumps(rows[-1]), flush=True)
    for G in SAMPLED_G:
        counts, _, gamma = synth_counts(N_SAMPLED, S, G, seed=100 + G)
        gamma = np.ascontiguousarray(gamma)
        ctx = _lib.Context(0)
        ctx.set_counts(counts)
        med, ms, res = timed(lambda: ctx.assign_tau_sampled(gamma, eta, seed=1, burn=B, kept=T), a.reps)
        if a.pairs > 0:
            pmed, pms, pres = timed(lambda: ctx.assign_tau_sampled(gamma, eta, seed=1, burn=B, kept=T, pair_every=a.pairs), a.reps)
        ctx.close()
        row = dict(form="sampled", N=N_SAMPLED, S=S, G=G, burn=B, kept=T, event_ms_median=med, event_ms_all=ms,
                   ms_per_position=med / N_SAMPLED, positions_per_s=N_SAMPLED / (med * 1e-3),
                   sweeps_positions_per_s=N_SAMPLED * 4 * (B + T) / (med * 1e-3),
                   fp64_logs_per_s=float((counts > 0).sum()) * 4 * 4 * (B + T) * G / (med * 1e-3),
                   share_spread_above_01=float((res["spread"] > 0.1).mean()), path=_lib.assign_sampled_debug_path(S, G))
        if a.pairs > 0:
            row.update(pair_every=a.pairs, pairs_event_ms_median=pmed, pairs_event_ms_all=pms, pairs_over_plain=pmed / med,
                       pairs_over_plain_by_arithmetic=1.0 + 2.0 * (G - 1) / a.pairs, plain_spread_of_reps=(max(ms) - min(ms)) / med,
                       pairs_share_spread_above_01=float((pres["spread"] > 0.1).mean()))
        if G in exact_ms:
            row["exact_over_sampled_per_position"] = exact_ms[G] / row["ms_per_position"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        out = dict(command="python scripts/bench_assign_sampled.py --reps %d%s" % (a.reps, " --pairs %d" % a.pairs if a.pairs > 0 else ""), device=torch.cuda.get_device_name(0),
                   timing="HIP events around the context forms (counts resident), warm-up call, median of reps", cases=rows)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
