#!/usr/bin/env python3
"""Throughput of the abundance fit (dsm_ctx_fit_gamma) on the synthetic generator: V = 10 000, G = 8 with 1 / 8 / 64 samples, with
and without the presence fits, and V = 50 000, G = 12 with 64 samples.  Every case runs a FIXED number of EM steps (tol = 0), so
that time per step and fit is a plain quotient; the default stop test is timed once per shape as well, with the step counts it
took.  Timing: HIP events on the default stream (the library's launches of this call run there) around the context form, which has
the counts resident -- a sample holds the call's scratch allocations and frees (dsm_ctx_fit_gamma keeps none between calls), the
repack launch, the EM launch, the parameter upload and the synchronous result copies, not the count upload; after a warm-up call,
median of --reps.  One more leg per shape times the profile-likelihood intervals (dsm_ctx_fit_gamma_interval) of the default fit's
abundances with a fixed --interval-steps EM steps per inner fit (tol = 0) and the default ctol; the number of inner fits is that of
the bisections and is recorded from the bracket widths.  A last leg per shape times the joint fit of the abundances and the error
matrix (dsm_ctx_fit_gamma_eta) at the same fixed --steps (tol = 0): a step is a pair of launches there, the timing holds the
reference fit with eta held fixed (loglik0) that the call makes as well.  --legs picks the legs to run.  With one sample and no presence fits that fixed cost is a visible part of the total.  The CPU comparator is the numpy restatement of tests/_abund_ref.py at one small shape.

    python scripts/bench_abund.py [--reps 7] [--steps 200] [--interval-steps 20] [--legs fit,interval,eta] [--out profiles/abund_bench.json]
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

CASES = [(10000, 8, 1), (10000, 8, 8), (10000, 8, 64), (50000, 12, 64)]          # V, G, S_new


def timed(fn, reps):
    import torch
    fn()                                                                 # warm-up
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [float(x) for x in ms], res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200, help="EM steps of the fixed-length runs")
    ap.add_argument("--interval-steps", type=int, default=20, help="EM steps of every inner fit of the interval leg")
    ap.add_argument("--legs", default="fit,interval,eta", help="comma-separated: fit, interval (needs fit), eta")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "abund_bench.json"))
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    import torch
    from desman_amd import _lib
    from desman_amd.synth import synth_counts
    rows = []
    eta = 0.96 * np.eye(4) + 0.01
    for (V, G, S) in CASES:
        counts, tau, _ = synth_counts(V, S, G, seed=100 + G)
        tau = np.ascontiguousarray(tau, dtype=np.int64)
        ctx = _lib.Context(0)
        ctx.set_counts(counts)
        for presence in ((False, True) if V == 10000 else (True,)) if "fit" in legs else ():
            fits = S * (1 + G) if presence else S
            ms, every, _ = timed(lambda: ctx.fit_gamma(eta, tau=tau, max_iter=a.steps, tol=0.0, presence=presence), a.reps)
            rows.append(dict(V=V, G=G, S_new=S, presence=presence, fits=fits, steps=a.steps, passes=a.steps + 2, event_ms_median=ms, event_ms_all=every,
                             us_per_step=ms * 1e3 / a.steps, us_per_step_and_fit=ms * 1e3 / a.steps / fits,
                             position_steps_per_s=float(V) * fits * a.steps / (ms * 1e-3)))
            print(json.dumps(rows[-1]), flush=True)
        if "eta" in legs:
            ms, every, res = timed(lambda: ctx.fit_gamma_eta(eta, tau=tau, max_iter=a.steps, tol=0.0), a.reps)
            rows.append(dict(V=V, G=G, S_new=S, fit_eta=True, steps=a.steps, launches=2 * a.steps + 2, event_ms_median=ms, event_ms_all=every,
                             us_per_step=ms * 1e3 / a.steps, position_steps_per_s=float(V) * S * a.steps / (ms * 1e-3),
                             note="holds the eta-fixed reference fit of the same %d steps (loglik0)" % a.steps, lr_eta=res["lr_eta"]))
            print(json.dumps(rows[-1]), flush=True)
        if "fit" not in legs:
            ctx.close()
            continue
        ms, every, res = timed(lambda: ctx.fit_gamma(eta, tau=tau, presence=True), min(a.reps, 3))
        rows.append(dict(V=V, G=G, S_new=S, presence=True, fits=S * (1 + G), stop="default max_iter / tol of desman_amd._lib", event_ms_median=ms,
                         event_ms_all=every, iters_min=int(res["iters"].min()), iters_median=float(np.median(res["iters"])),
                         iters_max=int(res["iters"].max()), converged=int(res["converged"].sum())))
        print(json.dumps(rows[-1]), flush=True)
        if "interval" not in legs:
            ctx.close()
            continue
        ghat = res["gamma"]
        ms, every, iv = timed(lambda: ctx.fit_gamma_interval(eta, ghat, tau=tau, max_iter=a.interval_steps, tol=0.0), min(a.reps, 3))
        # inner fits of a search: the endpoint test and one per halving of its bracket down to ctol (none where an end is a boundary)
        width = np.stack([ghat, 1.0 - ghat])
        fits = int(np.where(width > 0, 1 + np.ceil(np.log2(np.maximum(width, _lib.FIT_CTOL) / _lib.FIT_CTOL)), 0).sum())
        rows.append(dict(V=V, G=G, S_new=S, interval=True, searches=2 * G * S, inner_fits_at_most=fits, steps_per_inner_fit=a.interval_steps,
                         ctol=_lib.FIT_CTOL, event_ms_median=ms, event_ms_all=every, boundary_ends=int(((iv["flags"] & 3) != 0).sum())))
        print(json.dumps(rows[-1]), flush=True)
        ctx.close()
    # CPU comparator: the numpy restatement, one process
    import _abund_ref as R
    Vc, Gc, Sc, nc = 1000, 8, 2, 50
    counts, tau, _ = synth_counts(Vc, Sc, Gc, seed=100 + Gc)
    t0 = time.perf_counter()
    for s in range(Sc):
        R.fit(counts[:, s], tau.astype(np.int64), eta, n_iter=nc)
    tc = time.perf_counter() - t0
    cpu = dict(what="numpy restatement (tests/_abund_ref.py: fit), one process, BLAS threads as the environment sets them", V=Vc, G=Gc, fits=Sc,
               steps=nc, seconds=tc, us_per_step_and_fit=tc * 1e6 / nc / Sc, position_steps_per_s=Vc * Sc * nc / tc)
    print(json.dumps(dict(cpu=cpu)))
    out = dict(command="python scripts/bench_abund.py --reps %d --steps %d --interval-steps %d --legs %s" % (a.reps, a.steps, a.interval_steps, a.legs), device=torch.cuda.get_device_name(0),
               timing="HIP events around Context.fit_gamma (counts resident), warm-up call, median of reps", cases=rows, cpu=cpu)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
