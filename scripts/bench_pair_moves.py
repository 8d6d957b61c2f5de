"""Cost of pair moves in the main chain (dsm_ctx_set_pair_moves) -> profiles/pair_moves_bench.json.

    python scripts/bench_pair_moves.py [--out profiles/pair_moves_bench.json] [--iters 200] [--reps 7]
                                       [--parent-tree DIR] [--rounds 3]

ms per Gibbs iteration of dsm_ctx_gibbs_update at V = 10 000, S = 64, G = 8 and at V = 1000, S = 16, G = 5, for E = 0 (off), 5 and 1:
HIP events around a call of --iters iterations, one warm-up call, median of --reps.  There is no target; the file records what came out.

--parent-tree DIR: a built checkout of the parent commit.  E = 0 is then measured against it in the same session, alternating the two:
--rounds times (parent, this tree), each in a fresh process that measures E = 0 on both tables the same way.  The file records every
round's median of both and the spread (largest minus smallest) of the parent's own rounds, which is what the difference is read against.
The fresh processes run before this one opens the GPU.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(10000, 64, 8), (1000, 16, 5)]                                  # V, S, G
EVERY = (0, 5, 1)


def timed(fn, reps):
    import torch
    fn()                                                                 # warm-up
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [float(x) for x in ms]


def measure(tree, every, iters, reps):
    """rows of (V, S, G, E) -> ms per iteration, with the package of `tree`"""
    sys.path.insert(0, tree)
    import torch                                                         # before the library: one HIP runtime per process, torch's
    from desman_amd import _lib
    from desman_amd.synth import synth_counts, random_state
    rows = []
    for V, S, G in CASES:
        counts, _, _ = synth_counts(V, S, G, seed=V + S + G)
        tau, gamma, eta = random_state(V, S, G, seed=G)
        ctx = _lib.Context(0)
        ctx.set_counts(counts)
        for E in every:
            ctx.set_state(tau, gamma, eta)
            ctx.seed(7)
            if E:
                ctx.set_pair_moves(E)
            ms, each = timed(lambda: ctx.gibbs_update(iters), reps)
            rows.append(dict(V=V, S=S, G=G, E=E, iters=iters, ms_per_iteration=ms / iters, event_ms_all=each))
            print("V=%d S=%d G=%d E=%d  %8.3f ms / %d = %8.2f us per iteration" % (V, S, G, E, ms, iters, 1e3 * ms / iters), flush=True)
        ctx.close()
    return rows, torch.cuda.get_device_name(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_moves_bench.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-tree", dest="parent_tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)     # a fresh process of the A/B: the tree to measure E = 0 with
    a = ap.parse_args()
    if a.child is not None:
        rows, _ = measure(a.child, (0,), a.iters, a.reps)
        print("RESULT " + json.dumps(rows), flush=True)
        return
    ab = None
    if a.parent_tree is not None:
        ab = dict(parent=[], this=[])
        for r in range(a.rounds):
            for name, tree in (("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)):
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--iters", str(a.iters), "--reps", str(a.reps)],
                                     capture_output=True, text=True, timeout=300, cwd=tree)
                if run.returncode != 0:
                    sys.exit("the %s process of round %d ended with %d:\n%s" % (name, r, run.returncode, run.stderr[-2000:]))
                line = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1]
                ab[name].append(json.loads(line[len("RESULT "):]))
                print("round %d %-6s %s" % (r, name, ["%.2f us" % (1e3 * x["ms_per_iteration"]) for x in ab[name][-1]]), flush=True)
    rows, device = measure(ROOT, EVERY, a.iters, a.reps)
    out = dict(what="dsm_ctx_gibbs_update with pair moves off (E = 0), after every fifth iteration (E = 5) and after every iteration (E = 1): "
                    "ms per Gibbs iteration",
               device=device, timing="HIP events around a call of `iters` iterations, one warm-up call, median of reps",
               not_measured=["the pair kernel in isolation by kernel trace", "G > 8", "a target: there is none"], cases=rows)
    if ab is not None:
        cmp_rows = []
        for i, (V, S, G) in enumerate(CASES):
            p = [r[i]["ms_per_iteration"] for r in ab["parent"]]
            t = [r[i]["ms_per_iteration"] for r in ab["this"]]
            cmp_rows.append(dict(V=V, S=S, G=G, parent_ms_per_iteration=p, this_ms_per_iteration=t, parent_median=float(np.median(p)),
                                 this_median=float(np.median(t)), parent_spread=float(max(p) - min(p)),
                                 within_parent_spread=bool(abs(np.median(t) - np.median(p)) <= max(p) - min(p))))
        out["e0_against_parent"] = dict(how="alternating fresh processes (parent, this), %d rounds, E = 0, the same tables and timing" % a.rounds,
                                        cases=cmp_rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
