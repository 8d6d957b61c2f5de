"""The partly held chain (dsm_ctx_gibbs_update_held_tau) as `desman-abund --novel K` uses it: the haplotypes of a
finished run are held, K further haplotypes are placed IN FRONT of them (the library holds the last haplotypes of a state) and
sampled together with the abundances on the counts of new samples.  Nothing here is tuned: the start is the one documented below.
"""
import os

import numpy as np
import pandas as pd

from .fixed_tau import summarize

MAX_G = 32                                   # include/desman_hip.h: DSM_MAX_G


def novel_labels(G, K):
    """haplotype labels in the column order of the chain: the K free ones first, then the run's G under their own numbers"""
    return ["novel%d" % k for k in range(K)] + ["%d" % g for g in range(G)]


def novel_start(counts, held, K, seed):
    """tau digits [V, K + G] of the start state: columns K.. are ``held`` ([V,G] digits), every free digit is drawn uniformly from the
    bases with a non-zero count at its position, pooled over the samples (all four where a position has no read), by
    numpy.random.RandomState(seed mod 2^32): one uniform per (position, free haplotype), position-major"""
    counts, held = np.asarray(counts), np.asarray(held, dtype=np.int64)
    V, G = held.shape
    if counts.ndim != 3 or counts.shape[0] != V or counts.shape[2] != 4:
        raise ValueError("novel_start: counts must be [V,S,4] with the V of the held haplotypes")
    if K < 1 or G < 1 or G + K > MAX_G:
        raise ValueError("novel_start: need K >= 1, G >= 1 and G + K <= %d haplotypes" % MAX_G)
    seen = counts.sum(axis=1) > 0                                               # [V,4]
    seen[~seen.any(axis=1)] = True
    n = seen.sum(axis=1)                                                        # 1..4 candidate bases per position
    order = np.argsort(~seen, axis=1, kind="stable")                            # the candidate bases first, ascending
    u = np.random.RandomState(int(seed) & 0xFFFFFFFF).random_sample((V, K))
    pick = np.minimum((u * n[:, None]).astype(np.int64), n[:, None] - 1)
    free = np.take_along_axis(order, pick, axis=1)
    return np.ascontiguousarray(np.concatenate([free, held], axis=1), dtype=np.int64)


def onehot(digits):
    d = np.asarray(digits, dtype=np.int64)
    out = np.zeros(d.shape + (4,), dtype=np.int64)
    np.put_along_axis(out, d[..., None], 1, axis=2)
    return out


def novel_chain(counts, held, eta, K, n_iter=1000, burn=200, fix_eta=True, level=0.95, seed=0, alpha=0.1, delta=0.1, epsilon=1.0e-6,
                device=0, context=None):
    """n_iter iterations of the chain with ``held`` ([V,G] digits) held and K free haplotypes in front of them on ``counts`` [V,S,4], from
    novel_start(), uniform abundance rows and ``eta`` (held unless fix_eta is False); stream key ``seed``, MT19937 seed = its low 31
    bits (1 if those are 0).  Returns summarize() of the kept abundance draws [n_iter - burn, S, K + G] plus ll (kept iterations),
    tau_star [V, K + G] digits, gamma_star, lp_star, start (the start digits) and labels.  ``context`` (tests): a class to use in place
    of _lib.Context."""
    x = np.ascontiguousarray(counts, dtype=np.int64)
    n_iter, burn = int(n_iter), int(burn)
    if n_iter < 1 or burn < 0 or burn >= n_iter:
        raise ValueError("novel_chain: need n_iter >= 1 and 0 <= burn < n_iter")
    held = np.ascontiguousarray(held, dtype=np.int64)
    start = novel_start(x, held, K, seed)
    S, G = x.shape[1], held.shape[1]
    if context is None:
        from . import _lib
        context = _lib.Context
    ctx = context(device)
    try:
        ctx.set_counts(x)
        ctx.set_priors(alpha, delta, epsilon)
        ctx.set_state(onehot(start), np.full((S, G + K), 1.0 / (G + K)), np.ascontiguousarray(eta, dtype=np.float64))
        ctx.seed((int(seed) & 0x7FFFFFFF) or 1, ctr_seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        ctx.gibbs_update_held_tau(n_iter, G, fix_eta=fix_eta)
        tr, star = ctx.get_trace(), ctx.get_star()
    finally:
        ctx.close()
    res = summarize(tr["gamma"][burn:], level)
    res["ll"] = np.asarray(tr["ll"][burn:])
    res["tau_star"] = np.ascontiguousarray(np.argmax(np.asarray(star["tau"]) == 1, axis=2), dtype=np.int64)
    res["gamma_star"], res["lp_star"] = np.asarray(star["gamma"]), float(star["lp"])
    res["start"], res["labels"] = start, novel_labels(G, K)
    return res


def fit_rows(base, novel, K):
    """the two rows of Novel_fit.csv from the K = 0 chain (fixed_tau.posterior_gamma) and the chain with K free haplotypes"""
    rows = []
    for k, r in ((0, base), (K, novel)):
        rows.append({"K": k, "deviance": -2.0 * float(np.mean(r["ll"])), "lp_star": float(r["lp_star"]), "iters": int(len(r["ll"]))})
    return pd.DataFrame(rows).set_index("K")


def haplotype_rows(novel, K):
    """Novel_haplotypes.csv: per free haplotype of the MAP state the number of positions in which it differs from the nearest held
    haplotype (the lowest-numbered one on a tie), that haplotype's label, and the mean / largest posterior-mean abundance over samples"""
    star, labels = novel["tau_star"], novel["labels"]
    held = star[:, K:]
    rows = []
    for k in range(K):
        d = (star[:, k][:, None] != held).sum(axis=0)
        h = int(np.argmin(d))
        rows.append({"haplotype": labels[k], "distance": int(d[h]), "nearest": labels[K + h],
                     "mean_abundance": float(novel["mean"][:, k].mean()), "max_abundance": float(novel["mean"][:, k].max())})
    return pd.DataFrame(rows).set_index("haplotype")


def write_novel(out_dir, names, contigs, positions, base, novel, K):
    """the five Novel_* files of `desman-abund --novel K`"""
    os.makedirs(out_dir, exist_ok=True)
    labels = novel["labels"]
    flat = onehot(novel["tau_star"]).reshape(len(contigs), -1)                  # Filtered_Tau_star.csv's layout (Output_Results._haplotype_table)
    frame = pd.DataFrame(flat, index=list(contigs))
    frame.insert(0, "Position", np.asarray(positions))
    frame.to_csv(os.path.join(out_dir, "Novel_Tau_star.csv"))
    pd.DataFrame(novel["gamma_star"], index=names, columns=labels).to_csv(os.path.join(out_dir, "Novel_Gamma_star.csv"))
    cols = {}
    for g, lab in enumerate(labels):
        for key in ("mean", "sd", "lo", "med", "hi"):
            cols["%s_%s" % (lab, key)] = novel[key][:, g]
    pd.DataFrame(cols, index=names).to_csv(os.path.join(out_dir, "Novel_Gamma_posterior.csv"))
    fit_rows(base, novel, K).to_csv(os.path.join(out_dir, "Novel_fit.csv"))
    haplotype_rows(novel, K).to_csv(os.path.join(out_dir, "Novel_haplotypes.csv"))
