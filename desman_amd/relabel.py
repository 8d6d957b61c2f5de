"""Posterior summaries of a chain that survive label switching.

The posterior is invariant under permutations of the haplotype labels, so nothing keeps "haplotype g" the same strain in every stored
iteration; averages over iterations (Tau_Mean, Gamma_mean) silently mix strains when a chain swaps labels.  Here every stored
iteration is matched to a reference -- the chain's own MAP haplotypes, or another run's -- by the permutation of its labels that
minimises the summed single-nucleotide distance.  The distances come from the tau trace resident on the device in one reduction
(_lib.Context.trace_snd: [n, G, G] integers); the matching is a minimum-cost assignment per iteration on the host (G <= 32).

``ctx`` below is a _lib.Context or anything with its ``trace_snd`` method and ``V`` / ``G`` / ``n_trace`` attributes.
"""
import numpy as np

from . import _lib


def min_cost_assignment(cost):
    """The permutation p (p[row] = column) of a square integer matrix that minimises sum_r cost[r, p[r]], and that minimum: the
    Hungarian method with potentials (shortest augmenting paths), O(G^3), exact in Python integers.  If the identity attains the
    minimum, the identity is returned: an iteration that did not switch keeps its labels whatever ties there are."""
    c = np.asarray(cost)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.dtype.kind not in "iu":
        raise ValueError("min_cost_assignment: a square integer matrix is expected; got %s %s" % (c.dtype, c.shape))
    n = c.shape[0]
    a = c.astype(object).tolist() if c.dtype.kind == "u" and c.dtype.itemsize == 8 else c.astype(np.int64).tolist()
    INF = float("inf")
    u, v = [0] * (n + 1), [0] * (n + 1)
    p, way = [0] * (n + 1), [0] * (n + 1)               # p[j] = row matched to column j (1-based; 0 = none)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = [INF] * (n + 1)
        used = [False] * (n + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], INF, 0
            row = a[i0 - 1]
            for j in range(1, n + 1):
                if not used[j]:
                    cur = row[j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(n + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    perm = np.zeros(n, dtype=np.int64)
    for j in range(1, n + 1):
        perm[p[j] - 1] = j - 1
    best = sum(a[r][int(perm[r])] for r in range(n))
    if sum(a[r][r] for r in range(n)) == best:
        perm = np.arange(n, dtype=np.int64)
    return perm, int(best)


def _reference(ctx, ref):
    """(mode, digits or None) of a reference given as None (the MAP record), [V,G] digits or [V,G,4] one-hot"""
    if ref is None:
        return _lib.SND_STAR, None
    r = np.asarray(ref)
    if r.ndim == 3 and r.shape[2] == 4:
        r = np.argmax(r, axis=2)
    if r.shape != (ctx.V, ctx.G):
        raise ValueError("relabel: the reference must hold the chain's %d positions and %d haplotypes; got %s" % (ctx.V, ctx.G, r.shape))
    return _lib.SND_GIVEN, np.ascontiguousarray(r, dtype=np.int64)


def relabel_trace(ctx, ref=None):
    """Per stored iteration the relabelling onto ``ref`` (default: the MAP haplotypes): dict of perm [n, G] uint8 (haplotype g of
    iteration t is the reference's haplotype perm[t, g]), cost_identity [n] and cost_best [n] (the summed distance before and after)
    and snd [n, G, G], the distances the matching was made on -- one trace_snd call."""
    mode, r = _reference(ctx, ref)
    snd = ctx.trace_snd(mode, ref=r)
    n, G = snd.shape[0], ctx.G
    perm = np.zeros((n, G), dtype=np.uint8)
    ident = np.trace(snd, axis1=1, axis2=2).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    best = np.zeros(n, dtype=np.int64)
    for t in range(n):
        perm[t], best[t] = min_cost_assignment(snd[t])
    return dict(perm=perm, cost_identity=ident, cost_best=best, snd=snd)


def inverse(perm):
    """inv[t, perm[t, g]] = g"""
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty_like(perm)
    np.put_along_axis(inv, perm, np.broadcast_to(np.arange(perm.shape[1]), perm.shape), axis=1)
    return inv


def gamma_mean_relabelled(gamma_store, perm):
    """the mean over iterations of gamma_store [n, S, G] with column g of iteration t moved to column perm[t, g]"""
    g = np.asarray(gamma_store, dtype=np.float64)
    inv = inverse(perm)
    return np.mean(np.take_along_axis(g, inv[:, None, :], axis=2), axis=0)


def snd_posterior(ctx, perm, level=0.95, snd_map=None):
    """The posterior of the distance between haplotypes g < h under the relabelling ``perm``: dict of pairs [P, 2] and, per pair, mean,
    sd (population form), lo, med, hi (quantiles (1 - level) / 2, 0.5, 1 - (1 - level) / 2 of the stored iterations) of the
    within-iteration distance, and -- where ``snd_map`` [G, G] is given -- map, the distance in the MAP state."""
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError("sndPosterior: level must lie in (0, 1); got %r" % level)
    d = ctx.trace_snd(_lib.SND_SELF)
    inv = inverse(perm)
    d = np.take_along_axis(np.take_along_axis(d, inv[:, :, None], axis=1), inv[:, None, :], axis=2)     # d'[t, a, b] = d[t, inv a, inv b]
    G = ctx.G
    gi, hi_ = np.triu_indices(G, k=1)
    x = d[:, gi, hi_].astype(np.float64)                      # [n, P]
    q = (1.0 - level) / 2.0
    out = dict(pairs=np.stack([gi, hi_], axis=1), mean=x.mean(axis=0), sd=x.std(axis=0))
    lo, med, hi = np.quantile(x, [q, 0.5, 1.0 - q], axis=0) if x.shape[1] else (np.zeros(0),) * 3
    out.update(lo=lo, med=med, hi=hi)
    if snd_map is not None:
        out["map"] = np.asarray(snd_map)[gi, hi_].astype(np.int64)
    return out


def haplotype_stability(ctx, rel):
    """How firmly the chain holds each haplotype of the reference ``rel`` (a relabel_trace result) was made on: per label the mean and
    the maximum over the stored iterations of the fraction of positions at which the iteration's haplotype of that label (after
    relabelling) differs from the reference's, and moved, the number of iterations whose matching gave the label to another index."""
    inv = inverse(rel["perm"])
    labels = np.arange(ctx.G)
    frac = rel["snd"][np.arange(inv.shape[0])[:, None], inv, labels[None, :]] / float(ctx.V)     # [n, G]
    return dict(mean=frac.mean(axis=0), max=frac.max(axis=0), moved=(inv != labels[None, :]).sum(axis=0).astype(np.int64))


def read_reference(path, positions, contigs, G):
    """The haplotypes of another run's Filtered_Tau_star.csv as [V, G] digits, for `desman --relabel-ref`.  The file must list exactly
    the positions of this run (contig names and Position column, in order) with G haplotypes; ValueError with the reason otherwise."""
    import pandas as pd
    t = pd.read_csv(path, header=0, index_col=0)
    if "Position" not in t.columns or (t.shape[1] - 1) % 4 != 0:
        raise ValueError("%s is not a Filtered_Tau_star.csv (a Position column, then four columns per haplotype)" % path)
    Gr = (t.shape[1] - 1) // 4
    if Gr != G:
        raise ValueError("%s holds %d haplotypes, this run infers %d: relabelling needs the same number" % (path, Gr, G))
    if t.shape[0] != len(positions) or list(t.index.astype(str)) != [str(c) for c in contigs] \
            or not np.array_equal(t["Position"].to_numpy(), np.asarray(positions)):
        raise ValueError("%s lists other positions than this run fits (%d rows there, %d here): relabelling needs the same positions"
                         % (path, t.shape[0], len(positions)))
    onehot = t.drop(columns="Position").to_numpy().reshape(t.shape[0], G, 4)
    if not (((onehot == 0) | (onehot == 1)).all() and (onehot.sum(axis=2) == 1).all()):
        raise ValueError("%s: every haplotype needs exactly one base per position" % path)
    return np.argmax(onehot, axis=2).astype(np.int64)
