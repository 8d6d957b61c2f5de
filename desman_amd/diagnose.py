"""Convergence diagnostics of a chain from its stored iterations: Monte Carlo standard error and effective sample
size by non-overlapping batch means, and split R-hat -- for the haplotype indicators x_t[v, l, a] = [label l has base a at position v
in iteration t] from exact integer batch sums made on the device (_lib.Context.trace_batch_stats), and for float series (lp, ll,
gamma) on the host.  Pure numpy; the same code serves the tests and the product.

The range rule, everywhere: with L the batch length, B = 2 (n // (2 L)) batches (even: two halves of equal length) and N = B L, the
LAST N of the n iterations are used and the first n - N are skipped.  Default L = floor(sqrt(n)).

    p      = sum / N
    sigma2 = (B bsq - sum^2) / (B (B - 1) L)          the batch-means estimate of the asymptotic variance of sqrt(N) (p - E p)
    mcse   = sqrt(sigma2 / N)
    ess    = N var / sigma2, var = p (1 - p)          (float series: the computed population variance); N where sigma2 = 0

ess is not capped at N: a series that alternates faster than independent draws (antithetic) has batch means that vary less than
those of independent draws, and its ess exceeds N -- that is information, not an error.  With fewer than two batches mcse and ess are
NaN.  Split R-hat compares the two halves (h = N / 2 iterations each) as two chains:

    W = mean_j s_j^2, s_j^2 = h / (h - 1) p_j (1 - p_j)   var+ = (h - 1) / h W + (p_1 - p_2)^2 / 2   R-hat = sqrt(var+ / W)

and where W = 0 it is 1 if the halves agree and inf if they do not; with h < 2 it is NaN.
"""
import math

import numpy as np

ESS_LOW, RHAT_HIGH = 100.0, 1.1          # the thresholds of the one summary line `desman --diagnose` logs: conventions, not tuned


def default_batch_len(n):
    """floor(sqrt(n)), at least 1"""
    return max(1, math.isqrt(max(int(n), 0)))


def batch_range(n, L):
    """(B, N, skip) of n stored iterations in batches of L"""
    n, L = int(n), int(L)
    if L < 1:
        raise ValueError("diagnose: the batch length must be at least 1; got %d" % L)
    B = 2 * (n // (2 * L))
    return B, B * L, n - B * L


def rhat(means, variances, n):
    """The potential scale reduction of m chains of n draws each from their means and sample variances (n - 1 form), both [m, ...]:
    sqrt(((n - 1) / n W + var_j(mean_j)) / W), W = mean_j variance_j; where W = 0: 1 if the means agree, else inf; NaN for n < 2"""
    means, variances = np.asarray(means, dtype=np.float64), np.asarray(variances, dtype=np.float64)
    if n < 2 or means.shape[0] < 2:
        return np.full(means.shape[1:], np.nan)
    W = variances.mean(axis=0)
    between = means.var(axis=0, ddof=1)
    same = (means == means[:1]).all(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(((n - 1.0) / n * W + between) / W)
    return np.where(W > 0, r, np.where(same, 1.0, np.inf))


def _indicator_variance(count, n):
    """the sample variance (n - 1 form) of a 0/1 series with ``count`` ones among n"""
    p = count / float(n)
    return n / (n - 1.0) * p * (1.0 - p)


def tau_diagnostics(stats):
    """From a trace_batch_stats result (sum, first, bsq [V, G, 4] int64, B, N, L): dict of p, mcse, ess, split_rhat [V, G, 4], sigma2
    and num = B bsq - sum^2 (int64: an exact 0 is a cell whose batches all hold the same count)."""
    s, bsq = np.asarray(stats["sum"], dtype=np.int64), np.asarray(stats["bsq"], dtype=np.int64)
    B, N, L = int(stats["B"]), int(stats["N"]), int(stats["L"])
    num = B * bsq - s * s
    nan = np.full(s.shape, np.nan)
    if B < 2:
        return dict(p=nan, mcse=nan, ess=nan.copy(), split_rhat=nan.copy(), sigma2=nan.copy(), num=num, B=B, N=N, L=L)
    p = s / float(N)
    sigma2 = num / float(B * (B - 1) * L)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.where(num > 0, N * p * (1.0 - p) / sigma2, float(N))
    out = dict(p=p, mcse=np.sqrt(sigma2 / N), ess=ess, sigma2=sigma2, num=num, B=B, N=N, L=L)
    if stats.get("first") is not None:
        f = np.asarray(stats["first"], dtype=np.int64)
        h = N // 2
        halves = np.stack([f, s - f])
        out["split_rhat"] = rhat(halves / float(h), _indicator_variance(halves, h) if h > 1 else halves * 0.0, h)
    return out


def scalar_diagnostics(series, L=None):
    """The same estimators for float series [n, ...] (one series per trailing index): dict of mean, sd (population form), mcse, ess,
    split_rhat over the last N iterations, with B, N, L.  Variances are computed from the values."""
    x = np.asarray(series, dtype=np.float64)
    n = x.shape[0]
    L = default_batch_len(n) if L is None else int(L)
    B, N, skip = batch_range(n, L)
    rest = x.shape[1:]
    nan = np.full(rest, np.nan)
    if B < 2:
        return dict(mean=nan, sd=nan.copy(), mcse=nan.copy(), ess=nan.copy(), split_rhat=nan.copy(), B=B, N=N, L=L)
    x = x[skip:]
    mean, var = x.mean(axis=0), x.var(axis=0)
    sigma2 = L * x.reshape((B, L) + rest).mean(axis=1).var(axis=0, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.where(sigma2 > 0, N * var / sigma2, float(N))
    h = N // 2
    halves = x.reshape((2, h) + rest)
    split = rhat(halves.mean(axis=1), halves.var(axis=1, ddof=1) if h > 1 else halves[:, 0] * 0.0, h)
    return dict(mean=mean, sd=np.sqrt(var), mcse=np.sqrt(sigma2 / N), ess=ess, split_rhat=split, B=B, N=N, L=L)


def relabel_gamma(gamma_store, perm):
    """gamma_store [n, S, G] with column g of iteration t moved to column perm[t, g] (perm None: as it is)"""
    g = np.asarray(gamma_store, dtype=np.float64)
    if perm is None:
        return g
    from .relabel import inverse
    return np.take_along_axis(g, inverse(perm)[:, None, :], axis=2)


def cell_summary(diag, flips):
    """Per (position, label) from a tau_diagnostics result: ess_min over the bases with 0 < p < 1 (N where there is none: the cell
    never moved), rhat_max over the four bases, flips, base (the most frequent one) and its p"""
    p, ess = diag["p"], diag["ess"]
    if diag["B"] < 2:
        nan = np.full(p.shape[:2], np.nan)
        return dict(ess_min=nan, rhat_max=nan.copy(), flips=np.asarray(flips), base=np.zeros(p.shape[:2], dtype=np.int64), p=nan.copy())
    mixed = (p > 0) & (p < 1)
    ess_min = np.where(mixed, ess, np.inf).min(axis=2)
    ess_min = np.where(np.isfinite(ess_min), ess_min, float(diag["N"]))
    base = np.argmax(p, axis=2)
    return dict(ess_min=ess_min, rhat_max=diag["split_rhat"].max(axis=2), flips=np.asarray(flips), base=base,
                p=np.take_along_axis(p, base[:, :, None], axis=2)[:, :, 0])


def flagged_share(cells):
    """the share of (position, label) cells with ess_min < ESS_LOW or rhat_max > RHAT_HIGH"""
    bad = (cells["ess_min"] < ESS_LOW) | (cells["rhat_max"] > RHAT_HIGH)
    return float(bad.mean()) if bad.size else 0.0


def rhat_chains(samplers, ref=None, batch_len=None):
    """The ordinary m-chain R-hat of replicate chains that still hold their contexts (HaploSNP_Sampler objects after update() or
    update_batch()).  Every chain's stored iterations are relabelled to ``ref`` ([V, G] digits or [V, G, 4] one-hot; default: the
    first chain's tau_star), each through one relabel_trace call with a given reference; the per-chain sums over the last N
    iterations come from trace_batch_stats under that relabelling.  Returns dict of tau [V, G, 4], gamma [S, G], lp (one number), N, L
    and m.  ValueError when the chains differ in shape."""
    from .relabel import relabel_trace
    samplers = list(samplers)
    if len(samplers) < 2:
        raise ValueError("rhat_chains: at least two chains are needed; got %d" % len(samplers))
    shapes = {(s.V, s.S, s.G, s.max_iter) for s in samplers}
    if len(shapes) != 1:
        raise ValueError("rhat_chains: the chains differ in shape (V, S, G, iterations): %s" % sorted(shapes))
    n = samplers[0].max_iter
    L = default_batch_len(n) if batch_len is None else int(batch_len)
    B, N, skip = batch_range(n, L)
    if B < 2:
        raise ValueError("rhat_chains: %d stored iterations are fewer than two batches of %d" % (n, L))
    ref = np.asarray(samplers[0].tau_star if ref is None else ref)
    counts, gm, gv, lm, lv = [], [], [], [], []
    for s in samplers:
        ctx = s._trace_ctx()
        perm = relabel_trace(ctx, ref)["perm"]
        counts.append(ctx.trace_batch_stats(L, perm=perm, want=("sum",))["sum"])
        g = relabel_gamma(s.gamma_store[:n], perm)[skip:]
        gm.append(g.mean(axis=0)); gv.append(g.var(axis=0, ddof=1))
        lp = np.asarray(s.lp_store[:n], dtype=np.float64)[skip:]
        lm.append(lp.mean()); lv.append(lp.var(ddof=1))
    counts = np.stack(counts)
    return dict(tau=rhat(counts / float(N), _indicator_variance(counts, N), N), gamma=rhat(np.stack(gm), np.stack(gv), N),
                lp=float(rhat(np.array(lm)[:, None], np.array(lv)[:, None], N)[0]), N=N, L=L, m=len(samplers))
