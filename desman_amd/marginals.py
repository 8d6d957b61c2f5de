"""Rao-Blackwellised posterior marginals of tau for the positions of the fit: instead of averaging the sampled
one-hot digits (Tau_Mean.csv), average the exact full conditional q_t[v, l, a] = P(tau[v][g] = a | the rest of tau_t, gamma_t, eta_t,
data), l the label of haplotype g in iteration t, over the stored iterations.  Both averages estimate P(tau[v][l] = a | data); by
Rao-Blackwell the variance of q is never larger than that of the digit, its resolution is not 1 / n, and a cell whose base never flipped
no longer reads exactly 0 or 1.  The sums are made on the device (_lib.Context.trace_rb_marginals); this module turns them into tables.
Pure numpy; the same code serves the tests and the product.

The range rule is that of desman_amd/diagnose.py: with L the batch length, B = 2 (n // (2 L)) batches and N = B L, the LAST N of the n
stored iterations are used.

    p      = sum / N
    sigma2 = (B bsq - sum^2) / (B (B - 1) L)          the batch-means estimate, clipped at 0 (the sums are floating point here)
    mcse   = sqrt(sigma2 / N)
"""
import numpy as np

PROB_LOW = 0.9          # the threshold of the one summary line `desman --marginals` logs: a convention, not tuned


def rb_marginals(stats):
    """From a trace_rb_marginals result (sum, bsq [V, G, 4] float64, dead, B, N, L): dict of p, mcse, sigma2 [V, G, 4], dead, B, N, L;
    with fewer than two batches p and mcse are NaN"""
    s, bsq = np.asarray(stats["sum"], dtype=np.float64), np.asarray(stats["bsq"], dtype=np.float64)
    B, N, L = int(stats["B"]), int(stats["N"]), int(stats["L"])
    dead = int(stats.get("dead", 0))
    if B < 2:
        nan = np.full(s.shape, np.nan)
        return dict(p=nan, mcse=nan.copy(), sigma2=nan.copy(), dead=dead, B=B, N=N, L=L)
    sigma2 = np.maximum(B * bsq - s * s, 0.0) / float(B * (B - 1) * L)
    return dict(p=s / float(N), mcse=np.sqrt(sigma2 / N), sigma2=sigma2, dead=dead, B=B, N=N, L=L)


def tau_digits(tau):
    """[V, G] digits of a tau given as [V, G] digits or [V, G, 4] one-hot"""
    t = np.asarray(tau)
    return np.argmax(t, axis=2).astype(np.int64) if t.ndim == 3 else t.astype(np.int64)


def calls(p, star):
    """Per (position, haplotype) from marginals p [V, G, 4] and the MAP state ``star`` ([V, G] digits or one-hot): call (the base of
    the largest marginal, ties to the lower base), prob (its marginal), star, agree (call == star, 0 / 1) and entropy (nats,
    0 ln 0 = 0)"""
    p = np.asarray(p, dtype=np.float64)
    call = np.argmax(p, axis=2).astype(np.int64)                  # the first of equal maxima: the lower base
    prob = np.take_along_axis(p, call[:, :, None], axis=2)[:, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        entropy = -np.where(p > 0, p * np.log(p), 0.0).sum(axis=2)
    star = tau_digits(star)
    return dict(call=call, prob=prob, star=star, agree=(call == star).astype(np.int64), entropy=entropy)


def summary(cells, dead=0):
    """the numbers of the summary line: cells, expected_wrong = sum(1 - prob), low = cells with prob < PROB_LOW, disagree = cells whose
    call is not the MAP base, dead"""
    prob = np.asarray(cells["prob"], dtype=np.float64)
    return dict(cells=int(prob.size), expected_wrong=float((1.0 - prob).sum()), low=int((prob < PROB_LOW).sum()),
                disagree=int((np.asarray(cells["agree"]) == 0).sum()), dead=int(dead))
