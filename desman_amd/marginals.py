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
PAIR_FLAG_LOW = 0.9     # Tau_pairs.csv has a row where the call of either haplotype has a marginal below this: a convention, not tuned
PHASE_MASS = 0.9        # kind `phase`: an unordered pair of bases has at least this mass, neither of its two orders does: a convention


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


# ---- the joint posterior of two haplotypes' bases (`desman --marginal-pairs`; _lib.Context.trace_rb_pairs)
def rb_pairs(stats, V=None):
    """From a trace_rb_pairs result (joint [V, P, 4, 4] and / or same_batch [B, P], pairs, dead, B, N, L): dict of
        J         [V, P, 4, 4]  joint / N: J[v, p, a, a'] = P(the pair's lower label carries a, the higher a' | data)
        p_same    [V, P]        the trace of J
        dist      [P]           the expected SNP distance V - mean over the used iterations of the number of positions with the same base
        dist_mcse [P]           its Monte Carlo standard error by batch means: sd of the B batch means / sqrt(B)
        differ    [P]           the share of positions with p_same < 0.5
    (J, p_same and differ only with joint; dist and dist_mcse only with same_batch, V taken from joint where it is not given) and pairs,
    dead, B, N, L.  With fewer than two batches everything is NaN."""
    B, N, L = int(stats["B"]), int(stats["N"]), int(stats["L"])
    out = dict(pairs=np.asarray(stats["pairs"], dtype=np.int64), dead=int(stats.get("dead", 0)), B=B, N=N, L=L)
    joint = None if stats.get("joint") is None else np.asarray(stats["joint"], dtype=np.float64)
    same = None if stats.get("same_batch") is None else np.asarray(stats["same_batch"], dtype=np.float64)
    if joint is not None:
        V = joint.shape[0]
        joint = joint.reshape(V, -1, 4, 4)
        J = joint / float(N) if B >= 2 else np.full(joint.shape, np.nan)
        p_same = np.trace(J, axis1=2, axis2=3)
        with np.errstate(invalid="ignore"):
            differ = (p_same < 0.5).mean(axis=0) if V and B >= 2 else np.full(J.shape[1], np.nan)
        out.update(J=J, p_same=p_same, differ=differ)
    if same is not None:
        if V is None:
            raise ValueError("rb_pairs: same_batch without joint needs the number of positions V")
        P = out["pairs"].shape[0]
        if B >= 2:
            means = same / float(L)                                   # [B, P] the batch means of the number of positions that agree
            out.update(dist=float(V) - means.mean(axis=0), dist_mcse=means.std(axis=0, ddof=1) / np.sqrt(B))
        else:
            out.update(dist=np.full(P, np.nan), dist_mcse=np.full(P, np.nan))
    return out


def pair_tables(J):
    """Per (position, pair) from normalised joints J [..., 4, 4]: dict of
        best, best_prob   the most probable ordered pair of bases k = 4 a + a' (ties to the lower k) and its probability
        p_same            sum_a J[a, a]
        swap              sum_{a < a'} 2 min(J[a, a'], J[a', a]): the mass that is indifferent to which of the two carries which base
        mi                the mutual information of the two digits, nats (0 ln 0 = 0)
        kind              'phase' where the unordered pair {a, a'}, a != a', of the largest mass has at least PHASE_MASS while neither
                          J[a, a'] nor J[a', a] has -- the data know the two bases, not who carries which --, else 'base'"""
    J = np.asarray(J, dtype=np.float64)
    flat = J.reshape(J.shape[:-2] + (16,))
    best = np.argmax(flat, axis=-1).astype(np.int64)
    best_prob = np.take_along_axis(flat, best[..., None], axis=-1)[..., 0]
    p_same = np.trace(J, axis1=-2, axis2=-1)
    Jt = np.swapaxes(J, -1, -2)
    iu = np.triu_indices(4, k=1)
    lo, hi = np.minimum(J, Jt)[..., iu[0], iu[1]], np.maximum(J, Jt)[..., iu[0], iu[1]]            # [..., 6]
    swap = 2.0 * lo.sum(axis=-1)
    unordered = (J + Jt)[..., iu[0], iu[1]]
    top = np.argmax(unordered, axis=-1)[..., None]
    u_top = np.take_along_axis(unordered, top, axis=-1)[..., 0]
    o_top = np.take_along_axis(hi, top, axis=-1)[..., 0]
    kind = np.where((u_top >= PHASE_MASS) & (o_top < PHASE_MASS), "phase", "base")
    rows, cols = J.sum(axis=-1), J.sum(axis=-2)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(J > 0, J * (np.log(J) - np.log(rows[..., :, None]) - np.log(cols[..., None, :])), 0.0)
    mi = np.maximum(term.sum(axis=(-1, -2)), 0.0)
    return dict(best=best, best_prob=best_prob, p_same=p_same, swap=swap, mi=mi, kind=kind)


def pair_flags(prob, pairs):
    """[V, P] bool: the (position, pair)s of Tau_pairs.csv -- the call of at least one of the two haplotypes has a marginal (prob [V, G]:
    calls()['prob']) below PAIR_FLAG_LOW"""
    prob = np.asarray(prob, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64)
    return np.minimum(prob[:, pairs[:, 0]], prob[:, pairs[:, 1]]) < PAIR_FLAG_LOW


def star_distance(star, pairs):
    """[P] int64: in how many positions the two haplotypes of every pair differ in the MAP state ``star`` ([V, G] digits or one-hot)"""
    d = tau_digits(star)
    pairs = np.asarray(pairs, dtype=np.int64)
    return (d[:, pairs[:, 0]] != d[:, pairs[:, 1]]).sum(axis=0).astype(np.int64)


def pairs_stride(n, L, target=50):
    """the K of a bare `--marginal-pairs`: the largest stride that still uses about ``target`` iterations and never fewer than the
    batch rule's minimum of two batches -- K = max(1, n // max(target, 2 L)), so ceil(n / K) >= min(n, max(target, 2 L))"""
    return max(1, int(n) // max(int(target), 2 * int(L)))
