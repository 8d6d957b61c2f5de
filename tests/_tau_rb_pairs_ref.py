"""The specification of dsm_ctx_trace_rb_pairs (include/desman_hip.h) restated in numpy, for the tests.  It shares no
code with the kernel: the sixteen totals of a pair come from tests/_assign_pairs_ref.py: pair_candidates (numpy's logarithm, numpy's own
order over samples), the softmax, the dead rule, the relabelling with its transposition, the stride and the batch rule are written out
here.

For a used iteration (tau, gamma, eta), a position v and a pair g < h, the other bases at their values in tau:

    L_k  = pair_candidates                                                            k = 4 a + a'
    q_k  = exp(L_k - max) / (e_0 + e_1 + ... + e_15, in this order);  all sixteen -inf: the one-hot of the current pair, counted in dead
    same = ((q_0 + q_5) + q_10) + q_15

The tolerance (`k_bound`) is derived from operation counts the way tests/_tau_rb_ref.py: k_bound derives its own; nothing in it was
taken from the device's error.
"""
import numpy as np

from _assign_pairs_ref import pair_candidates
from _tau_rb_ref import EPS, LN_FLOOR, batch_range


def pair_list(G):
    return [(g, h) for g in range(G) for h in range(g + 1, G)]


def pair_index(G, l, m):
    """the place of the pair of labels {l, m} in lexicographic order"""
    lo, hi = min(l, m), max(l, m)
    return lo * (2 * G - lo - 1) // 2 + (hi - lo - 1)


def pair_conditionals(x, tau, gamma, eta):
    """x [V, S, 4] counts, tau [V, G] digits, gamma [S, G], eta [4, 4] -> dict of q [V, P, 16], L [V, P, 16], dead [V, P] bool and
    A [V, P] = the largest |L_k| among the finite totals (0 for a dead pair).  Every mixture value is a probability, so every term
    x ln p of a total has the same sign and |L_k| IS the sum of |x ln p| the tolerance is relative to."""
    x = np.asarray(x, dtype=np.int64)
    tau = np.asarray(tau, dtype=np.int64)
    gamma = np.asarray(gamma, dtype=np.float64)
    eta = np.asarray(eta, dtype=np.float64)
    V, G = tau.shape
    pairs = pair_list(G)
    X = x.astype(np.float64)
    q = np.zeros((V, len(pairs), 16))
    Lall = np.zeros((V, len(pairs), 16))
    A = np.zeros((V, len(pairs)))
    dead = np.zeros((V, len(pairs)), dtype=bool)
    for pi, (g, h) in enumerate(pairs):
        L = pair_candidates(X, gamma, eta, tau[:, None, :], g, h)[:, 0, :]                 # [V, 16]
        mx = L.max(axis=1)
        dd = np.isneginf(mx)
        with np.errstate(invalid="ignore"):
            e = np.where(np.isneginf(L), 0.0, np.exp(L - np.where(dd, 0.0, mx)[:, None]))
        tot = np.zeros(V)
        for k in range(16):
            tot = tot + e[:, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            qp = e / tot[:, None]
        onehot = np.eye(16)[4 * tau[:, g] + tau[:, h]]
        q[:, pi] = np.where(dd[:, None], onehot, qp)
        Lall[:, pi] = L
        dead[:, pi] = dd
        A[:, pi] = np.where(np.isfinite(L), np.abs(L), 0.0).max(axis=1)
    return dict(q=q, L=Lall, dead=dead, A=A, X=X.sum(axis=(1, 2)))


def k_bound(S, G, ln_floor=LN_FLOOR):
    """K of the tolerance |dq| <= q K eps A + K eps between the device and `pair_conditionals` (in units of eps = 2^-52, for tables with
    every mixture value p <= exp(-ln_floor) < 1, ln_floor <= 1):
        per term x ln p of a total L_k, relative to x |ln p| >= x ln_floor:
            (G + 9) / ln_floor     p itself: on either side at most G - 2 additions for the weights m, four products and three additions
                                   for rest, two products and two additions for the pair -- G + 9 roundings of half an eps each, all of
                                   positive numbers, on the device and as many in the restatement; taken through the logarithm (an
                                   absolute error, hence the floor)
            1 / ln_floor + 1       the table logarithm, documented within 1 ulp of max(1, |ln p|) (dsm_device.h), and libm's
            1                      the two roundings of x * ln p
            4 S                    two sums of 4 S terms in different orders, half an eps per term and sum each
        a q is exp(L_k - max) normalised: its relative error is that of L_k less the q-weighted mean of all sixteen, at most twice the
        largest error of a total; plus 24 eps for the subtraction, two exponentials good to an ulp or two, fifteen additions and the
        division on either side"""
    k1 = (G + 9.0) / ln_floor + 1.0 / ln_floor + 1.0 + 1.0 + 4.0 * S
    return 2.0 * k1 + 24.0


def q_tolerance(q, A, S, G, ln_floor=LN_FLOOR):
    """the allowed |dq| per cell [V, P, 16]"""
    K = k_bound(S, G, ln_floor)
    return q * (K * EPS) * A[:, :, None] + K * EPS


def used_iterations(n_it, stride, L):
    """(the indices, within the range, of the used iterations; B; n_used): every stride-th iteration of the range, of these the last B L"""
    taken = np.arange(0, n_it, stride)
    B, N, skip = batch_range(len(taken), L)
    return taken[skip:], B, len(taken)


def pairs(x, taus, gammas, etas, perm=None, L=1, stride=1, res=None, ln_floor=LN_FLOOR, no_floor=False):
    """the call restated: taus [n_it, V, G], gammas [n_it, S, G], etas [n_it, 4, 4] of the range, perm [n_it, G] or None -> dict of
    joint [V, P, 4, 4], same_batch [B, P], dead, tol_joint, tol_same (the allowed differences: the used iterations' q tolerances under
    the labels, plus the additions' roundings), res (the per-iteration `pair_conditionals` by index within the range, which another call
    on the same trace can be given), n_used, B, N, L.
    no_floor: for a table whose mixture values may reach 1 (eta = identity).  k_bound takes the error of a term relative to x |ln p|
    through |ln p| >= ln_floor; without that, relative to x max(|ln p|, ln_floor) <= x |ln p| + x ln_floor: A + ln_floor X, X the
    position's reads, stands in the place of A."""
    taus = np.asarray(taus, dtype=np.int64)
    n_it, V, G = taus.shape
    S = np.asarray(x).shape[1]
    P = G * (G - 1) // 2
    used, B, n_used = used_iterations(n_it, stride, L)
    N = B * L
    res = {} if res is None else res
    joint, tol_joint = np.zeros((V, P, 4, 4)), np.zeros((V, P, 4, 4))
    same_v, tol_same_v = np.zeros((B, V, P)), np.zeros((B, V, P))
    dead = 0
    for u, t in enumerate(used):
        if t not in res:
            res[t] = pair_conditionals(x, taus[t], gammas[t], etas[t])
        r = res[t]
        tq = q_tolerance(r["q"], r["A"] + (ln_floor * r["X"][:, None] if no_floor else 0.0), S, G, ln_floor)
        lab = np.arange(G) if perm is None else np.asarray(perm[t], dtype=np.int64)
        for pi, (g, h) in enumerate(pair_list(G)):
            slot = pair_index(G, lab[g], lab[h])
            q, tol = r["q"][:, pi].reshape(V, 4, 4), tq[:, pi].reshape(V, 4, 4)
            if lab[g] > lab[h]:
                q, tol = q.transpose(0, 2, 1), tol.transpose(0, 2, 1)
            joint[:, slot] = joint[:, slot] + q
            tol_joint[:, slot] += tol
            s = ((q[:, 0, 0] + q[:, 1, 1]) + q[:, 2, 2]) + q[:, 3, 3]
            same_v[u // L, :, slot] = same_v[u // L, :, slot] + s
            tol_same_v[u // L, :, slot] += tol[:, 0, 0] + tol[:, 1, 1] + tol[:, 2, 2] + tol[:, 3, 3] + 3 * EPS
        dead += int(r["dead"].sum())
    same_batch = np.zeros((B, P))
    for v in range(V):                                               # positions ascending from 0
        same_batch = same_batch + same_v[:, v, :]
    tol_joint += float(N) * N * EPS
    tol_same = tol_same_v.sum(axis=1) + float(L * V) * (L * V) * EPS
    return dict(joint=joint, same_batch=same_batch, dead=dead, tol_joint=tol_joint, tol_same=tol_same, res=res, n_used=n_used, B=B, N=N, L=L)


def exact_posterior(x, gamma, eta):
    """the exact posterior over all 4^G states of every position under (gamma, eta) and a flat prior: (post [V, 4^G], digits [4^G, G]),
    by enumeration -- numpy only, nothing of pair_candidates"""
    x = np.asarray(x, dtype=np.float64)
    S, G = gamma.shape
    n = 4 ** G
    digits = (np.arange(n)[:, None] >> (2 * np.arange(G))[None, :]) & 3                       # [n, G]
    onehot = (digits[:, :, None] == np.arange(4)[None, None, :]).astype(np.float64)             # [n, G, a]
    m = np.einsum("nga,sg->nsa", onehot, gamma)
    p = np.einsum("nsa,ab->nsb", m, eta)
    with np.errstate(divide="ignore"):
        lp = np.log(p)
    seen = x > 0
    L = np.zeros((x.shape[0], n))
    for v in range(x.shape[0]):
        L[v] = np.where(seen[v][None], x[v][None] * lp, 0.0).sum(axis=(1, 2))
    post = np.exp(L - L.max(axis=1, keepdims=True))
    return post / post.sum(axis=1, keepdims=True), digits


def exact_pair_joint(post, digits, g, h):
    """[V, 4, 4]: the exact posterior of (digit g, digit h)"""
    k = 4 * digits[:, g] + digits[:, h]
    return np.stack([np.bincount(k, weights=post[v], minlength=16) for v in range(post.shape[0])]).reshape(-1, 4, 4)
