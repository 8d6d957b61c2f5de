"""The specification of dsm_ctx_trace_rb_marginals (include/desman_hip.h) restated in numpy, for the tests.

For a stored iteration (tau, gamma, eta), a position v and a haplotype g

    rest[s][b] = the chain from 0 over h != g, h ascending, of eta[tau[v][h]][b] * gamma[s][h]          (G = 1: 0)
    L_a        = sum over s, b with x[v][s][b] > 0 of x ln(rest[s][b] + eta[a][b] gamma[s][g])            a = 0..3
    q_a        = exp(L_a - max) / (((e_0 + e_1) + e_2) + e_3);  all four -inf: the one-hot of tau[v][g], counted in `dead`

The device forms the links of the chain with fused multiply-adds, its logarithm is the table one and its sum over (s, b) has another
order: the comparison is by the tolerance of `k_bound`, not by bits.  The accumulation over iterations, however, has the device's order
(`accumulate`): a batch sum is the t-ascending sum from 0, the batch sums and their squares are added batches ascending.
"""
import numpy as np

EPS = 2.0 ** -52
LN_FLOOR = -np.log(0.85)          # the tests' tables keep every mixture value p <= 0.85, so |ln p| >= LN_FLOOR (asserted through `pmax`)


def conditionals(x, tau, gamma, eta):
    """x [V, S, 4] counts, tau [V, G] digits, gamma [S, G], eta [4, 4] -> dict of q [V, G, 4], L [V, G, 4], dead [V, G] bool,
    A [V, G] = max over the candidates with a finite total of sum x |ln p| (0 for a dead cell) and pmax = the largest mixture value
    under a positive count"""
    x = np.asarray(x, dtype=np.int64)
    tau = np.asarray(tau, dtype=np.int64)
    gamma = np.asarray(gamma, dtype=np.float64)
    eta = np.asarray(eta, dtype=np.float64)
    V, S, _ = x.shape
    G = tau.shape[1]
    xf = x.astype(np.float64)                                       # exact: counts are below 2^31
    seen = np.broadcast_to((x > 0)[:, None, :, :], (V, 4, S, 4))
    q = np.zeros((V, G, 4))
    Lall = np.zeros((V, G, 4))
    A = np.zeros((V, G))
    dead = np.zeros((V, G), dtype=bool)
    pmax = 0.0
    link = [eta[tau[:, h]][:, None, :] * gamma[None, :, h, None] for h in range(G)]        # [V, S, 4] each
    for g in range(G):
        rest = np.zeros((V, S, 4))
        for h in range(G):
            if h != g:
                rest += link[h]
        p = rest[:, None, :, :] + eta[None, :, None, :] * gamma[None, None, :, g, None]    # [V, a, S, b]
        lg = np.zeros((V, 4, S, 4))
        with np.errstate(divide="ignore"):
            np.log(p, out=lg, where=seen)                               # an unseen cell keeps 0; 0 under a count: -inf
        term = xf[:, None, :, :] * lg                                   # x = 0 meets only the 0 it kept
        L = term.sum(axis=(2, 3))
        Aa = np.abs(term).sum(axis=(2, 3))
        pmax = max(pmax, float(np.where(seen, p, 0.0).max()))
        mx = L.max(axis=1)
        dd = np.isneginf(mx)
        with np.errstate(invalid="ignore"):
            e = np.where(np.isneginf(L), 0.0, np.exp(L - np.where(dd, 0.0, mx)[:, None]))
        tot = ((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            qg = e / tot[:, None]
        onehot = np.eye(4)[tau[:, g]]
        q[:, g] = np.where(dd[:, None], onehot, qg)
        Lall[:, g] = L
        dead[:, g] = dd
        A[:, g] = np.where(np.isfinite(Aa), Aa, 0.0).max(axis=1)
    return dict(q=q, L=Lall, dead=dead, A=A, pmax=pmax)


def k_bound(S, G):
    """K of the tolerance |dq| <= q K eps A + K eps between the device and `conditionals` (derived in DESIGN.md sec. 8j; in units of
    eps = 2^-52, for tables with every mixture value p <= 0.85):
        per term x ln p of a total L_a, relative to x |ln p| >= x LN_FLOOR:
            (3 G + 1) / 2 / LN_FLOOR   p itself: G + 1 roundings in the device's fma chain, 2 G in the restatement's, half an eps each, taken
                                       through the logarithm (an absolute error, hence the floor)
            1 / LN_FLOOR + 1           the table logarithm, documented within 1 ulp of max(1, |ln p|) (dsm_device.h), and libm's
            1                          the two roundings of x * ln p
            4 S                        two sums of 4 S terms in different orders, half an eps per term and sum each
        a q is exp(L_a - max) normalised: twice the largest error of a total, plus 10 eps for the subtraction, two exponentials good to
        an ulp or two, three additions and the division on either side"""
    return k_bound_at(S, G, LN_FLOOR)


def k_bound_at(S, G, ln_floor):
    """k_bound for a table whose mixture values stay at or below exp(-ln_floor) < 1 (ln_floor <= 1)"""
    k1 = (3.0 * G + 1.0) / 2.0 / ln_floor + 1.0 / ln_floor + 1.0 + 1.0 + 4.0 * S
    return 2.0 * k1 + 10.0


def q_tolerance(q, A, S, G, ln_floor=LN_FLOOR):
    """the allowed |dq| per cell [V, G, 4]"""
    K = k_bound_at(S, G, ln_floor)
    return q * (K * EPS) * A[:, :, None] + K * EPS


def batch_range(n_it, L):
    B = 2 * (n_it // (2 * L))
    return B, B * L, n_it - B * L


def accumulate(qs, perm, L):
    """qs [n_it, V, G, 4] per-iteration conditionals, perm [n_it, G] labels or None, batch length L -> (sum, bsq) [V, G, 4] over the last
    B L iterations in the device's order"""
    qs = np.asarray(qs, dtype=np.float64)
    n_it, V, G, _ = qs.shape
    B, N, skip = batch_range(n_it, L)
    total, bsq = np.zeros((V, G, 4)), np.zeros((V, G, 4))
    for b in range(B):
        bs = np.zeros((V, G, 4))
        for t in range(skip + b * L, skip + (b + 1) * L):
            lab = np.arange(G) if perm is None else np.asarray(perm[t], dtype=np.int64)
            bs[:, lab, :] = bs[:, lab, :] + qs[t]
        total = total + bs
        bsq = bsq + bs * bs
    return total, bsq


def marginals(x, taus, gammas, etas, perm=None, L=1, res=None, data_floor=False):
    """the call restated: taus [n_it, V, G], gammas [n_it, S, G], etas [n_it, 4, 4] -> dict of sum, bsq, dead (cell-iterations among the
    used ones), tol (the allowed difference of `sum`: the used iterations' q tolerances under the labels, plus N^2 eps for the
    additions), qs, res (the per-iteration `conditionals`, which another call on the same trace can be given), pmax, B, N, L.
    data_floor: the tolerance with -ln(pmax) of this trace in the place of LN_FLOOR (a chain's own eta, whose diagonal is above 0.85)"""
    taus = np.asarray(taus, dtype=np.int64)
    n_it, V, G = taus.shape
    S = np.asarray(x).shape[1]
    B, N, skip = batch_range(n_it, L)
    if res is None:
        res = [conditionals(x, taus[t], gammas[t], etas[t]) for t in range(n_it)]
    qs = np.stack([r["q"] for r in res]) if n_it else np.zeros((0, V, G, 4))
    pmax = max([r["pmax"] for r in res] + [0.0])
    floor = min(1.0, -np.log(pmax)) if data_floor else LN_FLOOR
    total, bsq = accumulate(qs, perm, L)
    tol = np.zeros((V, G, 4))
    dead = 0
    for t in range(skip, n_it):
        lab = np.arange(G) if perm is None else np.asarray(perm[t], dtype=np.int64)
        tol[:, lab, :] += q_tolerance(res[t]["q"], res[t]["A"], S, G, floor)
        dead += int(res[t]["dead"].sum())
    tol += float(N) * N * EPS
    return dict(sum=total, bsq=bsq, dead=dead, tol=tol, qs=qs, res=res, pmax=pmax, B=B, N=N, L=L)


def smooth_trace(rng, n_it, V, S, G):
    """a planted trace whose mixture values stay at or below 0.84: eta with a diagonal in [0.6, 0.84] and the rest of each row split at
    random, gamma rows from a flat Dirichlet, tau uniform"""
    taus = rng.randint(0, 4, size=(n_it, V, G)).astype(np.int64)
    gammas = rng.dirichlet(np.ones(G), size=(n_it, S))
    etas = np.zeros((n_it, 4, 4))
    for t in range(n_it):
        for a in range(4):
            d = rng.uniform(0.6, 0.84)
            off = rng.dirichlet(np.ones(3)) * (1.0 - d)
            etas[t, a] = np.insert(off, a, d)
    return taus, gammas, etas


def sparse_counts(rng, V, S, hi=300, zero_share=0.25):
    """counts 0..hi with about ``zero_share`` of the cells zero"""
    x = rng.randint(0, hi + 1, size=(V, S, 4)).astype(np.int64)
    x[rng.uniform(size=x.shape) < zero_share] = 0
    return x
