"""Plain numpy restatement of the profile-likelihood intervals (include/desman_hip.h: dsm_fit_gamma_interval) -- a helper of
tests/test_abund_interval_cpu.py and tests/test_gpu_abund_interval.py, not a test file.

One sample: x [V,4] counts, tau [V,G] digits, eta [4,4], ghat [G] the fitted row.  For haplotype g
    l_g(c) = max { L(gamma) : gamma_g = c, gamma_h >= 0, sum gamma = 1 },     interval = { c : 2 (L(ghat) - l_g(c)) <= q }.
As in _abund_ref, written with the G-term sums per haplotype, not with the class sums of the kernel.  The rules are the header's, line
by line: the inner fit (gamma_g held at c, the others rescaled to 1 - c), its start, the endpoint test and the bisection."""
from statistics import NormalDist

import numpy as np

import _abund_ref as R


def quantile(level):
    """chi-square (1 d.o.f.) quantile: 3.841... for 0.95"""
    return NormalDist().inv_cdf(0.5 * (1.0 + level)) ** 2


def _sum(values):
    """left to right"""
    s = 0.0
    for v in values:
        s += float(v)
    return s


def inner_fit(x, E, g, c, prev, ghat, max_iter, tol):
    """the constrained fit at gamma_g = c started from the free part of `prev`: (l, the row it ended at, ended at max_iter?).
    A cell with reads and p = 0: l = -inf (and the row before that pass)."""
    G = E.shape[1]
    free = [h for h in range(G) if h != g]
    gam = np.array(prev, dtype=np.float64)
    F = _sum(gam[free])
    if not F > 0.0:
        gam = np.array(ghat, dtype=np.float64)
        F = _sum(gam[free])
        if not F > 0.0:
            gam = np.ones(G)
            F = float(G - 1)
    omc = 1.0 - c
    new = np.zeros(G)
    new[g] = c
    for h in free:
        new[h] = omc if G == 2 else omc * (0.999 * (gam[h] / F) + 0.001 / (G - 1))
    gam = new
    conv = G == 2 or c == 1.0                              # nothing to fit: one evaluation
    iters = 0
    xf = np.asarray(x, dtype=np.float64)
    pos = xf > 0
    while not conv and iters < max_iter:
        p = np.einsum("g,vgb->vb", gam, E)
        if (p[pos] <= 0).any():
            return -np.inf, gam, False
        q = np.zeros_like(xf)
        q[pos] = xf[pos] / p[pos]
        r = gam * np.einsum("vgb,vb->g", E, q)
        Rs = _sum(r[free])
        if not Rs > 0.0:
            conv = True
            break
        new = np.where(gam > 0.0, omc * r / Rs, 0.0)
        new[g] = c
        delta = np.abs(new - gam).max()
        gam = new
        iters += 1
        if tol > 0 and delta < tol:
            conv = True
    return R.loglik(x, E, gam), gam, not conv


def profile(x, tau, eta, ghat, g, c, max_iter=20000, tol=1e-9):
    """l_g(c) by one inner fit from ghat's free part"""
    return inner_fit(np.asarray(x, dtype=np.int64), R.emission(tau, eta), g, c, ghat, ghat, max_iter, tol)[0]


def interval(x, tau, eta, ghat, q, max_iter=20000, tol=1e-9, ctol=1e-6, trace=None):
    """(lo [G], hi [G], flags [G]) of one sample; trace: a list that receives (g, side, c, l, Lhat) of every inner fit"""
    x = np.asarray(x, dtype=np.int64)
    E = R.emission(tau, eta)
    G = E.shape[1]
    ghat = np.asarray(ghat, dtype=np.float64)
    nan = np.full(G, np.nan)
    if not ghat.any():
        return nan, nan.copy(), np.zeros(G, dtype=np.int32)
    if G == 1:
        return np.ones(1), np.ones(1), np.full(1, 2, dtype=np.int32)
    if x.sum() == 0:
        return np.zeros(G), np.ones(G), np.full(G, 3, dtype=np.int32)
    Lhat = R.loglik(x, E, ghat)
    if Lhat == -np.inf:
        return nan, nan.copy(), np.zeros(G, dtype=np.int32)
    ends = np.zeros((G, 2))
    flags = np.zeros(G, dtype=np.int32)
    for g in range(G):
        for side in (0, 1):
            b_in, b_out = float(ghat[g]), float(side)
            if b_in == b_out:
                ends[g, side] = b_out
                flags[g] |= 2 if side else 1
                continue
            gam, endpoint, c = ghat, True, b_out
            while True:
                ll, gam, hit = inner_fit(x, E, g, c, gam, ghat, max_iter, tol)
                if trace is not None:
                    trace.append((g, side, c, ll, Lhat))
                if hit:
                    flags[g] |= 4
                inside = 2.0 * (Lhat - ll) <= q
                if endpoint:
                    endpoint = False
                    if inside:
                        ends[g, side] = b_out
                        flags[g] |= 2 if side else 1
                        break
                elif inside:
                    b_in = c
                else:
                    b_out = c
                m = 0.5 * (b_in + b_out)
                if not abs(b_out - b_in) > ctol or m == b_in or m == b_out:
                    ends[g, side] = b_in
                    break
                c = m
    return ends[:, 0].copy(), ends[:, 1].copy(), flags


def interval_samples(counts, tau, eta, gamma_hat, q, **kw):
    """interval() for every sample of counts [V,S,4]: dict of lo [S,G], hi [S,G], flags [S,G]"""
    rows = [interval(counts[:, s, :], tau, eta, gamma_hat[s], q, **kw) for s in range(counts.shape[1])]
    return dict(lo=np.array([r[0] for r in rows]), hi=np.array([r[1] for r in rows]), flags=np.array([r[2] for r in rows]))
