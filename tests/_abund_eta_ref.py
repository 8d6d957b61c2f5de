"""Plain numpy restatement of the joint fit of abundances and error matrix (include/desman_hip.h: dsm_fit_gamma_eta) -- a helper of
tests/test_abund_eta_cpu.py and tests/test_gpu_abund_eta.py, not a test file.

counts [V,S,4], tau [V,G] digits fixed; gamma [S,G] and ONE eta [4,4] ([true][observed]) shared by the samples:
    L(gamma, eta) = sum_s sum_{v,b: x > 0} x_svb ln p_svb,     p_svb = sum_g gamma_sg eta[tau_vg][b]
One EM step from a single E-step, q = x / p where x > 0:
    gamma'_sg = gamma_sg / N_s  sum_{v,b} q_svb eta[tau_vg][b]
    M[a][b]   = eta[a][b]  sum_s sum_v sum_{g: tau_vg = a} gamma_sg q_svb,      eta'[a][b] = M[a][b] / sum_b M[a][b]
Written with the G-term sums per haplotype (one-hot T[v,g,a], E[v,g,b] = eta[tau_vg][b]) -- NOT with the class sums the kernel uses --
as tests/_abund_ref.py is, whose fit() gives loglik0."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _abund_ref as R  # noqa: E402

CHI2_12_999 = 32.90949040736021          # the 0.999 quantile of chi-square with 12 degrees of freedom


def onehot(tau):
    return np.eye(4)[np.asarray(tau, dtype=np.int64)]                     # T[v,g,a]


def sample_step(x, T, gamma, eta, reverse=False):
    """one sample's part of a step: (gamma' row, its 4 x 4 sums  sum_v sum_{g: tau_vg = a} gamma_g q_vb, bad)"""
    x = np.asarray(x, dtype=np.float64)
    if reverse:                                                           # the same sums over the positions in the opposite order
        x, T = x[::-1], T[::-1]
    E = np.einsum("vga,ab->vgb", T, eta)
    p = np.einsum("g,vgb->vb", gamma, E)
    pos = x > 0
    if (p[pos] <= 0).any():
        return gamma, np.zeros((4, 4)), True
    q = np.zeros_like(x)
    q[pos] = x[pos] / p[pos]
    r = np.einsum("vgb,vb->g", E, q)
    part = np.einsum("g,vga,vb->ab", gamma, T, q)
    return gamma * r / x.sum(), part, False


def step(counts, T, gamma, eta, reverse=False, order=None):
    """one step for all samples: (gamma', eta', delta, dead-row mask, bad).  Samples without reads keep their row and add nothing; the
    samples' sums are added in index order (`order`: another order, for the summation-order yardstick)"""
    S = counts.shape[1]
    new = gamma.copy()
    tot = np.zeros((4, 4))
    for s in (range(S) if order is None else order):
        if counts[:, s].sum() == 0:
            continue
        row, part, bad = sample_step(counts[:, s], T, gamma[s], eta, reverse)
        if bad:
            return gamma, eta, 0.0, 0, True
        new[s] = row
        tot = tot + part
    M = eta * tot
    eta_new, rows = eta.copy(), 0
    for a in range(4):
        rs = ((M[a, 0] + M[a, 1]) + M[a, 2]) + M[a, 3]
        if rs > 0:
            eta_new[a] = M[a] / rs
        else:
            rows |= 1 << a                                                # a dead row keeps its values
    delta = max(np.abs(new - gamma).max(), np.abs(eta_new - eta).max())
    return new, eta_new, delta, rows, False


def loglik(counts, tau, gamma, eta):
    """per-sample L at (gamma, eta): an array [S]; 0 for a sample without reads, -inf where a cell with reads has p = 0"""
    E = R.emission(tau, eta)
    return np.array([R.loglik(counts[:, s], E, gamma[s]) for s in range(counts.shape[1])])


def fit(counts, tau, eta0, n_iter=None, tol=0.0, max_iter=None, reverse=False, order=None, trace=False):
    """n_iter steps from the uniform rows and eta0 (or up to max_iter with the stop test max(|gamma' - gamma|, |eta' - eta|) < tol): a dict
    of gamma, eta, loglik [S], loglik0 [S], deviance [S], iters, converged, dead_rows, lr_eta -- and, with trace, ll_trace = sum_s L
    before every step and at the end.  A cell with reads and p = 0 in any pass: the documented dead call."""
    counts = np.asarray(counts, dtype=np.int64)
    eta0 = np.asarray(eta0, dtype=np.float64)
    S, G = counts.shape[1], np.asarray(tau).shape[1]
    steps = n_iter if n_iter is not None else max_iter
    T = onehot(tau)
    gamma, eta = np.full((S, G), 1.0 / G), eta0.copy()
    out = dict(iters=0, converged=0, dead_rows=0)
    fit0 = R.fit_samples(counts, tau, eta0, n_iter=n_iter, tol=tol, max_iter=max_iter)
    out["loglik0"] = fit0["loglik"]
    lls, dead = [], False
    for _ in range(steps):
        if trace:
            lls.append(loglik(counts, tau, gamma, eta).sum())
        gamma_new, eta_new, delta, rows, bad = step(counts, T, gamma, eta, reverse, order)
        if bad:
            dead = True
            break
        gamma, eta = gamma_new, eta_new
        out["iters"] += 1
        out["dead_rows"] |= rows
        if tol > 0 and delta < tol:
            out["converged"] = 1
            break
    L = loglik(counts, tau, gamma, eta)
    if dead or np.isneginf(L).any():
        out.update(gamma=np.zeros((S, G)), eta=eta0.copy(), loglik=np.full(S, -np.inf), deviance=np.full(S, np.inf), converged=0,
                   lr_eta=np.nan, ll_trace=lls + [-np.inf])
        return out
    sat = np.array([R.saturated(counts[:, s]) for s in range(S)])
    out.update(gamma=gamma, eta=eta, loglik=L, deviance=2.0 * (sat - L), lr_eta=max(0.0, 2.0 * (L.sum() - out["loglik0"].sum())),
               ll_trace=lls + [L.sum()])
    return out


def synth(V, S, G, eta, depth=20, seed=0, zero_frac=0.0):
    """(counts [V,S,4], tau [V,G], gamma_true [S,G]) as _abund_ref.synth, with reads drawn under the given eta"""
    rs = np.random.RandomState(seed)
    tau = rs.randint(0, 4, size=(V, G))
    if V >= 2 * G:
        for g in range(G):                                                # haplotype g differs from every other one at position g
            tau[g, :] = rs.randint(0, 4)
            tau[g, g] = (tau[g, g] + 1 + rs.randint(0, 3)) % 4
    gamma = rs.dirichlet(np.full(G, 4.0), size=S)
    p = np.einsum("sg,vgb->vsb", gamma, np.asarray(eta)[tau])
    n = rs.poisson(depth, size=(V, S))
    counts = np.zeros((V, S, 4), dtype=np.int64)
    for v in range(V):
        for s in range(S):
            counts[v, s] = rs.multinomial(n[v, s], p[v, s] / p[v, s].sum())
    if zero_frac > 0:
        counts[rs.random_sample(counts.shape) < zero_frac] = 0
    return counts, tau, gamma


def random_eta(seed, lo=0.01, hi=0.05):
    """an error matrix whose rows carry between lo and hi of off-diagonal mass, spread unevenly"""
    rs = np.random.RandomState(seed)
    eta = np.zeros((4, 4))
    for a in range(4):
        off = rs.uniform(lo, hi) * rs.dirichlet(np.ones(3))
        eta[a, [b for b in range(4) if b != a]] = off
        eta[a, a] = 1.0 - off.sum()
    return eta


def diag_eta(d=0.99):
    return (d - (1.0 - d) / 3.0) * np.eye(4) + (1.0 - d) / 3.0
