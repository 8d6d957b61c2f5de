"""Plain numpy restatement of the abundance fit (include/desman_hip.h: dsm_fit_gamma) -- a helper of tests/test_abund_cpu.py and
tests/test_gpu_abund.py, not a test file.

One sample: x [V,4] counts, tau [V,G] digits, eta [4,4] ([true][observed]).
    L(gamma) = sum_{v,b: x > 0} x_vb ln p_vb,   p_vb = sum_g gamma_g eta[tau_vg][b]
    EM step:   gamma'_g = gamma_g / N  sum_{v,b: x > 0} x_vb eta[tau_vg][b] / p_vb
Written with the G-term sums per haplotype (E[v,g,b] = eta[tau_vg][b]) -- NOT with the class sums the kernel uses -- so that the two
share the model and nothing else."""
import numpy as np

# tables with an interior maximum (no duplicate haplotypes, depth >= 20), shared by the CPU and the GPU tests: V, G, depth, seed
INTERIOR = [(65, 3, 20, 11), (257, 8, 20, 12), (120, 5, 40, 13)]


def emission(tau, eta):
    """E[v,g,b] = eta[tau_vg][b]"""
    return np.asarray(eta, dtype=np.float64)[np.asarray(tau, dtype=np.int64)]


def start(G, mask=None):
    """uniform over the allowed haplotypes (mask = index of the excluded one)"""
    g = np.ones(G)
    if mask is not None:
        g[mask] = 0.0
    return g / g.sum()


def loglik(x, E, gamma):
    x = np.asarray(x, dtype=np.float64)
    p = np.einsum("g,vgb->vb", gamma, E)
    pos = x > 0
    if (p[pos] <= 0).any():
        return -np.inf
    return float((x[pos] * np.log(p[pos])).sum())


def saturated(x):
    """L_sat = sum x ln(x / n_v)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.sum(axis=1, keepdims=True) * np.ones_like(x)
    pos = x > 0
    return float((x[pos] * np.log(x[pos] / n[pos])).sum())


def em_step(x, E, gamma, reverse=False):
    x = np.asarray(x, dtype=np.float64)
    if reverse:                                       # the same sums over the positions in the opposite order
        x, E = x[::-1], E[::-1]
    p = np.einsum("g,vgb->vb", gamma, E)
    pos = x > 0
    q = np.zeros_like(x)
    q[pos] = x[pos] / p[pos]
    r = np.einsum("vgb,vb->g", E, q)
    return gamma * r / x.sum()


def fit(x, tau, eta, n_iter=None, mask=None, reverse=False, tol=0.0, max_iter=None, trace=False):
    """n_iter EM steps from the uniform start (or up to max_iter with the stop test max |gamma' - gamma| < tol): a dict of gamma,
    loglik (at gamma), deviance, iters, converged -- and, with trace, ll_trace = L before every step and at the end.
    N = 0: the start row, loglik 0.  A cell with reads and p = 0: gamma 0, loglik -inf, converged 0."""
    x = np.asarray(x, dtype=np.int64)
    E = emission(tau, eta)
    G = E.shape[1]
    gamma = start(G, mask)
    steps = n_iter if n_iter is not None else max_iter
    out = dict(iters=0, converged=0)
    lls = []
    if x.sum() == 0:
        return dict(gamma=gamma, loglik=0.0, deviance=0.0, iters=0, converged=1, ll_trace=[0.0])
    if loglik(x, E, gamma) == -np.inf:
        return dict(gamma=np.zeros(G), loglik=-np.inf, deviance=np.inf, iters=0, converged=0, ll_trace=[-np.inf])
    for _ in range(steps):
        if trace:
            lls.append(loglik(x, E, gamma))
        new = em_step(x, E, gamma, reverse)
        delta = np.abs(new - gamma).max()
        gamma = new
        out["iters"] += 1
        if tol > 0 and delta < tol:
            out["converged"] = 1
            break
    L = loglik(x, E, gamma)
    lls.append(L)
    out.update(gamma=gamma, loglik=L, deviance=2.0 * (saturated(x) - L), ll_trace=lls)
    return out


def fit_samples(counts, tau, eta, **kw):
    """fit() for every sample of counts [V,S,4]: dict of stacked arrays"""
    rows = [fit(counts[:, s, :], tau, eta, **kw) for s in range(counts.shape[1])]
    return dict(gamma=np.array([r["gamma"] for r in rows]), loglik=np.array([r["loglik"] for r in rows]),
                deviance=np.array([r["deviance"] for r in rows]), iters=np.array([r["iters"] for r in rows]),
                converged=np.array([r["converged"] for r in rows]))


def lr_absent(x, tau, eta, g, **kw):
    """2 (L(full fit) - L(fit with haplotype g excluded)), clamped at 0; G = 1: +inf"""
    G = np.asarray(tau).shape[1]
    full = fit(x, tau, eta, **kw)
    if G == 1:
        return np.inf
    return max(0.0, 2.0 * (full["loglik"] - fit(x, tau, eta, mask=g, **kw)["loglik"]))


def kkt_gradient(x, tau, eta, gamma):
    """grad_g = (1/N) sum_{v,b: x > 0} x_vb eta[tau_vg][b] / p_vb: 1 on the support of the maximiser, <= 1 off it"""
    x = np.asarray(x, dtype=np.float64)
    E = emission(tau, eta)
    p = np.einsum("g,vgb->vb", gamma, E)
    pos = x > 0
    q = np.zeros_like(x)
    q[pos] = x[pos] / p[pos]
    return np.einsum("vgb,vb->g", E, q) / x.sum()


def kkt_residual(x, tau, eta, gamma, floor=1e-12):
    """max over the support of |grad - 1|, and over the rest of max(grad - 1, 0)"""
    g = kkt_gradient(x, tau, eta, gamma)
    on = gamma > floor
    return max(np.abs(g[on] - 1.0).max() if on.any() else 0.0, np.maximum(g[~on] - 1.0, 0.0).max() if (~on).any() else 0.0)


def synth(V, S, G, depth=20, seed=0, zero_frac=0.0, distinct=True):
    """(counts [V,S,4], tau [V,G], eta, gamma_true [S,G]): multinomial reads of depth ~ Poisson(depth) per position under interior
    abundances (Dirichlet(4)); distinct: no two haplotypes agree everywhere (an interior, unique maximum where V allows)"""
    rs = np.random.RandomState(seed)
    tau = rs.randint(0, 4, size=(V, G))
    if distinct and V >= 2 * G:
        for g in range(G):                              # haplotype g differs from every other one at position g
            tau[g, :] = rs.randint(0, 4)
            tau[g, g] = (tau[g, g] + 1 + rs.randint(0, 3)) % 4
    eta = 0.96 * np.eye(4) + 0.01
    gamma = rs.dirichlet(np.full(G, 4.0), size=S)
    p = np.einsum("sg,vgb->vsb", gamma, eta[tau])
    counts = np.zeros((V, S, 4), dtype=np.int64)
    n = rs.poisson(depth, size=(V, S))
    for v in range(V):
        for s in range(S):
            counts[v, s] = rs.multinomial(n[v, s], p[v, s] / p[v, s].sum())
    if zero_frac > 0:
        counts[rs.random_sample(counts.shape) < zero_frac] = 0
    return counts, tau, eta, gamma
