"""The position-marginal predictive density straight from its definition, in numpy fp64 with np.log: for every used iteration t and
position v all 4^G joint haplotype states are enumerated,

    L_t(state) = sum_{s, b: x > 0} x[v][s][b] ln sum_g gamma_t[s][g] eta_t[state_g][b],      logz[t][v] = ln sum_state exp L_t(state),

then lppd, mean and var over the iterations.  Shared by tests/test_predictive_cpu.py and tests/test_gpu_predictive.py."""
import numpy as np


def states(G):
    """[4^G, G] digits; haplotype 0 is the most significant digit of the state index"""
    idx = np.arange(4 ** G)
    return np.stack([(idx >> (2 * (G - 1 - g))) & 3 for g in range(G)], axis=1)


def logz_one(counts, gamma, eta):
    """logz [V] and labs [V] = max over the finite states of |L| (1 where there is none), for one (gamma [S, G], eta [4, 4])"""
    counts = np.asarray(counts, dtype=np.int64)
    gamma, eta = np.asarray(gamma, dtype=np.float64), np.asarray(eta, dtype=np.float64).reshape(4, 4)
    dg = states(gamma.shape[1])
    p = np.einsum("sg,kgb->ksb", gamma, eta[dg])                     # [K, S, 4]
    with np.errstate(divide="ignore"):
        lp = np.log(p)
    logz, labs = np.empty(counts.shape[0]), np.empty(counts.shape[0])
    for v, x in enumerate(counts):
        seen = x > 0                                                 # cells without reads are not evaluated: 0 ln 0 never arises
        L = (lp[:, seen] * x[seen].astype(np.float64)[None, :]).sum(axis=1)
        fin = np.isfinite(L)
        if not fin.any():
            logz[v], labs[v] = -np.inf, 1.0
            continue
        M = L[fin].max()
        logz[v] = M + np.log(np.exp(L[fin] - M).sum())
        labs[v] = max(1.0, np.abs(L[fin]).max())
    return logz, labs


def stats(logz_it):
    """lppd, mean, var [V] of a logz matrix [n, V]: -inf is zero mass in lppd, makes mean -inf and var +inf; var = 0 for n = 1"""
    z = np.asarray(logz_it, dtype=np.float64)
    n, V = z.shape
    lppd, mean, var = np.empty(V), np.empty(V), np.empty(V)
    for v in range(V):
        col = z[:, v]
        fin = np.isfinite(col)
        if fin.any():
            M = col[fin].max()
            lppd[v] = M + np.log(np.exp(col[fin] - M).sum() / n)
        else:
            lppd[v] = -np.inf
        if fin.all():
            mean[v] = col.mean()
            var[v] = ((col - mean[v]) ** 2).sum() / (n - 1) if n > 1 else 0.0
        else:
            mean[v], var[v] = -np.inf, np.inf
    return lppd, mean, var


def trace_predictive(counts, gamma, eta, it0=0, n_it=None, stride=1):
    """what Context.trace_predictive returns for gamma [n, S, G], eta [n, 4, 4] -- lppd, mean, var [V], logz_it [n_used, V], n_used --
    and labs [n_used, V], the magnitude the tolerance of a comparison goes by"""
    n_it = len(gamma) - it0 if n_it is None else n_it
    used = range(it0, it0 + n_it, stride)
    rows = [logz_one(counts, gamma[t], eta[t]) for t in used]
    logz_it = np.stack([r[0] for r in rows])
    lppd, mean, var = stats(logz_it)
    return dict(lppd=lppd, mean=mean, var=var, logz_it=logz_it, labs=np.stack([r[1] for r in rows]), n_used=len(used))
