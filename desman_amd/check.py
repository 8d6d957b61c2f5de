"""Posterior predictive fit of a chain per sample and per position: does the model explain the table it was run on?
Pure numpy; the same code serves the tests and the product.  The device makes the sums (_lib.Context.trace_fit_stats); this module
restates a cell's terms and turns the sums into scores.

For a stored iteration and a cell (v, s) with counts n_b over the four bases, N = sum_b n_b > 0, and the likelihood's own

    p_b = sum_g gamma[s][g] eta[tau[v][g]][b]                  k = #{b : p_b > 0}

    X = sum_{b: p_b > 0} (n_b - N p_b)^2 / (N p_b)             Pearson's discrepancy
    D = 2 sum_{b: n_b > 0} n_b ln(n_b / (N p_b))               the deviance against the saturated model
    E = k - 1                                                  the exact mean of X under multinomial(N, p)
    W = 2 (k - 1) + (sum_{b: p_b > 0} 1 / p_b - k^2 - 2 k + 2) / N       its exact variance

A base with p_b = 0 < n_b makes X and D of the cell +inf, one with p_b = 0 = n_b adds exactly 0, an empty cell adds nothing anywhere,
and nothing is ever NaN.  The standardised discrepancy of a sample or a position is z = (mean X - mean E) / sqrt(mean W), the means
taken over the stored iterations of the sums over the other index.  At fitted parameters X sits a little below E -- by about the
share of fitted parameters per cell -- so z is conservative: a score, not a p-value.
"""
import numpy as np

Z_HIGH = 3.0          # the threshold of the one summary line `desman --check` logs: a convention, not tuned


def cell_terms(counts, tau_digits, gamma, eta):
    """X, D, E, W [V, S] of one iteration -- counts [V, S, 4], tau_digits [V, G] (0..3), gamma [S, G], eta [4, 4] ([true][observed]) --
    and absX, absD: the sums of the absolute values of the terms that enter X and D (D's terms cancel), which the tolerance of a
    comparison goes by.  Every sum runs in the order of the device's (kernels_fit.hip): g ascending into the four mixture weights, then
    the true bases, then the observed bases."""
    n = np.asarray(counts, dtype=np.float64)
    d = np.asarray(tau_digits, dtype=np.int64)
    gamma, eta = np.asarray(gamma, dtype=np.float64), np.asarray(eta, dtype=np.float64).reshape(4, 4)
    V, S = n.shape[0], n.shape[1]
    m = np.zeros((4, V, S))
    for g in range(d.shape[1]):
        for a in range(4):
            m[a] += np.where((d[:, g] == a)[:, None], gamma[None, :, g], 0.0)
    N = n.sum(axis=2)
    live = N > 0
    X, dv, absX, absD, rs = (np.zeros((V, S)) for _ in range(5))
    k = np.zeros((V, S), dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(4):
            p = ((m[0] * eta[0, b] + m[1] * eta[1, b]) + m[2] * eta[2, b]) + m[3] * eta[3, b]
            nb = n[:, :, b]
            pos, seen = p > 0, nb > 0
            e = N * p
            dl = nb - e
            xb = np.where(pos, dl * dl / e, np.where(seen, np.inf, 0.0))
            db = np.where(seen, np.where(pos, nb * np.log(nb / e), np.inf), 0.0)
            X += xb
            dv += db
            absX += np.abs(xb)
            absD += np.abs(db)
            rs += np.where(pos, 1.0 / p, 0.0)
            k += pos
        W = 2.0 * (k - 1.0) + (rs - (k * k + 2 * k - 2.0)) / N
    zero = np.zeros((V, S))
    pick = lambda x: np.where(live, x, zero)
    return dict(X=pick(X), D=pick(2.0 * dv), E=pick(k - 1.0), W=pick(W), absX=pick(absX), absD=pick(2.0 * absD))


def trace_sums(counts, tau_digits, gamma, eta):
    """what trace_fit_stats returns for the iterations given -- tau_digits [n, V, G] (or [V, G]: one tau for all), gamma [n, S, G],
    eta [n, 4, 4] -- by cell_terms: sample [S, 4], position [V, 4], cell [V, S], and abs_sample / abs_position / abs_cell, the sums of
    the absolute values of the terms behind every element (for D those of n_b ln(n_b / (N p_b)), which cancel)"""
    counts = np.asarray(counts)
    V, S = counts.shape[0], counts.shape[1]
    tau_digits = np.asarray(tau_digits)
    n = np.asarray(gamma).shape[0]
    out = dict(sample=np.zeros((S, 4)), position=np.zeros((V, 4)), cell=np.zeros((V, S)),
               abs_sample=np.zeros((S, 4)), abs_position=np.zeros((V, 4)), abs_cell=np.zeros((V, S)), n_it=n)
    for t in range(n):
        c = cell_terms(counts, tau_digits if tau_digits.ndim == 2 else tau_digits[t], gamma[t], eta[t])
        for q, (key, mag) in enumerate((("X", "absX"), ("D", "absD"), ("E", "E"), ("W", "W"))):
            out["sample"][:, q] += c[key].sum(axis=0)
            out["position"][:, q] += c[key].sum(axis=1)
            out["abs_sample"][:, q] += np.abs(c[mag]).sum(axis=0)
            out["abs_position"][:, q] += np.abs(c[mag]).sum(axis=1)
        out["cell"] += c["X"]
        out["abs_cell"] += c["absX"]
    return out


def _scores(sums, n_it, cells):
    sums = np.asarray(sums, dtype=np.float64)
    if n_it < 1:
        nan = np.full(sums.shape[0], np.nan)
        return dict(cells=cells, X2=nan, deviance=nan.copy(), expected=nan.copy(), variance=nan.copy(), z=nan.copy())
    x, d, e, w = (sums[:, q] / float(n_it) for q in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(w > 0, (x - e) / np.sqrt(w), 0.0)        # (no non-empty cell: nothing to score)
    return dict(cells=cells, X2=x, deviance=d, expected=e, variance=w, z=z)


def fit_scores(sums, n_it, counts):
    """From a trace_fit_stats result (sample [S, 4], position [V, 4], optionally cell [V, S]) over n_it iterations and the counts
    [V, S, 4]: dict of ``sample`` and ``position``, each a dict of cells (the non-empty cells of the row, from the counts), X2,
    expected, variance, deviance (per-iteration means of the sums) and z = (X2 - expected) / sqrt(variance) (0 for a row without a
    non-empty cell, +inf where X2 is), and -- where the sums hold it -- ``cell`` [V, S], the posterior mean of X per cell."""
    full = np.asarray(counts).sum(axis=2) > 0
    out = {}
    if sums.get("sample") is not None:
        out["sample"] = _scores(sums["sample"], n_it, full.sum(axis=0))
    if sums.get("position") is not None:
        out["position"] = _scores(sums["position"], n_it, full.sum(axis=1))
    if sums.get("cell") is not None:
        out["cell"] = np.asarray(sums["cell"], dtype=np.float64) / float(n_it) if n_it >= 1 else np.full(full.shape, np.nan)
    return out


def flagged(scores):
    """the number of rows of a fit_scores table with z > Z_HIGH"""
    return int((scores["z"] > Z_HIGH).sum())


# ---- posterior predictive p-values from replicate tables (_lib.Context.trace_ppc)
REPS = 20             # replicates per used iteration of a bare `--check-reps`: a convention, not tuned
N_USE = 50            # about this many evenly spaced stored iterations are used unless --check-stride says otherwise (as --predictive)
P_LOW = 0.01          # the thresholds of the one summary line `desman --check --check-reps` logs: conventions
Q_LOW = 0.1
PPP_COLUMNS = ("T_obs", "T_rep", "T_rep_sd", "p", "p_mcse")


def default_stride(n_stored, n_use=N_USE):
    """the stride that uses about n_use of n_stored iterations"""
    return max(1, int(n_stored) // int(n_use))


def bh_qvalues(p):
    """Benjamini-Hochberg q-values of the p-values p [n]: q_(i) = min over j >= i of n p_(j) / j in ascending order of p, at most 1;
    NaN stays NaN and does not count"""
    p = np.asarray(p, dtype=np.float64)
    q = np.full(p.shape, np.nan)
    ok = np.flatnonzero(~np.isnan(p))
    n = ok.size
    if n == 0:
        return q
    order = ok[np.argsort(p[ok], kind="stable")]
    scaled = p[order] * n / np.arange(1, n + 1)
    q[order] = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    return q


def ppp_batches(n_stored, stride):
    """The used iterations 0, stride, ... below n_stored cut for the batch-means error of a p-value (diagnose.batch_range over the used
    iterations, L = floor(sqrt(n_used))): a list of (it0, n_it, counts) -- one trace_ppc call each, `counts` false for the iterations before
    the first batch -- and B.  The calls together use every used iteration once."""
    from . import diagnose
    n_used = -(-int(n_stored) // int(stride)) if n_stored > 0 else 0
    L = diagnose.default_batch_len(n_used)
    B, N, skip = diagnose.batch_range(n_used, L)
    calls = []
    if skip > 0:
        calls.append((0, min(n_stored, skip * stride), False))
    for b in range(B):
        k0 = skip + b * L
        calls.append((k0 * stride, min(n_stored - k0 * stride, L * stride), True))
    return calls, B


def ppp_table(parts, kind):
    """From the trace_ppc results of the calls of ppp_batches, ``parts`` = [(result, counts)], for kind = "sample" or "position": dict of
    T_obs, T_rep (means over t and over (t, r)), T_rep_sd, p = ge / (n_used R) and p_mcse (the standard error of the mean of the B batch
    p-values; NaN below two batches)"""
    n = sum(r["n_used"] * r["R"] for r, _ in parts)
    n_t = sum(r["n_used"] for r, _ in parts)
    ge = sum(np.asarray(r["ge_" + kind], dtype=np.float64) for r, _ in parts)
    rep = sum(np.asarray(r["rep_" + kind], dtype=np.float64) for r, _ in parts)
    obs = sum(np.asarray(r["obs_" + kind], dtype=np.float64) for r, _ in parts)
    if n < 1:
        nan = np.full(ge.shape, np.nan)
        return dict(T_obs=nan, T_rep=nan.copy(), T_rep_sd=nan.copy(), p=nan.copy(), p_mcse=nan.copy())
    mean = rep[:, 0] / n
    with np.errstate(invalid="ignore"):
        sd = np.sqrt(np.maximum(rep[:, 1] / n - mean * mean, 0.0))
    bp = np.array([np.asarray(r["ge_" + kind], dtype=np.float64) / (r["n_used"] * r["R"]) for r, c in parts if c and r["n_used"] > 0])
    mcse = bp.std(axis=0, ddof=1) / np.sqrt(bp.shape[0]) if bp.shape[0] >= 2 else np.full(ge.shape, np.nan)
    return dict(T_obs=obs / n_t, T_rep=mean, T_rep_sd=sd, p=ge / n, p_mcse=mcse)


def ppp_summary(samples, positions):
    """what the one log line of `desman --check --check-reps` says: the samples and positions with p < P_LOW against the number a
    well-specified model expects at most (P_LOW times their number: posterior predictive p-values are conservative), and the positions
    with q < Q_LOW"""
    return dict(samples_low=int((samples["p"] < P_LOW).sum()), samples=len(samples["p"]), samples_expected=P_LOW * len(samples["p"]),
                positions_low=int((positions["p"] < P_LOW).sum()), positions=len(positions["p"]),
                positions_expected=P_LOW * len(positions["p"]), positions_q=int((positions["q"] < Q_LOW).sum()))
