"""What the fixed-tau tests share (tests/test_gpu_fixed_tau.py, tests/test_fixed_tau_cpu.py): the loop restated from the oracle's
pieces, the exact moments of the mu/E sums, and the inequalities both files check -- on the CPU for the restatement first, so that the
seeds the GPU tests use are known to pass for the reference."""
import numpy as np

from desman_amd.fixed_tau import pool_by_tau_word, summarize, words_to_digits
from oracle import cbind

LAW_SHAPE, LAW_DEPTH, LAW_N, LAW_SEED = (300, 4, 3), 30, 400, 0x51A7F1C5
POST_SHAPE, POST_DEPTH, POST_N, POST_BURN, POST_SEED = (300, 4, 3), 50, 600, 100, 0x0BADC0FFEE123457


def stats(spec, tau_idx, gamma, eta, counts, cseed, it):
    args = (np.ascontiguousarray(tau_idx, dtype=np.uint8), np.ascontiguousarray(gamma), np.ascontiguousarray(eta),
            np.ascontiguousarray(counts, dtype=np.int64), cseed, it)
    return cbind.stats_agg(*args, spec=spec) if spec >= 2 else cbind.stats_counter(*args)


def ref_chain(tau_idx, gamma0, eta0, counts, cseed, it0, n_iter, spec, fix_eta, want_ll=True):
    """dsm_ctx_gibbs_update_fixed_tau(pool = 0) from the oracle's pieces: per iteration the mu/E sums at (tau, gamma, eta) with counter
    it0 + k, the Dirichlet draws from them, ll / lp of the new state (eta held under fix_eta)"""
    tau_idx = np.ascontiguousarray(tau_idx, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    g, e = np.ascontiguousarray(gamma0), np.ascontiguousarray(eta0)
    out = dict(gamma=[], eta=[], ll=[], lp=[])
    for k in range(n_iter):
        mu, E = stats(spec, tau_idx, g, e, counts, cseed, it0 + k)
        g, e_new, _ = cbind.dirichlet_counter(mu, E, cseed, it0 + k)
        if not fix_eta:
            e = e_new
        out["gamma"].append(g); out["eta"].append(e)
        if want_ll:
            out["ll"].append(cbind.loglik(tau_idx, g, e, counts)); out["lp"].append(cbind.logpost(tau_idx, g, e, counts))
    return {k: np.array(v) for k, v in out.items()}


def pooled_table(tau_idx, counts):
    """(digits [W,G] uint8, pooled counts [W,S,4] int64) of the numpy pooling"""
    words, _, pooled = pool_by_tau_word(tau_idx, counts)
    return np.ascontiguousarray(words_to_digits(words, np.shape(tau_idx)[1]).astype(np.uint8)), np.ascontiguousarray(pooled)


def sum_moments(tau_idx, gamma, eta, counts):
    """exact mean and variance of sum_mu [S,G] and Esum [4,4] = [observed][true] at a fixed state: a read of base b at (v, s) goes to
    haplotype g with probability q = gamma_sg eta[tau_vg, b] / p_vsb, so each sum is a sum of independent binomial counts"""
    tau_idx = np.asarray(tau_idx).astype(np.int64)
    x = np.asarray(counts, dtype=np.float64)                                   # [V,S,4]
    w = gamma[None, :, :, None] * eta[tau_idx][:, None, :, :]                   # [V,S,G,b]
    p = w.sum(axis=2, keepdims=True)
    q = np.where(p > 0, w / np.where(p > 0, p, 1.0), 0.0)
    xe = x[:, :, None, :]
    e_mu, v_mu = (xe * q).sum(axis=(0, 3)), (xe * q * (1 - q)).sum(axis=(0, 3))
    e_E, v_E = np.zeros((4, 4)), np.zeros((4, 4))
    for a in range(4):
        r = (q * (tau_idx == a)[:, None, :, None]).sum(axis=2)                 # [V,S,b]: the read's true base is a
        e_E[:, a], v_E[:, a] = (x * r).sum(axis=(0, 1)), (x * r * (1 - r)).sum(axis=(0, 1))
    return e_mu, v_mu, e_E, v_E


def law_case():
    """(counts, tau digits, gamma, eta) of the law test: 300 x 4 x 3 at depth 30"""
    V, S, G = LAW_SHAPE
    rng = np.random.default_rng(77)
    tau = rng.integers(0, 4, size=(V, G)).astype(np.uint8)
    gamma = np.ascontiguousarray(rng.dirichlet(np.ones(G), size=S))
    eta = 0.94 * np.eye(4) + 0.015
    p = np.einsum("sg,vgb->vsb", gamma, eta[tau])
    counts = rng.multinomial(LAW_DEPTH, p).astype(np.int64)
    return np.ascontiguousarray(counts), tau, gamma, np.ascontiguousarray(eta)


def law_violations(mus, Es, moments):
    """components of the means of n draws of (sum_mu, Esum) further than 5 standard errors from their exact expectation"""
    e_mu, v_mu, e_E, v_E = moments
    n = len(mus)
    bad = []
    for name, draws, e, v in (("sum_mu", np.asarray(mus, dtype=np.float64), e_mu, v_mu), ("Esum", np.asarray(Es, dtype=np.float64), e_E, v_E)):
        m, se = draws.mean(axis=0), np.sqrt(v / n)
        z = np.abs(m - e) / np.where(se > 0, se, 1.0)
        print("%s: largest |mean - expectation| = %.2f standard errors" % (name, np.where(se > 0, z, 0.0).max()))
        for idx in zip(*np.nonzero(np.where(se > 0, z > 5.0, m != e))):
            bad.append((name, idx, m[idx], e[idx], se[idx]))
    return bad


def posterior_case():
    """(counts, tau digits, eta) of the end-to-end test: 300 x 4 x 3 at depth 50 (15 000 reads per sample) from a generating tau and eta,
    abundances ~ Dir(4): inside the simplex.  (A haplotype near absence mixes slowly under alpha = 0.1 -- the restated chain's draws of
    an abundance generated at 0.001 have autocorrelation 0.77 at lag 5 -- so a standard error from every fifth draw, which test 5
    prescribes, does not describe it; the comparison of two chains' means needs components whose thinned draws are close to independent.)"""
    V, S, G = POST_SHAPE
    rng = np.random.default_rng(2024)
    tau = rng.integers(0, 4, size=(V, G)).astype(np.int64)
    gamma = rng.dirichlet(np.full(G, 4.0), size=S)
    eta = 0.96 * np.eye(4) + 0.01
    p = np.einsum("sg,vgb->vsb", gamma, eta[tau])
    counts = rng.multinomial(POST_DEPTH, p).astype(np.int64)
    return np.ascontiguousarray(counts), tau, np.ascontiguousarray(eta)


def mc_se(draws, thin=5):
    """Monte-Carlo standard error of the mean of a chain's draws [n, ...] from every thin-th draw (successive draws of a Gibbs chain are
    correlated; thinned ones much less)"""
    d = np.asarray(draws)[::thin]
    return d.std(axis=0, ddof=1) / np.sqrt(d.shape[0])


def posterior_violations(post, ml_gamma):
    """what test 5 asks of one posterior: the mean within 5 posterior sd of the ML estimate wherever that exceeds 0.05, ordered
    quantiles, mean rows summing to 1"""
    bad = []
    big = ml_gamma > 0.05
    z = np.abs(post["mean"] - ml_gamma) / post["sd"]
    print("largest |posterior mean - ML| = %.2f posterior sd over %d abundances above 0.05" % (z[big].max(), int(big.sum())))
    if (z[big] > 5.0).any():
        bad.append("mean further than 5 sd from the ML estimate")
    if not ((post["lo"] <= post["med"]) & (post["med"] <= post["hi"])).all():
        bad.append("quantiles out of order")
    if np.abs(post["mean"].sum(axis=1) - 1.0).max() > 1e-12:
        bad.append("mean rows do not sum to 1")
    return bad


def means_disagree(a, b):
    """components in which two chains' posterior means differ by more than 5 Monte-Carlo standard errors of the difference (mc_se)"""
    se = np.sqrt(mc_se(a["draws"]) ** 2 + mc_se(b["draws"]) ** 2)
    z = np.abs(a["mean"] - b["mean"]) / se
    print("pool 0 vs 1: largest difference of the means = %.2f Monte-Carlo standard errors" % z.max())
    return z > 5.0


