"""The chain with the haplotypes held (dsm_ctx_gibbs_update_fixed_tau): the posterior of the abundances -- and,
on request, of the error matrix -- of given samples under the chain's own Dirichlet priors, and the numpy restatement of the pooling
by tau word the library does on the device.
"""
import numpy as np

POSTERIOR_SEED = 0x8C1F3A5D7E9B2468       # stream key of posterior_gamma when the caller names none: a call is reproducible


def tau_words(tau):
    """packed words [V] uint64 of tau ([V,G] digits or [V,G,4] one-hot): digit of haplotype g in bits 2g, 2g + 1 (G <= 32)"""
    t = np.asarray(tau)
    if t.ndim == 3 and t.shape[2] == 4:
        t = np.argmax(t == 1, axis=2)
    t = t.astype(np.uint64)
    shift = (2 * np.arange(t.shape[1])).astype(np.uint64)
    return np.bitwise_or.reduce(t << shift[None, :], axis=1) if t.shape[1] else np.zeros(t.shape[0], dtype=np.uint64)


def pool_by_tau_word(tau, counts):
    """(words [W] uint64 ascending, row [V] of each position's word, pooled [W,S,4] int64): the counts of all positions that carry one
    tau word, added.  Cells of one word have the same base probabilities, so the pooled table has the likelihood of the original in
    (gamma, eta) up to the constant of the multinomial coefficients."""
    counts = np.asarray(counts)
    words, row = np.unique(tau_words(tau), return_inverse=True)
    row = np.asarray(row).reshape(-1)
    pooled = np.zeros((len(words),) + counts.shape[1:], dtype=np.int64)
    np.add.at(pooled, row, counts)
    return words, row.astype(np.int32), pooled


def words_to_digits(words, G):
    """[W,G] int64 digits of packed words"""
    w = np.asarray(words, dtype=np.uint64)
    shift = (2 * np.arange(G)).astype(np.uint64)
    return ((w[:, None] >> shift[None, :]) & np.uint64(3)).astype(np.int64)


def summarize(draws, level=0.95):
    """posterior summary of kept draws [n, ...]: dict of mean, sd (n - 1 in the denominator), lo / med / hi = the quantiles
    (1 - level) / 2, 0.5 and 1 - (1 - level) / 2, and the draws themselves"""
    d = np.asarray(draws, dtype=np.float64)
    if d.shape[0] < 1:
        raise ValueError("summarize: no draws kept")
    if not 0.0 < level < 1.0:
        raise ValueError("summarize: level must lie between 0 and 1")
    a = 0.5 * (1.0 - level)
    lo, med, hi = np.quantile(d, [a, 0.5, 1.0 - a], axis=0)
    sd = d.std(axis=0, ddof=1) if d.shape[0] > 1 else np.zeros(d.shape[1:])
    return dict(mean=d.mean(axis=0), sd=sd, lo=lo, med=med, hi=hi, draws=d)


def posterior_gamma(counts, tau, eta, n_iter=1000, burn=200, fix_eta=True, level=0.95, seed=POSTERIOR_SEED, pool=-1,
                    alpha=0.1, delta=0.1, epsilon=1.0e-6, device=0):
    """Posterior of the abundances of the haplotypes ``tau`` ([V,G] digits or [V,G,4] one-hot) in the samples of ``counts`` [V,S,4]
    under gamma_s ~ Dir(alpha), with tau held and eta [4,4] held (fix_eta) or sampled under eta_a ~ Dir(delta) from ``eta`` as the
    start: n_iter iterations of the fixed-tau chain from uniform abundance rows, stream key ``seed``, the first ``burn`` dropped.
    Returns summarize() of the kept gamma draws ([n_iter - burn, S, G]) plus ll (kept iterations), lp_star and -- with fix_eta=False -- eta_mean,
    eta_sd [4,4] and eta_draws."""
    from . import _lib
    x = np.ascontiguousarray(counts, dtype=np.int64)
    if x.ndim != 3 or x.shape[2] != 4:
        raise ValueError("posterior_gamma: counts must be [V,S,4]")
    n_iter, burn = int(n_iter), int(burn)
    if n_iter < 1 or burn < 0 or burn >= n_iter:
        raise ValueError("posterior_gamma: need n_iter >= 1 and 0 <= burn < n_iter")
    V, S = x.shape[0], x.shape[1]
    t = _lib._fit_tau(tau, V)
    G = t.shape[1]
    onehot = np.zeros((V, G, 4), dtype=np.int64)
    np.put_along_axis(onehot, t[..., None], 1, axis=2)
    ctx = _lib.Context(device)
    try:
        ctx.set_counts(x)
        ctx.set_priors(alpha, delta, epsilon)
        ctx.set_state(onehot, np.full((S, G), 1.0 / G), _lib._fit_eta(eta))
        ctx.seed(1, ctr_seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        ctx.gibbs_update_fixed_tau(n_iter, fix_eta=fix_eta, pool=pool)
        tr = ctx.get_trace()
        lp_star = float(ctx.get_star()["lp"])
    finally:
        ctx.close()
    res = summarize(tr["gamma"][burn:], level)
    res["ll"] = tr["ll"][burn:]
    res["lp_star"] = lp_star                              # lp of the MAP record over the whole chain (the entry state included)
    if not fix_eta:
        e = summarize(tr["eta"][burn:], level)
        res["eta_mean"], res["eta_sd"], res["eta_draws"] = e["mean"], e["sd"], e["draws"]
    return res
