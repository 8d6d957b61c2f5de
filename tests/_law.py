"""Shared helpers of the law (T1) tests: chi-square of draws against an exact pmf, two-sample chi-square of two sets of
draws, and the cases on which the counter-based mu/E samplers are compared with the reference's own sampleMu
(/root/reference/desman/HaploSNP_Sampler.py:284-309, restated RandomState-exactly in oracle/ref_numpy.py: sample_mu and pinned
there by the golden fixtures of tests/test_oracle_golden.py); and the exact joint law of the gamma / eta Dirichlet draws
(stick-breaking), with the cases both the specification (tests/test_law_cpu.py) and the device draw (tests/test_gpu_dirichlet.py) are
held to."""
import functools

import numpy as np
from scipy import stats as st


def chi2_vs_binom(draws, n, p, nbins=40, min_expected=50.0):
    """p-value of `draws` (integers) against Binomial(n, p): bins cut at the exact quantiles (so the test works for any n),
    merged until every bin expects >= min_expected draws."""
    draws = np.asarray(draws, dtype=np.int64)
    N = draws.size
    nbins = int(max(2, min(nbins, N / (2.0 * min_expected))))
    qs = np.unique(st.binom.ppf(np.linspace(0.0, 1.0, nbins + 1)[1:-1], n, p)).astype(np.int64)   # upper edges (inclusive)
    edges = np.concatenate(([-1], qs, [n]))
    edges = np.unique(edges)
    cdf = st.binom.cdf(edges, n, p)
    cdf[0], cdf[-1] = 0.0, 1.0
    exp = np.diff(cdf) * N
    obs = np.histogram(draws, bins=edges.astype(np.float64) + 0.5)[0].astype(np.float64)
    assert obs.sum() == N, "draws outside 0..n"
    # merge small bins from the left
    e2, o2, ea, oa = [], [], 0.0, 0.0
    for e, o in zip(exp, obs):
        ea += e; oa += o
        if ea >= min_expected:
            e2.append(ea); o2.append(oa); ea, oa = 0.0, 0.0
    if ea > 0.0:
        if e2:
            e2[-1] += ea; o2[-1] += oa
        else:
            e2.append(ea); o2.append(oa)
    e2, o2 = np.array(e2), np.array(o2)
    if e2.size < 2:
        return 1.0 if o2[0] == N else 0.0
    stat = ((o2 - e2) ** 2 / e2).sum()
    return float(st.chi2.sf(stat, e2.size - 1))


def chi2_vs_pmf(draws, pmf, min_expected=50.0):
    """p-value of integer `draws` against the explicit pmf over 0..len(pmf)-1 (bins merged to >= min_expected)."""
    draws = np.asarray(draws, dtype=np.int64)
    N = draws.size
    assert draws.min() >= 0 and draws.max() < len(pmf)
    obs = np.bincount(draws, minlength=len(pmf)).astype(np.float64)
    exp = np.asarray(pmf, dtype=np.float64) * N
    e2, o2, ea, oa = [], [], 0.0, 0.0
    for e, o in zip(exp, obs):
        ea += e; oa += o
        if ea >= min_expected:
            e2.append(ea); o2.append(oa); ea, oa = 0.0, 0.0
    if e2:
        e2[-1] += ea; o2[-1] += oa
    else:
        e2.append(ea); o2.append(oa)
    e2, o2 = np.array(e2), np.array(o2)
    e2 *= N / e2.sum()                      # a truncated pmf tail
    if e2.size < 2:
        return 1.0
    return float(st.chi2.sf(((o2 - e2) ** 2 / e2).sum(), e2.size - 1))


def chi2_two_sample(a, b, nbins=10):
    """p-value of the hypothesis that integer samples a and b come from one distribution (pooled-quantile bins)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    pooled = np.concatenate((a, b))
    edges = np.unique(np.quantile(pooled, np.linspace(0, 1, nbins + 1)[1:-1]))
    ca = np.bincount(np.searchsorted(edges, a, side="left"), minlength=edges.size + 1).astype(np.float64)
    cb = np.bincount(np.searchsorted(edges, b, side="left"), minlength=edges.size + 1).astype(np.float64)
    keep = (ca + cb) > 0
    ca, cb = ca[keep], cb[keep]
    if ca.size < 2:
        return 1.0
    na, nb = ca.sum(), cb.sum()
    ea, eb = (ca + cb) * na / (na + nb), (ca + cb) * nb / (na + nb)
    stat = ((ca - ea) ** 2 / ea).sum() + ((cb - eb) ** 2 / eb).sum()
    return float(st.chi2.sf(stat, ca.size - 1))


def sum_of_binomials_pmf(ns, ps):
    """exact pmf of a sum of independent Binomial(n_i, p_i)"""
    pmf = np.array([1.0])
    for n, p in zip(ns, ps):
        if n == 0 or p <= 0.0:
            continue
        pmf = np.convolve(pmf, st.binom.pmf(np.arange(int(n) + 1), int(n), float(p)))
    return pmf


# ---- cases for "spec = reference in law" ------------------------------------------------------------------------------
# name -> (V, S, G, depth_scale, kind of state)
LAW_CASES = {
    "G3": (30, 6, 3, 1.0, "random"),                    # the shape the first law test used
    "G10": (16, 3, 10, 1.0, "random"),                  # stage 2 as its own launch (G >= 10)
    "G12": (12, 2, 12, 1.0, "random"),
    "deep": (20, 4, 4, 15.0, "random"),                 # x 15 depth: BTRS in stage 1, deferred lists, stats_big_kernel
    "converged": (40, 4, 4, 4.0, "truth"),              # eta ~ 0.97 I, tau = the generating haplotypes: rare-outcome inversion
    "words": (80, 4, 2, 3.0, "truth"),                  # 80 positions on at most 16 tau words: what spec 4 pools (5 positions a word)
}


def law_case(name):
    """(counts, tau one-hot, gamma, eta) of a case"""
    from desman_amd.synth import synth_counts, random_state
    from oracle import cbind
    V, S, G, depth, kind = LAW_CASES[name]
    seed = 4000 + sorted(LAW_CASES).index(name)
    counts, tau_true, gamma_true = synth_counts(V, S, G, seed=seed, depth_scale=depth)
    if kind == "truth":
        tau = cbind.idx_to_onehot(tau_true)
        gamma = np.ascontiguousarray(gamma_true)
        eta = 0.96 * np.eye(4) + 0.01
    else:
        tau, gamma, eta = random_state(V, S, G, seed=seed + 1)
    return counts, tau, gamma, eta


@functools.lru_cache(maxsize=None)
def reference_draws(name, n):
    """n draws of (sum_mu [S,G], Esum [4,4] = [observed][true]) by the reference's sampleMu"""
    from oracle import ref_numpy as rn
    counts, tau, gamma, eta = law_case(name)
    rs = np.random.RandomState(777)
    mus, es = [], []
    for _ in range(n):
        E, mu = rn.sample_mu(rs, tau, gamma, eta, counts)
        mus.append(mu.sum(axis=(0, 2)))
        es.append(E.sum(axis=(0, 1)))
    return np.array(mus), np.array(es)


def assert_same_law(mu_a, E_a, mu_b, E_b, what):
    """per-(s,g) marginals of sum_mu and the 16 entries of Esum: two-sample chi-square (Bonferroni over all of them),
    means by z-test, variances within Monte-Carlo error"""
    mu_a, mu_b = np.asarray(mu_a, dtype=np.float64), np.asarray(mu_b, dtype=np.float64)
    E_a, E_b = np.asarray(E_a, dtype=np.float64), np.asarray(E_b, dtype=np.float64)
    cols_a = np.concatenate((mu_a.reshape(len(mu_a), -1), E_a.reshape(len(E_a), -1)), axis=1)
    cols_b = np.concatenate((mu_b.reshape(len(mu_b), -1), E_b.reshape(len(E_b), -1)), axis=1)
    ps = []
    for j in range(cols_a.shape[1]):
        a, b = cols_a[:, j], cols_b[:, j]
        if a.std() == 0.0 and b.std() == 0.0:
            assert a[0] == b[0], (what, j)
            continue
        ps.append(chi2_two_sample(a, b))
        se = np.sqrt(a.var() / a.size + b.var() / b.size)
        assert abs(a.mean() - b.mean()) < 5.0 * se + 1e-9, (what, j, a.mean(), b.mean(), se)
        va, vb = a.var(ddof=1), b.var(ddof=1)
        # var of a sample variance ~ 2 sigma^4 / (n - 1) for near-normal sums (kurtosis-padded by the factor 2)
        tol = 5.0 * np.sqrt(2.0 * 2.0 * (max(va, vb) ** 2) * (1.0 / (a.size - 1) + 1.0 / (b.size - 1)))
        assert abs(va - vb) < tol + 1e-9, (what, j, va, vb, tol)
    ps = np.array(ps)
    assert ps.min() * ps.size > 1e-3, (what, "chi-square: smallest of %d p-values %.3g" % (ps.size, ps.min()))
    assert (ps < 0.01).mean() < 0.08, (what, "too many small p-values", np.sort(ps)[:8])


# ---- exact joint law of the gamma / eta Dirichlet draws ----------------------------------------------------------------
def chi2_uniform(u, nbins=20):
    """p-value of `u` against Uniform(0, 1): chi-square over nbins equal bins (values that round to an end point fall in the end bins)"""
    u = np.asarray(u, dtype=np.float64)
    obs = np.bincount(np.clip((u * nbins).astype(np.int64), 0, nbins - 1), minlength=nbins).astype(np.float64)
    exp = u.size / float(nbins)
    return float(st.chi2.sf(((obs - exp) ** 2 / exp).sum(), nbins - 1))


def stick_variables(x, a):
    """(z [n, G-1], a_g [G-1], b_g [G-1]): with the components of the rows of x [n, G] ~ Dir(a) in ascending order of shape,
    z_g = x_g / sum_{j >= g} x_j (g = 0 .. G-2) are mutually independent Beta(a_g, b_g = sum_{j > g} a_j): the G - 1 marginals and
    the independence ARE the joint law.  The tail sums are formed by adding components from the large end (never as 1 - ...), so a
    component next to a shape of 1e7 keeps its z away from 1.0."""
    x, a = np.asarray(x, dtype=np.float64), np.asarray(a, dtype=np.float64)
    order = np.argsort(a, kind="stable")
    xs, sa = x[:, order], a[order]
    tail = np.cumsum(xs[:, ::-1], axis=1)[:, ::-1]                # tail[:, g] = x_{G-1} + ... + x_g
    atail = np.cumsum(sa[::-1])[::-1]
    return xs[:, :-1] / tail[:, :-1], sa[:-1], atail[1:]


def stick_breaking(x, a):
    """(G - 1 p-values, largest |Spearman rho| between consecutive columns) of the rows of x [n, G] against Dir(a):
    u = Beta cdf of the stick variables, tested for uniformity by a 20-bin chi-square (bins, not KS: robust to the few values
    that round to an end point)"""
    z, sa, sb = stick_variables(x, a)
    u = st.beta.cdf(z, sa[None, :], sb[None, :])
    ps = np.array([chi2_uniform(u[:, g]) for g in range(u.shape[1])])
    rho = max([abs(st.spearmanr(u[:, g], u[:, g + 1])[0]) for g in range(u.shape[1] - 1)] + [0.0])
    return ps, float(rho)


def assert_same_sticks(xa, xb, a, what):
    """two samples of rows, both meant to be Dir(a): two-sample chi-square on every stick variable (no theory involved), with
    the conventions of assert_same_law"""
    za, zb = stick_variables(xa, a)[0], stick_variables(xb, a)[0]
    ps = np.array([chi2_two_sample(za[:, g], zb[:, g]) for g in range(za.shape[1])])
    assert ps.min() * ps.size > 1e-3, (what, "two-sample chi-square: smallest of %d p-values %.3g" % (ps.size, ps.min()))
    assert (ps < 0.01).mean() < 0.08, (what, "too many small p-values", np.sort(ps)[:8])


def dirichlet_law_violations(x, a):
    """what keeps the rows of x [n, G] from being n independent draws of Dir(a) (a list of strings, empty if nothing does):
    the conventions of assert_same_law -- smallest p-value x their number > 1e-3, fewer than 8 % of them below 0.01 -- on the stick
    variables, their rank correlation below 5 / sqrt(n), rows that sum to 1 within 1e-12, and no value twice among all entries
    below 1/2 of the sample (two rows, lanes or iterations on one counter would repeat values).  With fewer than 13 p-values the 8 %
    rule reads "none below 0.01", which a sound sampler misses about once in 100 / (G - 1) seeds: seeds are fixed, and a case that
    misses is answered by the figures of the specification at that seed (tests/test_law_cpu.py), never by another threshold."""
    x, a = np.asarray(x, dtype=np.float64), np.asarray(a, dtype=np.float64)
    n, G = x.shape
    bad = []
    if np.isnan(x).any():
        return ["NaN"]
    if G == 1:
        return [] if (x == 1.0).all() else ["a row of one component is not exactly 1.0"]
    if np.abs(x.sum(axis=1) - 1.0).max() > 1e-12:
        bad.append("row sums off 1 by %.3g" % np.abs(x.sum(axis=1) - 1.0).max())
    if (x < 0.0).any():
        bad.append("negative entries")
    low = x[x < 0.5]                                              # (entries near 1 round onto few doubles -- Dir(0.1, 0.1) gives exactly 1.0
    n_dup = low.size - np.unique(low).size                        # 2 % of the time; every row of G >= 2 has entries below 1/2)
    if n_dup:
        bad.append("%d repeated values among %d" % (n_dup, low.size))
    ps, rho = stick_breaking(x, a)
    if not ps.min() * ps.size > 1e-3:
        bad.append("stick chi-square: smallest of %d p-values %.3g" % (ps.size, ps.min()))
    if not (ps < 0.01).mean() < 0.08:
        bad.append("too many small p-values: %s" % np.sort(ps)[:8])
    if not rho < 5.0 / np.sqrt(n):
        bad.append("sticks are rank-correlated: |rho| = %.4f, bound %.4f" % (rho, 5.0 / np.sqrt(n)))
    return bad


def assert_dirichlet_law(x, a, what):
    bad = dirichlet_law_violations(x, a)
    assert not bad, (what, bad)


def eta_law_violations(etas, esum, delta, transposed=False):
    """eta [n, 4, 4]: row a (true base a) ~ Dir(delta + esum[:, a]) (HaploSNP_Sampler.py:281; esum = E[observed][true]);
    transposed=True judges the rows by esum[a, :] instead, which draws of the right law must FAIL"""
    esum = np.asarray(esum, dtype=np.float64)
    bad = []
    for a in range(4):
        bad += ["row %d: %s" % (a, b) for b in dirichlet_law_violations(etas[:, a, :], delta + (esum[a, :] if transposed else esum[:, a]))]
    # rows of one draw, and draws, share no counter
    flat = np.asarray(etas).reshape(-1)
    flat = flat[flat < 0.5]
    if flat.size - np.unique(flat).size:
        bad.append("repeated values across eta rows")
    return bad


def clamp_law_violations(x, a, eps):
    """gamma rows after the clamp x < eps -> eps and the renormalisation (HaploSNP_Sampler.py:271-273), x [n, G], eps > 0.
    Before the clamp x_g ~ Beta(a_g, a_0 - a_g): the share of entries at the floor (x_post <= eps) is p = cdf(eps), judged by
    z-score (|z| < 5) per column; the entries above the floor are x_pre / (1 + O(G eps)) and follow that Beta truncated at eps
    (20-bin chi-square, Bonferroni over the columns)."""
    x, a = np.asarray(x, dtype=np.float64), np.asarray(a, dtype=np.float64)
    n, G = x.shape
    bad = []
    if np.isnan(x).any():
        return ["NaN"]
    if np.abs(x.sum(axis=1) - 1.0).max() > 1e-12:
        bad.append("row sums off 1 by %.3g" % np.abs(x.sum(axis=1) - 1.0).max())
    lo = eps / (1.0 + G * eps)
    if x.min() < lo * (1.0 - 1e-12):
        bad.append("an entry below the floor: %.6g < %.6g" % (x.min(), lo))
    ps = []
    for g in range(G):
        b = st.beta(a[g], a.sum() - a[g])
        p = float(b.cdf(eps))
        at_floor = x[:, g] <= eps
        sd = np.sqrt(p * (1.0 - p) / n)
        if sd == 0.0:
            if at_floor.mean() != p:
                bad.append("column %d: share at the floor %.4f, exact %.4f" % (g, at_floor.mean(), p))
        elif abs(at_floor.mean() - p) >= 5.0 * sd:
            bad.append("column %d: share at the floor %.4f, exact %.4f (z = %.1f)" % (g, at_floor.mean(), p, (at_floor.mean() - p) / sd))
        above = x[~at_floor, g]
        if above.size >= 400:                                    # 20 bins of >= 20
            ps.append(chi2_uniform((b.cdf(above) - p) / (1.0 - p)))
    ps = np.array(ps)
    if ps.size and not ps.min() * ps.size > 1e-3:
        bad.append("truncated Beta chi-square: smallest of %d p-values %.3g" % (ps.size, ps.min()))
    return bad


# name -> (row of sum_mu, alpha): every case is S = 64 identical rows x 100 iteration counters = 6400 independent rows.
# alpha >= 0.1: below that u^(1/alpha) can underflow to 0.
DIRICHLET_LAW_S, DIRICHLET_LAW_ITERS = 64, 100
DIRICHLET_LAW_CASES = {
    "all-empty": ([0] * 8, 0.1),                                  # every variate through the shape < 1 boost
    "mixed": ([0, 1, 0, 5, 40, 0, 300, 2], 0.1),
    "one-huge": ([0, 10 ** 7, 3, 0], 0.1),
    "G32": ([0, 1] * 16, 0.1),
    "G2": ([0, 0], 0.1),
    "G1": ([5], 0.1),
    "boundary": ([0, 0, 3, 0, 1, 0], 1.0),                        # shape == 1 exactly: the first shape that takes no boost
    "above-one": ([0, 10, 0, 1], 2.5),                            # no variate boosted
}
# asymmetric, with zeros, and a 1000 next to 0.1s: eta row a follows COLUMN a
DIRICHLET_LAW_ESUM = np.array([[500, 0, 3, 40], [0, 0, 1, 7], [2, 9, 1000, 0], [30, 0, 0, 5]], dtype=np.uint64)
DIRICHLET_LAW_ETA_ITERS = 6000
DIRICHLET_CLAMP_CASE = ([0, 10 ** 4, 0, 3, 0, 0], 0.1, 1e-6)       # (row, alpha, epsilon): floor share 0.6626 on the empty columns


def dirichlet_law_draws(draw, row, iters=DIRICHLET_LAW_ITERS, S=DIRICHLET_LAW_S, esum=None):
    """(gamma [iters * S, G], eta [iters, 4, 4]) from draw(it, sum_mu, esum) -> (gamma [S, G], eta [4, 4]), sum_mu = S copies of `row`"""
    sum_mu = np.ascontiguousarray(np.tile(np.asarray(row, dtype=np.uint64), (S, 1)))
    esum = DIRICHLET_LAW_ESUM if esum is None else esum
    gs, es = [], []
    for it in range(iters):
        g, e = draw(it, sum_mu, esum)[:2]
        gs.append(np.array(g)); es.append(np.array(e))
    return np.concatenate(gs, axis=0), np.array(es)
