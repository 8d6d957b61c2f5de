"""The gamma / eta Dirichlet launch (kernels_gibbs.hip: dirichlet_body / gamma_variate) judged on its own terms, and the priors
(dsm_ctx_set_priors) away from their defaults.

  * The exact JOINT law of the device draws: every row against Dir(alpha + sum_mu) / Dir(delta + Esum[:, a]) by stick-breaking
    (tests/_law.py: stick_variables; tests/test_law_cpu.py does the same for the restated specification and shows that the judge
    rejects a missing boost, a wrong boost exponent, a shared uniform, a shared counter and a transposed Esum).  Value parity with
    oracle: orc_dirichlet_counter cannot see a mistake the two share; this can, and a change of the counter layout has to pass it.
  * alpha / delta / epsilon other than 0.1 / 0.1 / 1e-6 through every place they reach: the draw, the clamp (epsilon = 0 too), the
    log-prior terms of dirichlet_body, prior_kernel and prior_batch_kernel, per-chain priors inside a batch, the host class.
Run on an MI355X with:  python -m pytest tests/test_gpu_dirichlet.py -m gpu
"""
import numpy as np
import pytest

from desman_amd import _lib, sampletau
from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
from desman_amd.synth import synth_counts, random_state
from oracle import cbind

from _law import (DIRICHLET_CLAMP_CASE, DIRICHLET_LAW_CASES, DIRICHLET_LAW_ESUM, DIRICHLET_LAW_ETA_ITERS, DIRICHLET_LAW_S,
                  assert_dirichlet_law, clamp_law_violations, dirichlet_law_draws, dirichlet_law_violations, eta_law_violations)

pytestmark = pytest.mark.gpu

# (alpha, delta, epsilon): shapes below 1 with a wide clamp; the branch boundary shape == 1 with the clamp off; no boost at all
PRIORS = [(0.5, 2.0, 1e-4), (1.0, 1.0, 0.0), (2.5, 0.3, 1e-3)]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _load(ctx, counts, tau, gamma, eta, mt_seed=None):
    ctx.set_counts(counts)
    ctx.set_state(tau, gamma, eta)
    if mt_seed is not None:
        ctx.seed(mt_seed)
    ctx.set_tau_rng(_lib.RNG_MT19937)


def _dummy_state(ctx, S, G, ctr_seed):
    """draw_gamma_eta needs a resident state of the shape only: V = 4 dummy counts"""
    counts, _, _ = synth_counts(4, S, max(G, 2), seed=52)
    _load(ctx, counts, *random_state(4, S, G, seed=53))
    ctx.seed(1, ctr_seed=ctr_seed)


# ---------------------------------------------------------------- the law of the device draws
@pytest.mark.parametrize("name", sorted(DIRICHLET_LAW_CASES))
def test_device_dirichlet_draws_have_the_exact_joint_law(ctx, name):
    """clamp off (epsilon = 0), 64 identical rows x 100 iteration counters = 6400 rows a case, against Dir(alpha + sum_mu)"""
    row, alpha = DIRICHLET_LAW_CASES[name]
    _dummy_state(ctx, DIRICHLET_LAW_S, len(row), 99)
    ctx.set_priors(alpha, 0.1, 0.0)
    try:
        g, _ = dirichlet_law_draws(ctx.draw_gamma_eta, row)
    finally:
        ctx.set_priors()
    assert g.shape == (6400, len(row))
    assert_dirichlet_law(g, alpha + np.asarray(row, dtype=np.float64), name)


@pytest.mark.parametrize("delta", [0.1, 2.0])
def test_device_eta_rows_follow_the_columns_of_esum(ctx, delta):
    """eta row a ~ Dir(delta + Esum[:, a]) over 6000 iteration counters; judged by Esum[a, :] the same draws fail"""
    _dummy_state(ctx, 1, 2, 99)
    ctx.set_priors(0.1, delta, 0.0)
    try:
        _, e = dirichlet_law_draws(ctx.draw_gamma_eta, [0, 3], iters=DIRICHLET_LAW_ETA_ITERS, S=1)
    finally:
        ctx.set_priors()
    bad = eta_law_violations(e, DIRICHLET_LAW_ESUM, delta)
    assert not bad, bad
    assert eta_law_violations(e, DIRICHLET_LAW_ESUM, delta, transposed=True)


def test_device_clamp_has_the_exact_floor_share(ctx):
    """epsilon = 1e-6, four empty haplotypes next to 1e4 reads: 66.26 % of their draws at the floor, the rest the truncated Beta"""
    row, alpha, eps = DIRICHLET_CLAMP_CASE
    a = alpha + np.asarray(row, dtype=np.float64)
    _dummy_state(ctx, DIRICHLET_LAW_S, len(row), 99)
    ctx.set_priors(alpha, 0.1, eps)
    try:
        g, _ = dirichlet_law_draws(ctx.draw_gamma_eta, row)
    finally:
        ctx.set_priors()
    bad = clamp_law_violations(g, a, eps)
    assert not bad, bad
    assert dirichlet_law_violations(g, a)                         # and the clamp was on


# ---------------------------------------------------------------- non-default priors: value parity
@pytest.mark.parametrize("alpha,delta,epsilon", PRIORS)
@pytest.mark.parametrize("S,G", [(1, 1), (16, 8), (96, 12), (64, 32)])
def test_dirichlet_draws_match_spec_under_priors(ctx, S, G, alpha, delta, epsilon):
    """test_dirichlet_draws_match_spec (tests/test_gpu_parity.py) with the priors passed through, same tolerance"""
    seed = 0x1234ABCD5678EF01
    _dummy_state(ctx, S, G, seed)
    rng = np.random.default_rng(S * 100 + G)
    sum_mu = rng.integers(0, 3000, size=(S, G)).astype(np.uint64)
    sum_mu[0, :] = 0                                              # every shape = alpha
    if S > 1:
        sum_mu[1, :] = 0; sum_mu[1, 0] = 10 ** 7                  # one huge shape next to alphas: the clamp
    if S > 2:
        sum_mu[2, :] = 10 ** 7
    if S > 3:
        sum_mu[3, ::2] = 0                                        # boosted and plain variates side by side
    esum = rng.integers(0, 9000, size=(4, 4)).astype(np.uint64)   # asymmetric
    esum[3, :] = 0; esum[3, 3] = 10 ** 7
    esum[0, 1] = 0
    ctx.set_priors(alpha, delta, epsilon)
    try:
        for it in (0, 3, 1000):
            g, e = ctx.draw_gamma_eta(it, sum_mu, esum)
            g_ref, e_ref, _ = cbind.dirichlet_counter(sum_mu, esum, seed, it, alpha, delta, epsilon)
            np.testing.assert_allclose(g, g_ref, rtol=1e-13, atol=0)
            np.testing.assert_allclose(e, e_ref, rtol=1e-13, atol=0)
            if epsilon > 0 and G > 1:
                assert g.min() >= epsilon / (1.0 + G * epsilon) * (1 - 1e-12)
    finally:
        ctx.set_priors()
    g, e = ctx.draw_gamma_eta(0, sum_mu, esum)                     # and back at the defaults
    g_ref, e_ref, _ = cbind.dirichlet_counter(sum_mu, esum, seed, 0)
    np.testing.assert_allclose(g, g_ref, rtol=1e-13, atol=0)
    np.testing.assert_allclose(e, e_ref, rtol=1e-13, atol=0)


@pytest.mark.parametrize("alpha,delta,epsilon", PRIORS)
@pytest.mark.parametrize("V,S,G", [(333, 20, 3), (200, 96, 12), (50, 300, 1)])
def test_logpost_under_priors(ctx, V, S, G, alpha, delta, epsilon):
    """prior_kernel + dirichlet_consts: lp of a given state"""
    counts, _, _ = synth_counts(V, S, max(G, 2), seed=7)
    tau, gamma, eta = random_state(V, S, G, seed=8)
    _load(ctx, counts, tau, gamma, eta)
    idx = cbind.onehot_to_idx(tau)
    lp_default = ctx.loglik()[1]
    ctx.set_priors(alpha, delta, epsilon)
    try:
        ll, lp = ctx.loglik()
    finally:
        ctx.set_priors()
    assert ll == pytest.approx(cbind.loglik(idx, gamma, eta, counts), rel=1e-12)
    assert lp == pytest.approx(cbind.logpost(idx, gamma, eta, counts, alpha, delta), rel=1e-12)
    assert lp_default == pytest.approx(cbind.logpost(idx, gamma, eta, counts), rel=1e-12)
    # the priors do reach lp: the two differ by the difference of the Dirichlet log-priors (both lp are sums of ~1e7: 1e-12 rel each)
    d_prior = cbind.logprior(gamma, eta, V, alpha, delta) - cbind.logprior(gamma, eta, V)
    assert abs(d_prior) > 1.0
    assert lp - lp_default == pytest.approx(d_prior, abs=2e-12 * abs(lp))


# ---------------------------------------------------------------- non-default priors: the loops
@pytest.mark.parametrize("spec", [2, 1])
@pytest.mark.parametrize("V,S,G,n_iter", [(400, 16, 5, 12), (200, 20, 11, 4)])      # stage 2 fused into the Dirichlet launch / its own launch
def test_gibbs_update_under_priors_is_self_consistent_with_oracle(ctx, V, S, G, n_iter, spec):
    """the walk of test_gibbs_update_is_self_consistent_with_oracle (tests/test_gpu_parity.py) at alpha = 0.5, delta = 2, epsilon = 1e-4"""
    alpha, delta, epsilon = PRIORS[0]
    counts, _, _ = synth_counts(V, S, G, seed=60)
    tau0, gamma0, eta0 = random_state(V, S, G, seed=61)
    _load(ctx, counts, tau0, gamma0, eta0, mt_seed=123)
    cseed = 0x5EEDC0DE1000 + spec
    ctx.seed(123, ctr_seed=cseed)
    ctx.force_stats_spec(spec)
    ctx.set_priors(alpha, delta, epsilon)
    try:
        ll0, lp0 = ctx.loglik()
        ctx.gibbs_update(n_iter)
    finally:
        ctx.set_priors()
        ctx.force_stats_spec(0)
    tr = ctx.get_trace()
    assert lp0 == pytest.approx(cbind.logpost(cbind.onehot_to_idx(tau0), gamma0, eta0, counts, alpha, delta), rel=1e-12)
    g_prev, e_prev, t_prev = gamma0, eta0, tau0
    for it in range(n_iter):
        args = (cbind.onehot_to_idx(t_prev), np.ascontiguousarray(g_prev), np.ascontiguousarray(e_prev), counts, cseed, it)
        mu, E = cbind.stats_agg(*args, spec=spec) if spec >= 2 else cbind.stats_counter(*args)
        g_ref, e_ref, _ = cbind.dirichlet_counter(mu, E, cseed, it, alpha, delta, epsilon)
        np.testing.assert_allclose(tr["gamma"][it], g_ref, rtol=1e-13, atol=0)
        np.testing.assert_allclose(tr["eta"][it], e_ref, rtol=1e-13, atol=0)
        g_prev, e_prev, t_prev = tr["gamma"][it], tr["eta"][it], ctx.get_tau_at(it)
    assert tr["gamma"].min() >= epsilon / (1.0 + G * epsilon) * (1 - 1e-12)
    mt = cbind.MT19937(123)
    tau_prev, eta_prev = tau0.copy(), eta0.copy()
    lps = [lp0]
    for it in range(n_iter):
        tau_it = ctx.get_tau_at(it)
        ref = tau_prev.copy()
        n_ref = cbind.sample_tau_u(ref, np.ascontiguousarray(tr["gamma"][it]), eta_prev, counts, mt.uniform(V * G))
        assert np.array_equal(tau_it, ref) and tr["nchange"][it] == n_ref          # bit-exact
        idx = cbind.onehot_to_idx(tau_it)
        g_it, e_it = np.ascontiguousarray(tr["gamma"][it]), np.ascontiguousarray(tr["eta"][it])
        assert tr["ll"][it] == pytest.approx(cbind.loglik(idx, g_it, e_it, counts), rel=1e-12)
        assert tr["lp"][it] == pytest.approx(cbind.logpost(idx, g_it, e_it, counts, alpha, delta), rel=1e-12)
        lps.append(tr["lp"][it])
        tau_prev, eta_prev = tau_it, e_it
    star = ctx.get_star()
    k = int(np.argmax(lps))                                       # first strict maximum, entry state = slot 0
    assert star["lp"] == lps[k]
    if k == 0:
        assert np.array_equal(star["tau"], tau0) and np.array_equal(star["gamma"], gamma0)
    else:
        assert np.array_equal(star["tau"], ctx.get_tau_at(k - 1)) and np.array_equal(star["gamma"], tr["gamma"][k - 1]) \
            and np.array_equal(star["eta"], tr["eta"][k - 1]) and star["it"] == k - 1


@pytest.mark.parametrize("alpha,delta,epsilon", PRIORS)
def test_update_tau_under_priors(ctx, alpha, delta, epsilon):
    """prior_batch_kernel: lp of every stored state of updateTau"""
    V, S, G, n = 200, 16, 4, 5
    counts, _, _ = synth_counts(V, S, G, seed=80)
    tau0, gamma0, eta0 = random_state(V, S, G, seed=81)
    rng = np.random.default_rng(1)
    gs = np.ascontiguousarray(rng.dirichlet(np.ones(G), size=(n, S)))
    es = np.ascontiguousarray(np.stack([random_state(1, 1, 1, seed=k)[2] for k in range(n)]))
    _load(ctx, counts, tau0, gamma0, eta0, mt_seed=99)
    ctx.set_priors(alpha, delta, epsilon)
    try:
        ctx.update_tau(gs, es)
    finally:
        ctx.set_priors()
    tr = ctx.get_trace()
    mt = cbind.MT19937(99)
    ref = tau0.copy()
    lp_best, tau_best = cbind.logpost(cbind.onehot_to_idx(ref), gs[0], es[0], counts, alpha, delta), ref.copy()
    for it in range(n):
        cbind.sample_tau_u(ref, gs[it], es[it], counts, mt.uniform(V * G))
        assert np.array_equal(ctx.get_tau_at(it), ref)
        lp = cbind.logpost(cbind.onehot_to_idx(ref), gs[it], es[it], counts, alpha, delta)
        assert tr["lp"][it] == pytest.approx(lp, rel=1e-12)
        assert tr["ll"][it] == pytest.approx(cbind.loglik(cbind.onehot_to_idx(ref), gs[it], es[it], counts), rel=1e-12)
        if lp > lp_best:
            lp_best, tau_best = lp, ref.copy()
    star = ctx.get_star()
    assert np.array_equal(star["tau"], tau_best) and star["lp"] == pytest.approx(lp_best, rel=1e-12)


# ---------------------------------------------------------------- per-chain priors inside a batch
def _chain(counts, state, seed, ctr_seed, priors, spec):
    c = _lib.Context(0)
    c.set_counts(counts)
    c.set_state(*state)
    c.set_tau_rng(_lib.RNG_MT19937)
    c.seed(seed, ctr_seed=ctr_seed)
    c.set_priors(*priors)
    c.force_stats_spec(spec)
    return c


def _snapshot(c):
    tr, star = c.get_trace(), c.get_star()
    out = dict(tau=c.get_state()[0], mt=c.get_mt_state(), lp_star=np.float64(star["lp"]), tau_star=star["tau"], gamma_star=star["gamma"])
    out.update({k: tr[k] for k in ("ll", "lp", "nchange", "gamma", "eta")})
    return out


@pytest.mark.parametrize("V,S,G,n_iter,spec", [(300, 16, 5, 6, 2), (300, 16, 5, 6, 0), (90, 20, 11, 4, 2)])
def test_batch_with_a_prior_setting_per_chain_equals_chains_run_one_by_one(V, S, G, n_iter, spec):
    """DirBatch carries alpha / delta / epsilon / lgc per chain: three chains of one shape, three settings, bit for bit"""
    counts, _, _ = synth_counts(V, S, G, seed=500 + V)
    states = [random_state(V, S, G, seed=600 + k) for k in range(3)]

    def build(k, priors):
        return _chain(counts, states[k], 1000 + k, 0xB47C5000 + k, priors, spec)

    single = []
    for k in range(3):
        a = build(k, PRIORS[k])
        a.gibbs_update(n_iter)
        single.append(_snapshot(a))
        a.close()
    ctxs = [build(k, PRIORS[k]) for k in range(3)]
    _lib.Context.batch_gibbs_update(ctxs, n_iter)
    got = [_snapshot(c) for c in ctxs]
    for c in ctxs:
        c.close()
    for k in range(3):
        for name in single[k]:
            assert np.array_equal(single[k][name], got[k][name]), (k, name)
    # the settings are told apart: chain 0 under chain 1's priors is another chain
    other = build(0, PRIORS[1])
    other.gibbs_update(n_iter)
    assert not np.array_equal(other.get_trace()["gamma"], single[0]["gamma"])
    other.close()


# ---------------------------------------------------------------- the host class forwards its priors
def test_sampler_class_forwards_its_priors():
    """HaploSNP_Sampler(alpha_constant=, delta_constant=, epsilon=) = a bare context given the same priors, state and streams"""
    alpha, delta, epsilon = PRIORS[0]
    V, S, G, n = 300, 16, 4, 5
    counts, _, _ = synth_counts(V, S, G, seed=17)
    sampletau.initRNG(); sampletau.setRNG(4321)
    try:
        mt0 = np.array(sampletau.getRNGState(), dtype=np.uint32)
        smp = HaploSNP_Sampler(counts, G, np.random.RandomState(3), max_iter=n, alpha_constant=alpha, delta_constant=delta,
                               epsilon=epsilon)
        tau0, gamma0, eta0 = smp.tau.copy(), smp.gamma.copy(), smp.eta.copy()
        smp.update()
        key, n_drawn = smp._ctx.counters()
    finally:
        sampletau.freeRNG()
    assert n_drawn == n
    c = _lib.Context(0)
    try:
        c.set_counts(counts)
        c.set_priors(alpha, delta, epsilon)
        c.set_state(tau0, gamma0, eta0)
        c.seed(1, ctr_seed=key)
        c.set_mt_state(mt0)
        c.gibbs_update(n)
        tr = c.get_trace()
        for k, store in (("gamma", smp.gamma_store), ("eta", smp.eta_store), ("lp", smp.lp_store), ("ll", smp.ll_store)):
            assert np.array_equal(tr[k], store), k
        assert np.array_equal(c.get_state()[0], smp.tau)
        # ... and those priors are the ones asked for
        for it in range(n):
            idx = cbind.onehot_to_idx(c.get_tau_at(it))
            lp = cbind.logpost(idx, np.ascontiguousarray(tr["gamma"][it]), np.ascontiguousarray(tr["eta"][it]), counts, alpha, delta)
            assert smp.lp_store[it] == pytest.approx(lp, rel=1e-12)
        assert smp.gamma_store.min() >= epsilon / (1.0 + G * epsilon) * (1 - 1e-12)
        c.set_priors()
        c.set_state(tau0, gamma0, eta0)
        c.seed(1, ctr_seed=key)
        c.set_mt_state(mt0)
        c.gibbs_update(n)
        assert not np.array_equal(c.get_trace()["gamma"], smp.gamma_store)
    finally:
        c.close()
