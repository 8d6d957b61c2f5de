"""The chain with tau held (dsm_ctx_gibbs_update_fixed_tau) on the GPU: every piece of every iteration against the oracle, the pooled
table against numpy, the pooled chain against the unpooled chain of the pooled table, the law of the pooled sums, and the posterior of
the abundances end to end (HaploSNP_Sampler.posteriorGamma, `desman-abund --posterior`).  The statistical conditions are checked for
the oracle's restatement with the same seeds in tests/test_fixed_tau_cpu.py.
Run on an MI355X with:  python -m pytest tests/test_gpu_fixed_tau.py -m gpu
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fixtau as F  # noqa: E402

from desman_amd import _lib, fixed_tau  # noqa: E402
from desman_amd.synth import synth_counts, random_state  # noqa: E402
from oracle import cbind  # noqa: E402

pytestmark = pytest.mark.gpu
MT_SEED = 123


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    c = _lib.Context(0)
    yield c
    c.close()


def _load(c, counts, tau, gamma, eta, cseed, spec=0):
    c.set_counts(counts)
    c.set_state(tau, gamma, eta)
    c.seed(MT_SEED, ctr_seed=cseed)
    c.set_tau_rng(_lib.RNG_MT19937)
    c.force_stats_spec(spec)


def _star_rule(star, lps, entry, tr, tau0):
    """the MAP record by the first strict maximum over (entry state, iterations), as tests/test_gpu_parity.py checks it"""
    k = int(np.argmax(lps))
    assert star["lp"] == lps[k] and np.array_equal(star["tau"], tau0)
    if k == 0:
        assert np.array_equal(star["gamma"], entry[0]) and np.array_equal(star["eta"], entry[1])
    else:
        assert np.array_equal(star["gamma"], tr["gamma"][k - 1]) and np.array_equal(star["eta"], tr["eta"][k - 1]) and star["it"] == k - 1


# ---- 1. every piece against the oracle, unpooled ----------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (65, 3, 2), (257, 16, 4), (600, 24, 8), (300, 9, 10), (130, 17, 12)]


@pytest.mark.parametrize("fix_eta", [0, 1])
@pytest.mark.parametrize("spec", [1, 2, 3, 4])
@pytest.mark.parametrize("V,S,G", SHAPES)
def test_every_piece_of_the_unpooled_chain_against_the_oracle(ctx, V, S, G, spec, fix_eta):
    n_iter = 4
    counts, _, _ = synth_counts(V, S, max(G, 2), seed=300 + V)
    tau0, gamma0, eta0 = random_state(V, S, G, seed=301 + G)
    idx0 = cbind.onehot_to_idx(tau0)
    cseed = 0xF1C5ED7A0000 + 16 * spec + fix_eta
    _load(ctx, counts, tau0, gamma0, eta0, cseed, spec)
    try:
        ll0, lp0 = ctx.loglik()
        mt0, (key0, it0) = ctx.get_mt_state(), ctx.counters()
        ctx.gibbs_update_fixed_tau(n_iter, fix_eta=bool(fix_eta), pool=0)
    finally:
        ctx.force_stats_spec(0)
    tr = ctx.get_trace()
    g_prev, e_prev = gamma0, eta0
    worst = 0.0
    for it in range(n_iter):
        mu, E = F.stats(spec, idx0, g_prev, e_prev, counts, cseed, it)
        g_ref, e_ref, _ = cbind.dirichlet_counter(mu, E, cseed, it)
        np.testing.assert_allclose(tr["gamma"][it], g_ref, rtol=1e-13, atol=0)
        if fix_eta:
            assert np.array_equal(tr["eta"][it], eta0)
        else:
            np.testing.assert_allclose(tr["eta"][it], e_ref, rtol=1e-13, atol=0)
        g_prev, e_prev = np.ascontiguousarray(tr["gamma"][it]), np.ascontiguousarray(tr["eta"][it])
        ll, lp = cbind.loglik(idx0, g_prev, e_prev, counts), cbind.logpost(idx0, g_prev, e_prev, counts)
        worst = max(worst, abs(tr["ll"][it] - ll) / abs(ll), abs(tr["lp"][it] - lp) / abs(lp))
        assert tr["ll"][it] == pytest.approx(ll, rel=1e-12) and tr["lp"][it] == pytest.approx(lp, rel=1e-12)
        assert np.array_equal(ctx.get_tau_at(it), tau0)
    print("V=%d S=%d G=%d spec %d fix_eta %d: largest relative distance of ll / lp from the oracle %.2e" % (V, S, G, spec, fix_eta, worst))
    tau_f, gamma_f, eta_f = ctx.get_state()
    assert np.array_equal(tau_f, tau0) and np.array_equal(gamma_f, tr["gamma"][-1]) and np.array_equal(eta_f, tr["eta"][-1])
    assert np.array_equal(ctx.get_tau_sum(), n_iter * tau0) and not tr["nchange"].any()
    assert lp0 == pytest.approx(cbind.logpost(idx0, gamma0, eta0, counts), rel=1e-12)
    _star_rule(ctx.get_star(), [lp0] + list(tr["lp"]), (gamma0, eta0), tr, tau0)
    assert np.array_equal(ctx.get_mt_state(), mt0) and ctx.counters() == (key0, it0 + n_iter)


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("fix_eta", [0, 1])
def test_two_calls_of_two_iterations_are_one_call_of_four(ctx, pool, fix_eta):
    V, S, G = 257, 16, 4
    counts, _, _ = synth_counts(V, S, G, seed=41)
    tau0, gamma0, eta0 = random_state(V, S, G, seed=42)
    _load(ctx, counts, tau0, gamma0, eta0, 0xABCDEF01)
    ctx.gibbs_update_fixed_tau(4, fix_eta=bool(fix_eta), pool=pool)
    one, state_one, ctr_one = ctx.get_trace(), ctx.get_state(), ctx.counters()
    _load(ctx, counts, tau0, gamma0, eta0, 0xABCDEF01)
    ctx.gibbs_update_fixed_tau(2, fix_eta=bool(fix_eta), pool=pool)
    a = ctx.get_trace()
    ctx.gibbs_update_fixed_tau(2, fix_eta=bool(fix_eta), pool=pool)
    b = ctx.get_trace()
    for key in ("gamma", "eta", "ll", "lp", "nchange"):
        assert np.array_equal(np.concatenate([a[key], b[key]]), one[key]), key
    assert all(np.array_equal(x, y) for x, y in zip(ctx.get_state(), state_one)) and ctx.counters() == ctr_one


@pytest.mark.parametrize("pool", [0, 1])
def test_a_gibbs_update_after_a_fixed_tau_call_is_the_chain_the_oracle_predicts(ctx, pool):
    """no state leaks: from the state, the MT19937 stream and the counters a fixed-tau call leaves behind, two full Gibbs iterations are
    what the oracle's pieces give"""
    V, S, G, spec, n_fix = 257, 16, 4, 2, 3
    counts, _, _ = synth_counts(V, S, G, seed=43)
    tau0, gamma0, eta0 = random_state(V, S, G, seed=44)
    cseed = 0x5EED0000F1C5
    _load(ctx, counts, tau0, gamma0, eta0, cseed, spec)
    try:
        ctx.gibbs_update_fixed_tau(n_fix, pool=pool)
        tau_e, g_prev, e_prev = ctx.get_state()
        assert np.array_equal(tau_e, tau0)
        ctx.gibbs_update(2)
    finally:
        ctx.force_stats_spec(0)
    tr = ctx.get_trace()
    mt = cbind.MT19937(MT_SEED)
    t_prev = tau0.copy()
    for it in range(2):
        mu, E = F.stats(spec, cbind.onehot_to_idx(t_prev), g_prev, e_prev, counts, cseed, n_fix + it)
        g_ref, e_ref, _ = cbind.dirichlet_counter(mu, E, cseed, n_fix + it)
        np.testing.assert_allclose(tr["gamma"][it], g_ref, rtol=1e-13, atol=0)
        np.testing.assert_allclose(tr["eta"][it], e_ref, rtol=1e-13, atol=0)
        ref = t_prev.copy()
        n_ref = cbind.sample_tau_u(ref, np.ascontiguousarray(tr["gamma"][it]), np.ascontiguousarray(e_prev), counts, mt.uniform(V * G))
        assert np.array_equal(ctx.get_tau_at(it), ref) and tr["nchange"][it] == n_ref
        g_prev, e_prev, t_prev = np.ascontiguousarray(tr["gamma"][it]), np.ascontiguousarray(tr["eta"][it]), ref
    assert np.array_equal(ctx.get_tau_sum(), ctx.get_tau_at(0) + ctx.get_tau_at(1)) and ctx.counters() == (cseed, n_fix + 2)


def test_no_state_and_negative_lengths_are_refused(ctx):
    counts, _, _ = synth_counts(20, 3, 2, seed=1)
    c = _lib.Context(0)
    try:
        c.set_counts(counts)
        assert c.lib.dsm_ctx_gibbs_update_fixed_tau(c._h, 2, 0, 0) == -3             # DSM_ERR_STATE
        tau, gamma, eta = random_state(20, 3, 2, seed=2)
        c.set_state(tau, gamma, eta)
        assert c.lib.dsm_ctx_gibbs_update_fixed_tau(c._h, -1, 0, 0) == -2            # DSM_ERR_ARG
        assert c.lib.dsm_ctx_gibbs_update_fixed_tau(c._h, 1, 0, 3) == -2
        c.seed(1)
        c.gibbs_update_fixed_tau(0)                                                  # the entry state only
        assert c.get_star()["it"] == 0 and np.array_equal(c.get_star()["gamma"], gamma)
    finally:
        c.close()


# ---- 2. the pooled table ------------------------------------------------------------------------------------------------------------
def _pool_cases():
    rng = np.random.default_rng(9)
    few = fixed_tau.words_to_digits(rng.permutation(16)[:10].astype(np.uint64), 2)[rng.integers(0, 10, size=300)]
    yield "few-words", few, rng.integers(0, 200, size=(300, 5, 4))
    yield "random", rng.integers(0, 4, size=(257, 4)), rng.integers(0, 200, size=(257, 3, 4))
    yield "distinct", fixed_tau.words_to_digits(rng.permutation(4 ** 8)[:64].astype(np.uint64), 8), rng.integers(0, 200, size=(64, 2, 4))
    yield "one-position", rng.integers(0, 4, size=(1, 3)), rng.integers(0, 200, size=(1, 4, 4))


POOL_CASES = {name: (np.ascontiguousarray(t, dtype=np.int64), np.ascontiguousarray(x, dtype=np.int64)) for name, t, x in _pool_cases()}


@pytest.mark.parametrize("case", sorted(POOL_CASES))
def test_the_pooled_table_is_numpys(ctx, case):
    digits, counts = POOL_CASES[case]
    V, G = digits.shape
    S = counts.shape[1]
    _, gamma, eta = random_state(V, S, G, seed=5)
    _load(ctx, counts, cbind.idx_to_onehot(digits), gamma, eta, 1)
    got = ctx.debug_fixtau_pool()
    w = fixed_tau.tau_words(digits)
    words, inv = np.unique(w, return_inverse=True)
    pooled = np.zeros((len(words), S, 4), dtype=np.int64)
    np.add.at(pooled, np.asarray(inv).reshape(-1), counts)
    assert got["W"] == len(words) and (case != "few-words" or got["W"] <= 16) and (case != "distinct" or got["W"] == V)
    assert np.array_equal(got["words"], words) and (np.diff(got["words"].astype(np.int64)) > 0).all()
    assert np.array_equal(got["row"], np.asarray(inv).reshape(-1)) and np.array_equal(got["pooled"], pooled)
    again = ctx.debug_fixtau_pool()
    assert all(np.array_equal(got[k], again[k]) for k in ("pooled", "words", "row"))


def test_a_pooled_count_above_int32_is_refused_or_runs_unpooled(ctx):
    counts = np.zeros((2, 1, 4), dtype=np.int64)
    counts[:, 0, 0] = 2 ** 30 + 1
    tau0 = cbind.idx_to_onehot(np.array([[1, 2], [1, 2]]))
    gamma0, eta0 = np.array([[0.4, 0.6]]), 0.96 * np.eye(4) + 0.01
    runs = []
    for pool in (1, -1, 0):
        _load(ctx, counts, tau0, gamma0, eta0, 77, 2)
        try:
            rc = ctx.lib.dsm_ctx_gibbs_update_fixed_tau(ctx._h, 2, 0, pool)
        finally:
            ctx.force_stats_spec(0)
        if pool == 1:
            assert rc == -4 and b"2^31" in ctx.lib.dsm_last_error()           # DSM_ERR_UNSUPPORTED
            continue
        assert rc == 0
        ctx.n_trace = 2
        runs.append((ctx.get_trace(), ctx.get_state()))
    for key in ("gamma", "eta", "ll", "lp"):
        assert np.array_equal(runs[0][0][key], runs[1][0][key]), key
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))


# ---- 3. the pooled chain is the unpooled chain of the pooled table -----------------------------------------------------------------------
@pytest.mark.parametrize("fix_eta", [0, 1])
@pytest.mark.parametrize("spec", [0, 2])
@pytest.mark.parametrize("case", ["few-words", "random", "one-position"])
def test_the_pooled_chain_is_the_unpooled_chain_of_the_pooled_table(ctx, ctx2, case, spec, fix_eta):
    digits, counts = POOL_CASES[case]
    V, G = digits.shape
    S = counts.shape[1]
    n_iter, cseed = 5, 0x0123456789AB + spec
    _, gamma0, eta0 = random_state(V, S, G, seed=6)
    pd_digits, pooled = F.pooled_table(digits, counts)
    _load(ctx, counts, cbind.idx_to_onehot(digits), gamma0, eta0, cseed, spec)
    _load(ctx2, pooled, cbind.idx_to_onehot(pd_digits), gamma0, eta0, cseed, spec)
    try:
        ctx.gibbs_update_fixed_tau(n_iter, fix_eta=bool(fix_eta), pool=1)
        ctx2.gibbs_update_fixed_tau(n_iter, fix_eta=bool(fix_eta), pool=0)
    finally:
        ctx.force_stats_spec(0); ctx2.force_stats_spec(0)
    a, b, sa, sb = ctx.get_trace(), ctx2.get_trace(), ctx.get_star(), ctx2.get_star()
    assert np.array_equal(a["gamma"], b["gamma"]) and np.array_equal(a["eta"], b["eta"]) and not a["nchange"].any()
    assert np.array_equal(sa["gamma"], sb["gamma"]) and np.array_equal(sa["eta"], sb["eta"]) and sa["it"] == sb["it"]
    assert np.array_equal(sa["tau"], cbind.idx_to_onehot(digits)) and ctx.counters() == ctx2.counters() == (cseed, n_iter)
    assert all(np.array_equal(x, y) for x, y in zip(ctx.get_state()[1:], ctx2.get_state()[1:]))
    assert np.array_equal(ctx.get_state()[0], cbind.idx_to_onehot(digits)) and np.array_equal(ctx.get_tau_sum(), n_iter * cbind.idx_to_onehot(digits))
    c_orig, c_pool = cbind.loglik_const(counts), cbind.loglik_const(pooled)
    K = c_orig - c_pool
    worst = 0.0
    idx = np.ascontiguousarray(digits, dtype=np.uint8)
    for it in range(n_iter):
        g, e = np.ascontiguousarray(a["gamma"][it]), np.ascontiguousarray(a["eta"][it])
        ll_ref = cbind.loglik(idx, g, e, counts)
        bound = 1e-12 * max(abs(ll_ref), abs(c_orig), abs(c_pool))
        d = max(abs(a["ll"][it] - (b["ll"][it] + K)), abs(a["lp"][it] - (b["lp"][it] + K)), abs(a["ll"][it] - ll_ref))
        worst = max(worst, d / bound)
        assert d <= bound
    assert abs(sa["lp"] - (sb["lp"] + K)) <= 1e-12 * max(abs(sa["lp"]), abs(c_orig), abs(c_pool))
    print("%s spec %d fix_eta %d: W = %d of V = %d, largest distance of ll / lp = %.3f of the bound" % (case, spec, fix_eta, len(pd_digits), V, worst))


# ---- 4. pooling keeps the law -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [0, 2, 4])
def test_pooling_keeps_the_law_of_the_sums(ctx, spec):
    """the means of 400 draws of sum_mu and Esum made ON THE POOLED state lie within 5 standard errors (exact multinomial variance) of
    their exact expectations ON THE ORIGINAL table; the oracle passes the same condition with the same seeds (tests/test_fixed_tau_cpu.py)"""
    counts, tau, gamma, eta = F.law_case()
    _load(ctx, counts, cbind.idx_to_onehot(tau), gamma, eta, F.LAW_SEED, spec)
    try:
        draws = [ctx.debug_fixtau_sample_stats(it) for it in range(F.LAW_N)]
    finally:
        ctx.force_stats_spec(0)
    assert all(int(m.sum()) == int(counts.sum()) for m, _ in draws)
    bad = F.law_violations([d[0] for d in draws], [d[1] for d in draws], F.sum_moments(tau, gamma, eta, counts))
    assert not bad, bad
    assert np.array_equal(ctx.get_state()[1], gamma) and ctx.counters() == (F.LAW_SEED, 0)      # the caller's chain is untouched


# ---- 5. posterior, end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def posteriors():
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    counts, tau, eta = F.posterior_case()
    smp = HaploSNP_Sampler(counts, F.POST_SHAPE[2], np.random.RandomState(1), max_iter=2)
    kw = dict(snps=counts, tau=tau, eta=eta, n_iter=F.POST_N, burn=F.POST_BURN, seed=F.POST_SEED)
    post = {pool: smp.posteriorGamma(pool=pool, **kw) for pool in (0, 1)}
    post["again"] = smp.posteriorGamma(pool=1, **kw)
    post["auto"] = smp.posteriorGamma(**kw)
    post["eta"] = smp.posteriorGamma(fix_eta=False, **kw)
    post["ml"] = smp.fitGamma(snps=counts, tau=tau, eta=eta)["gamma"]
    return post


def test_posterior_of_the_abundances_sits_on_the_ml_estimate(posteriors):
    for pool in (0, 1):
        assert posteriors[pool]["draws"].shape == (F.POST_N - F.POST_BURN,) + F.POST_SHAPE[1:]
        assert not F.posterior_violations(posteriors[pool], posteriors["ml"])
    e = posteriors["eta"]
    assert not F.posterior_violations(e, posteriors["ml"]) and np.abs(e["eta_mean"] - (0.96 * np.eye(4) + 0.01)).max() < 0.01
    assert np.allclose(e["eta_mean"].sum(axis=1), 1.0, atol=1e-12) and "eta_mean" not in posteriors[0]


def test_posterior_is_reproducible_and_pooling_does_not_move_it(posteriors):
    """the same seed gives the same bits; pool = 0 and pool = 1 are different draws of one law: their means agree within 5 Monte-Carlo
    standard errors of the difference, each chain's standard error taken from every fifth kept draw (_fixtau.mc_se)"""
    for key in ("draws", "mean", "sd", "lo", "med", "hi", "ll"):
        assert np.array_equal(posteriors[1][key], posteriors["again"][key]), key
    assert np.array_equal(posteriors["auto"]["draws"], posteriors[1]["draws"])                 # 300 positions, at most 64 words: auto pools
    assert not np.array_equal(posteriors[0]["draws"], posteriors[1]["draws"])
    assert not F.means_disagree(posteriors[0], posteriors[1]).any()


def test_update_fixed_tau_mirrors_the_reference_method():
    from desman_amd import sampletau
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    V, S, G, n = 120, 6, 3, 8
    counts, tau_true, _ = synth_counts(V, S, G, seed=8)
    sampletau.initRNG(); sampletau.setRNG(99)
    smp = HaploSNP_Sampler(counts, G, np.random.RandomState(2), fixed_tau=cbind.idx_to_onehot(tau_true), max_iter=n)
    tau0, mt0 = smp.tau.copy(), sampletau.getRNGState().copy()
    smp.update_fixed_tau()
    assert np.array_equal(smp.tau, tau0) and np.array_equal(sampletau.getRNGState(), mt0) and not smp.nchange_store.any()
    assert np.array_equal(smp.gamma, smp.gamma_store[-1]) and np.array_equal(smp.eta, smp.eta_store[-1]) and smp.lp == smp.lp_store[-1]
    assert smp.lp_star >= smp.lp_store.max() and np.array_equal(smp.tau_star, tau0) and np.array_equal(smp.tauMean(), tau0)
    idx = cbind.onehot_to_idx(tau0)
    for it in (0, n - 1):
        g, e = np.ascontiguousarray(smp.gamma_store[it]), np.ascontiguousarray(smp.eta_store[it])
        assert smp.ll_store[it] == pytest.approx(cbind.loglik(idx, g, e, counts), rel=1e-11)     # (pooled by the auto rule: + K in fp64)
    held = smp.eta.copy()
    smp.update_fixed_tau(fix_eta=True, pool=0)
    assert all(np.array_equal(row, held) for row in smp.eta_store) and np.array_equal(smp.eta_star, held)


# ---- 6. command line --------------------------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_desman_abund_posterior(tmp_path):
    """`desman` on the 240 x 12 table of the abund tests, then `desman-abund` for four new samples with and without --posterior"""
    from desman_amd import abund, cli
    V, S, G = 240, 12, 3
    counts, _, _ = synth_counts(V, S, G, seed=123)
    freq = str(tmp_path / "fit.freq")
    _write_freq(freq, counts, ["S%d" % s for s in range(S)], ["contig%d" % (v // 50) for v in range(V)], np.arange(V) * 7 + 3)
    run = str(tmp_path / "run")
    cli.main([freq, "-g", str(G), "-i", "40", "-o", run, "-s", "7"])
    contigs, positions, digits, eta_star = abund.load_model(run)
    rs = np.random.RandomState(5)
    gamma = rs.dirichlet(np.full(digits.shape[1], 4.0), size=4)
    p = np.einsum("sg,vgb->vsb", gamma, eta_star[digits])
    new = np.array([[rs.multinomial(60, p[v, s] / p[v, s].sum()) for s in range(4)] for v in range(len(digits))], dtype=np.int64)
    table = str(tmp_path / "new.freq")
    names = ["N0", "N1", "N2", "N3"]
    _write_freq(table, new, names, contigs, positions)
    plain, post = str(tmp_path / "plain"), str(tmp_path / "post")
    abund.main([run, table, "-o", plain, "--interval", "0.9"])
    abund.main([run, table, "-o", post, "--interval", "0.9", "--posterior", "300", "--burn", "50"])
    assert sorted(os.listdir(post)) == sorted(os.listdir(plain) + ["Projected_posterior.csv"])
    for name in os.listdir(plain):
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(post, name), "rb").read(), name
    rt = dict(index_col=0, float_precision="round_trip")
    t = pd.read_csv(os.path.join(post, "Projected_posterior.csv"), **rt)
    assert list(t.index) == names and list(t.columns) == ["%d_%s" % (g, k) for g in range(G) for k in ("mean", "sd", "lo", "med", "hi")]
    mean = t[["%d_mean" % g for g in range(G)]].to_numpy()
    proj = pd.read_csv(os.path.join(post, "Projected_Gamma.csv"), **rt).to_numpy()
    assert np.allclose(mean.sum(axis=1), 1.0, atol=1e-12) and np.abs(mean - proj).max() < 0.02
    direct = fixed_tau.posterior_gamma(new, digits, eta_star, n_iter=300, burn=50, level=0.9)
    assert np.array_equal(direct["mean"], mean) and np.array_equal(direct["lo"][:, 0], t["0_lo"].to_numpy())
    both = str(tmp_path / "both")
    abund.main([run, table, "-o", both, "--fit-eta", "--posterior", "300", "--burn", "50", "--posterior-seed", "0x11"])
    e = pd.read_csv(os.path.join(both, "Projected_Eta_posterior.csv"), **rt)
    assert e.shape == (4, 8) and np.allclose(e[["%d_mean" % b for b in range(4)]].to_numpy().sum(axis=1), 1.0, atol=1e-12)
    assert os.path.isfile(os.path.join(both, "Projected_posterior.csv")) and not os.path.exists(os.path.join(post, "Projected_Eta_posterior.csv"))
