"""The tau sweep's counter-based uniforms (dsm_ctx_set_tau_rng(DSM_RNG_PHILOX)) -- the only mode a chain sharded by positions can run --
against the C oracle's sweep fed uniforms from an independent numpy Philox (tests/_philox.py; checked on the CPU by
tests/test_philox_cpu.py).  tau and change counts bit for bit; gamma / eta to 1e-13 and ll / lp to 1e-12 relative, the tolerances of the
MT19937 twin (tests/test_gpu_parity.py: test_gibbs_update_is_self_consistent_with_oracle).

The iteration counter (api.hip: iter_ctr; dsm_ctx_seed sets it to 0, dsm_ctx_set_counters to anything): every dsm_ctx_sample_tau call,
every iteration of dsm_ctx_gibbs_update / dsm_batch_gibbs_update and every sweep of dsm_ctx_update_tau / dsm_batch_update_tau takes the
context's current value and leaves it one higher.  An iteration of the Gibbs loop uses its value three times: mu/E pass, gamma / eta
draws, sweep.

Which assertion catches what:
* a stuck iteration counter (the sweep of iteration it > 0 drawing iteration 0's uniforms): `tau of iteration` in _assert_chain_is_the_oracles
  at it >= 1, and sweeps 1, 2 of test_every_sweep_form_draws_the_oracles_uniforms;
* a dropped or swapped key word: the same assertion under the keys 0x5EEDC0DE00000001 and 0xABCDEF0100000000 (under 777 the high word is 0 and
  nothing could tell); `wrong oracle` in the same function shows that the oracle side would not agree with such a kernel either;
* a sweep form that skips the Philox branch or reads its uniforms differently: test_every_sweep_form_draws_the_oracles_uniforms (every
  tiling, screen on / off, single sweeps and the loop's instantiation), test_neartie_sweep_... (tau_kernel_nt), test_batch_... (tau_kernel_b),
  test_update_tau_... (the sweeps with the finalize rider);
* a counter that does not survive a second call: test_two_gibbs_calls_are_one_call, test_sample_tau_calls_count_up_and_the_loop_goes_on_from_there;
* a counter that does not survive a resume: test_resume_on_a_fresh_context_continues_the_chain, test_iteration_counter_above_2_to_31;
* a Philox chain that consumes the MT19937 stream: `MT19937 state` in test_gibbs_update_in_philox_mode_against_the_oracle."""
import numpy as np
import pytest

from desman_amd import _lib
from desman_amd.synth import synth_counts, random_state
from oracle import cbind

import test_gpu_parity as tp
from _philox import CTR_SEEDS, tau_uniforms, wrong_tau_uniforms

pytestmark = pytest.mark.gpu
ctx = tp.ctx                                                     # the module-scoped context fixture of the parity tests


@pytest.fixture
def pctx(ctx):
    """the shared context; whatever a test switches goes back to the defaults afterwards"""
    yield ctx
    ctx.set_tau_rng(_lib.RNG_MT19937)
    ctx.set_tau_screen(True)
    ctx.set_tau_neartie(-1)
    ctx.force_stats_spec(0)


def _load_philox(c, counts, tau, gamma, eta, cseed, mt_seed=123):
    """a fresh chain: state in, both streams seeded (iteration counter 0), the screening words of a new context, tau uniforms from Philox"""
    tp._load(c, counts, tau, gamma, eta, mt_seed=mt_seed)
    c.seed(mt_seed, ctr_seed=cseed)
    c.set_screen_state(np.zeros(2, dtype=np.uint32))
    c.set_tau_rng(_lib.RNG_PHILOX)


def _table(V, S, G, seed):
    """synthetic counts in which every fourth position, the last one among them, has no reads.  With tens of reads in every sample nearly every step's conditional is
    all but certain and a sweep hardly depends on its uniforms (two streams end on the same haplotypes but for a handful of steps:
    tests/test_philox_cpu.py); at a position without reads the four bases are equally likely and the uniform alone decides, in every sweep
    of a chain -- these positions are what tells one stream from another."""
    counts, tau_true, gamma_true = synth_counts(V, S, G, seed=seed)
    counts[(V - 1) % 4::4] = 0
    return counts, tau_true, gamma_true


def _set_counters(c, cseed, it):
    _lib.check(c.lib.dsm_ctx_set_counters(c._h, int(cseed), int(it)))


def _oracle_sweep(tau, gamma, eta, counts, cseed, ic):
    """in place: the oracle's sweep with the uniforms of iteration counter ic; returns the change count"""
    V, G = tau.shape[:2]
    return cbind.sample_tau_u(tau, np.ascontiguousarray(gamma), np.ascontiguousarray(eta), counts, tau_uniforms(cseed, ic, V, G))


def _assert_chain_is_the_oracles(c, counts, start, cseed, ic0, n_iter, spec, lp0=None, wrong=False):
    """The n_iter iterations context c has just run from `start` with iteration counters ic0, ic0 + 1, ... against the oracle, piece by
    piece in the reference's order (HaploSNP_Sampler.py:341-358), as the MT19937 twin does: mu/E sums + gamma / eta draws (specification
    `spec`), the sweep with (gamma_new, eta_old) and the Philox uniforms of the iteration's counter, ll / lp; with lp0 (log-posterior of
    the entry state) also final state, tau sum and MAP record.  wrong=True: the three wrong oracles of tests/_philox.py must each
    disagree with the device in one of the first two iterations."""
    tau0, gamma0, eta0 = start
    V, G = tau0.shape[:2]
    tr = c.get_trace()
    taus = [c.get_tau_at(it) for it in range(n_iter)]
    g_prev, e_prev, t_prev = gamma0, eta0, tau0
    for it in range(n_iter):
        args = (cbind.onehot_to_idx(t_prev), np.ascontiguousarray(g_prev), np.ascontiguousarray(e_prev), counts, cseed, ic0 + it)
        mu, E = cbind.stats_agg(*args, spec=spec) if spec >= 2 else cbind.stats_counter(*args)
        g_ref, e_ref, _ = cbind.dirichlet_counter(mu, E, cseed, ic0 + it)
        np.testing.assert_allclose(tr["gamma"][it], g_ref, rtol=1e-13, atol=0)
        np.testing.assert_allclose(tr["eta"][it], e_ref, rtol=1e-13, atol=0)
        g_prev, e_prev, t_prev = tr["gamma"][it], tr["eta"][it], taus[it]
    tau_prev, eta_prev = tau0.copy(), np.array(eta0)
    lps = [lp0]
    tau_sum = np.zeros_like(tau0)
    fooled = {}
    for it in range(n_iter):
        ref = tau_prev.copy()
        n_ref = _oracle_sweep(ref, tr["gamma"][it], eta_prev, counts, cseed, ic0 + it)
        assert np.array_equal(taus[it], ref), "tau of iteration %d (counter %d)" % (it, ic0 + it)
        assert tr["nchange"][it] == n_ref
        if wrong and it < 2:
            for name, u in wrong_tau_uniforms(cseed, ic0 + it, V, G).items():
                other = tau_prev.copy()
                cbind.sample_tau_u(other, np.ascontiguousarray(tr["gamma"][it]), np.ascontiguousarray(eta_prev), counts, u)
                fooled[name] = fooled.get(name, True) and np.array_equal(other, taus[it])
        idx = cbind.onehot_to_idx(taus[it])
        g_it, e_it = np.ascontiguousarray(tr["gamma"][it]), np.ascontiguousarray(tr["eta"][it])
        assert tr["ll"][it] == pytest.approx(cbind.loglik(idx, g_it, e_it, counts), rel=1e-12)
        assert tr["lp"][it] == pytest.approx(cbind.logpost(idx, g_it, e_it, counts), rel=1e-12)
        np.testing.assert_allclose(g_it.sum(axis=1), 1.0, rtol=1e-12)
        lps.append(tr["lp"][it]); tau_sum += taus[it]
        tau_prev, eta_prev = taus[it], e_it
    assert not any(fooled.values()), "wrong oracle agrees with the device: %s" % fooled
    assert not wrong or cseed != CTR_SEEDS[0] or len(fooled) == 3      # (the first key tells all three mistakes)
    if lp0 is None:
        return
    tau_f, gamma_f, eta_f = c.get_state()
    assert np.array_equal(tau_f, tau_prev) and np.array_equal(gamma_f, tr["gamma"][-1]) and np.array_equal(eta_f, tr["eta"][-1])
    assert np.array_equal(c.get_tau_sum(), tau_sum)
    star = c.get_star()
    k = int(np.argmax(lps))                                       # first strict maximum, entry state = slot 0
    assert star["lp"] == lps[k]
    if k == 0:
        assert np.array_equal(star["tau"], tau0) and np.array_equal(star["gamma"], gamma0)
    else:
        assert np.array_equal(star["tau"], taus[k - 1]) and np.array_equal(star["gamma"], tr["gamma"][k - 1]) \
            and np.array_equal(star["eta"], tr["eta"][k - 1]) and star["it"] == k - 1


# ---------------------------------------------------------------- (a) the whole loop
_LOOP_CASES = [(V, S, G, n, spec) for V, S, G, n in [(400, 16, 5, 8), (300, 64, 8, 5), (150, 96, 3, 4), (200, 20, 11, 4)] for spec in (2, 1)] + \
              [(900, 10, 2, 4, 4)]


@pytest.mark.parametrize("cseed", CTR_SEEDS, ids=["%#x" % s for s in CTR_SEEDS])
@pytest.mark.parametrize("V,S,G,n_iter,spec", _LOOP_CASES)
def test_gibbs_update_in_philox_mode_against_the_oracle(pctx, V, S, G, n_iter, spec, cseed):
    """every piece of every iteration of the device loop in Philox mode against the oracle; iteration it of the first call after
    dsm_ctx_seed runs under counter it (api.hip: gibbs_update, ic[k] = c->iter_ctr++).  The chain leaves the MT19937 stream alone."""
    c = pctx
    counts, _, _ = _table(V, S, G, seed=60)
    start = random_state(V, S, G, seed=61)
    _load_philox(c, counts, *start, cseed)
    c.force_stats_spec(spec)
    assert c.stats_spec() == spec
    assert c.counters() == (cseed, 0)
    mt_before = c.get_mt_state()
    _, lp0 = c.loglik()
    c.gibbs_update(n_iter)
    assert c.counters() == (cseed, n_iter)
    assert np.array_equal(c.get_mt_state(), mt_before), "MT19937 state"
    assert np.array_equal(mt_before, _lib.mt_seed_state(123))
    _assert_chain_is_the_oracles(c, counts, start, cseed, 0, n_iter, spec, lp0=lp0, wrong=True)


# ---------------------------------------------------------------- (b) the counter across calls
_B = (200, 16, 4)


def _b_case():
    V, S, G = _B
    counts, _, _ = _table(V, S, G, seed=62)
    return counts, random_state(V, S, G, seed=63)


def _snapshot(c, n):
    tr = c.get_trace()
    return dict(tr, taus=np.array([c.get_tau_at(i) for i in range(n)]), state=c.get_state())


def _assert_same_run(whole, parts):
    """the traces of consecutive calls, put end to end, are the trace of the one call; so is the state they end in"""
    for k in ("ll", "lp", "nchange", "gamma", "eta", "taus"):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts])), k
    assert all(np.array_equal(a, b) for a, b in zip(whole["state"], parts[-1]["state"]))


def test_two_gibbs_calls_are_one_call(pctx):
    """gibbs_update(3) + gibbs_update(4) = gibbs_update(7): the second call goes on at counter 3"""
    c = pctx
    counts, start = _b_case()
    cseed = CTR_SEEDS[0]
    _load_philox(c, counts, *start, cseed)
    c.gibbs_update(7)
    whole = _snapshot(c, 7)
    assert c.counters() == (cseed, 7)
    _load_philox(c, counts, *start, cseed)
    c.gibbs_update(3)
    first = _snapshot(c, 3)
    assert c.counters() == (cseed, 3)
    c.gibbs_update(4)
    second = _snapshot(c, 4)
    assert c.counters() == (cseed, 7)
    _assert_same_run(whole, [first, second])
    _assert_chain_is_the_oracles(c, counts, first["state"], cseed, 3, 4, c.stats_spec())


def test_sample_tau_calls_count_up_and_the_loop_goes_on_from_there(pctx):
    """three dsm_ctx_sample_tau calls run under counters 0, 1, 2 (api.hip: c->iter_ctr++ in the call); a Gibbs call after them starts at 3"""
    c = pctx
    V, S, G = _B
    counts, (tau, gamma, eta) = _b_case()
    cseed = CTR_SEEDS[0]
    _load_philox(c, counts, tau, gamma, eta, cseed)
    ref = tau.copy()
    for k in range(3):
        assert c.counters() == (cseed, k)
        n_ref = _oracle_sweep(ref, gamma, eta, counts, cseed, k)
        n = c.sample_tau()
        assert n == n_ref and np.array_equal(c.get_state()[0], ref), k
    assert c.counters() == (cseed, 3)
    c.gibbs_update(2)
    assert c.counters() == (cseed, 5)
    _assert_chain_is_the_oracles(c, counts, (ref, gamma, eta), cseed, 3, 2, c.stats_spec())
    # ... and single sweeps after the loop at 5
    t, g, e = c.get_state()
    n_ref = _oracle_sweep(t, g, e, counts, cseed, 5)
    assert c.sample_tau() == n_ref and np.array_equal(c.get_state()[0], t)
    assert c.counters() == (cseed, 6)


def test_resume_on_a_fresh_context_continues_the_chain(pctx):
    """checkpoint / resume by hand: counters, state and screening words of a chain after 3 iterations, put into a fresh context that was
    never seeded (a Philox chain needs no MT19937 stream), continue the chain bit for bit -- and both are the oracle's at counters 3 .. 6"""
    c = pctx
    counts, start = _b_case()
    cseed = CTR_SEEDS[1]
    _load_philox(c, counts, *start, cseed)
    c.gibbs_update(3)
    key, it = c.counters()
    assert (key, it) == (cseed, 3)
    state, screen = c.get_state(), c.screen_state()
    spec = c.stats_spec()
    c.gibbs_update(4)
    went_on = _snapshot(c, 4)
    f = _lib.Context(0)
    try:
        f.set_counts(counts)
        f.set_tau_rng(_lib.RNG_PHILOX)
        _set_counters(f, key, it)
        f.set_state(*state)
        f.set_screen_state(screen)
        assert f.counters() == (cseed, 3) and f.stats_spec() == spec
        f.gibbs_update(4)
        assert f.counters() == (cseed, 7)
        _assert_same_run(went_on, [_snapshot(f, 4)])
        _assert_chain_is_the_oracles(f, counts, state, cseed, 3, 4, spec)
    finally:
        f.close()


def test_iteration_counter_above_2_to_31(pctx):
    """dsm_ctx_set_counters(key, 3 000 000 000): the counter word is unsigned all the way into the kernel"""
    c = pctx
    counts, (tau, gamma, eta) = _b_case()
    cseed, it = CTR_SEEDS[0], 3_000_000_000
    _load_philox(c, counts, tau, gamma, eta, cseed)
    _set_counters(c, cseed, it)
    assert c.counters() == (cseed, it)
    ref = tau.copy()
    n_ref = _oracle_sweep(ref, gamma, eta, counts, cseed, it)
    assert c.sample_tau() == n_ref and np.array_equal(c.get_state()[0], ref)
    assert c.counters() == (cseed, it + 1)
    signed = tau.copy()                                           # (what a sign-extended or 31-bit counter would have drawn is something else)
    cbind.sample_tau_u(signed, gamma, eta, counts, tau_uniforms(cseed, it - 2 ** 31, *tau.shape[:2]))
    assert not np.array_equal(signed, ref)


# ---------------------------------------------------------------- (c) every sweep form
# the lane-group widths, haplotype counts and position counts of the fuzz edges (tests/test_gpu_fuzz.py: _gibbs_shapes): every (lanes per
# variant, samples per lane) tiling of the sweep, its register-lean forms included, ragged last samples, one / many workgroups
_FORM_SHAPES = [(150, S, 4) for S in (1, 16, 17, 33, 48, 65, 97, 129, 193, 257, 385)] + [(150, 24, G) for G in (1, 9, 16, 17, 32)] + \
               [(V, 64, 8) for V in (1, 3, 257)]


@pytest.mark.parametrize("screen", [True, False], ids=["screen", "fp64"])
@pytest.mark.parametrize("V,S,G", _FORM_SHAPES)
def test_every_sweep_form_draws_the_oracles_uniforms(pctx, V, S, G, screen):
    """three consecutive single sweeps (the sweep-only instantiation of the kernel, counters 0, 1, 2), then two sweeps of the tau-only
    loop (the instantiation the Gibbs loop runs, counters 3, 4), with the fp32 screen and without: the oracle's haplotypes exactly"""
    c = pctx
    counts, _, _ = _table(V, S, max(G, 2), seed=V + S)
    tau, gamma, eta = random_state(V, S, G, seed=G)
    cseed = CTR_SEEDS[0]
    _load_philox(c, counts, tau, gamma, eta, cseed)
    c.set_tau_screen(screen)
    ref = tau.copy()
    for k in range(3):
        n_ref = _oracle_sweep(ref, gamma, eta, counts, cseed, k)
        n = c.sample_tau()
        assert n == n_ref and np.array_equal(c.get_state()[0], ref), k
    assert c.counters() == (cseed, 3)
    c.update_tau(np.ascontiguousarray(np.broadcast_to(gamma, (2,) + gamma.shape)), np.ascontiguousarray(np.broadcast_to(eta, (2, 4, 4))))
    tr = c.get_trace()
    for k in range(2):
        n_ref = _oracle_sweep(ref, gamma, eta, counts, cseed, 3 + k)
        assert np.array_equal(c.get_tau_at(k), ref) and tr["nchange"][k] == n_ref, 3 + k
    assert c.counters() == (cseed, 5)


def test_neartie_sweep_draws_the_oracles_uniforms(pctx):
    """tau_kernel_nt, the Gibbs loop's instantiation with the screen on the differences of the candidates (the twin on the MT19937
    stream: test_gibbs_loop_with_the_neartie_sweep_is_the_same_chain): forced on, forced off or chosen by the chain's abundances the
    Philox chain is the same chain and its sweeps are the oracle's at counters 0, 1, 2.  Single sweeps never run this kernel
    (kernels_gibbs.hip: launch_tau), so this case runs the loop.  Forced on, it leaves fewer steps to fp64 than the totals screen alone:
    the near-tie path did decide steps."""
    c = pctx
    V, S, G, spare, scale = 400, 64, 8, (2, 5, 7), 1e-3
    live = [g for g in range(G) if g not in spare]
    counts, tau_true, gamma_true = _table(V, S, len(live), seed=V + G)
    rng = np.random.default_rng(V + S)
    # a settled over-fitted state: the live haplotypes carry the generating tau, the spare ones random bases at abundances <= 2e-3 in every sample
    tau_idx = rng.integers(0, 4, size=(V, G)).astype(np.uint8)
    tau_idx[:, live] = tau_true[:, :len(live)]
    tau = cbind.idx_to_onehot(tau_idx)
    gamma = np.full((S, G), 0.0)
    gamma[:, list(spare)] = rng.uniform(0.2 * scale, 2.0 * scale, size=(S, len(spare)))
    gamma[:, live] = gamma_true[:, :len(live)] * (1.0 - gamma[:, list(spare)].sum(axis=1))[:, None] / gamma_true[:, :len(live)].sum(axis=1)[:, None]
    gamma = np.ascontiguousarray(gamma / gamma.sum(axis=1)[:, None])
    assert gamma[:, list(spare)].max() <= 0.01
    eta = 0.96 * np.eye(4) + 0.01
    cseed, n_it = CTR_SEEDS[0], 3
    runs = {}
    for mode in (1, 0, -1):
        _load_philox(c, counts, tau, gamma, eta, cseed)
        c.force_stats_spec(2)
        c.set_tau_neartie(mode)
        c.sweep_stats(reset=True)
        c.gibbs_update(n_it)
        runs[mode] = dict(_snapshot(c, n_it), star=c.get_star(), stats=c.sweep_stats())
        _assert_chain_is_the_oracles(c, counts, (tau, gamma, eta), cseed, 0, n_it, 2)
    for mode in (0, -1):
        _assert_same_run(runs[1], [runs[mode]])
        assert runs[1]["star"]["lp"] == runs[mode]["star"]["lp"] and np.array_equal(runs[1]["star"]["tau"], runs[mode]["star"]["tau"])
    (st0, ex0), (st1, ex1) = runs[0]["stats"], runs[1]["stats"]
    print("near-tie sweep: wavefront-steps %d, left to fp64 without / with the near-tie screen %d / %d" % (st1, ex0, ex1))
    assert st0 == st1 > 0
    assert ex1 < ex0, (ex0, ex1, st1)                             # steps the totals left open were decided on the differences
    assert runs[-1]["stats"] == runs[1]["stats"]                  # the abundances of such a state switch it on by themselves


# ---------------------------------------------------------------- (d) batch
def test_batch_of_philox_chains(pctx):
    """dsm_batch_gibbs_update (tau_kernel_b: chain = blockIdx.y, each with its own key and counter) over three Philox chains with different
    keys: every chain is the chain its context runs alone, and chain 0 is the oracle's"""
    V, S, G, K, n_iter = 200, 64, 8, 3, 5
    counts, _, _ = _table(V, S, G, seed=64)
    starts = [random_state(V, S, G, seed=65 + k) for k in range(K)]
    single = []
    for k in range(K):
        _load_philox(pctx, counts, *starts[k], CTR_SEEDS[k], mt_seed=200 + k)
        pctx.gibbs_update(n_iter)
        single.append(dict(_snapshot(pctx, n_iter), lp_star=pctx.get_star()["lp"]))
    cs = [_lib.Context(0) for _ in range(K)]
    try:
        for k, c in enumerate(cs):
            _load_philox(c, counts, *starts[k], CTR_SEEDS[k], mt_seed=200 + k)
        spec = cs[0].stats_spec()
        _, lp0 = cs[0].loglik()
        _lib.Context.batch_gibbs_update(cs, n_iter)
        for k, c in enumerate(cs):
            assert c.counters() == (CTR_SEEDS[k], n_iter)
            _assert_same_run(single[k], [_snapshot(c, n_iter)])
            assert c.get_star()["lp"] == single[k]["lp_star"]
            assert np.array_equal(c.get_mt_state(), _lib.mt_seed_state(200 + k)), "MT19937 state"
        _assert_chain_is_the_oracles(cs[0], counts, starts[0], CTR_SEEDS[0], 0, n_iter, spec, lp0=lp0, wrong=True)
    finally:
        for c in cs:
            c.close()


# ---------------------------------------------------------------- (e) updateTau
def test_update_tau_in_philox_mode(pctx):
    """updateTau (tau-only sweeps over stored traces) in Philox mode: sweep it of the call runs under counter (counter at entry) + it --
    here 1 + it, after one single sweep --, alone and as a batch of two"""
    V, S, G = _B
    n = 5
    counts, (tau0, gamma0, eta0) = _b_case()
    rng = np.random.default_rng(1)
    gs = np.ascontiguousarray(rng.dirichlet(np.ones(G), size=(n, S)))
    es = np.ascontiguousarray(np.stack([random_state(1, 1, 1, seed=k)[2] for k in range(n)]))
    want = []
    for cseed in CTR_SEEDS[:2]:
        c = pctx
        _load_philox(c, counts, tau0, gamma0, eta0, cseed)
        ref = tau0.copy()
        assert c.sample_tau() == _oracle_sweep(ref, gamma0, eta0, counts, cseed, 0)
        mt_before = c.get_mt_state()
        c.update_tau(gs, es)
        assert c.counters() == (cseed, 1 + n)
        assert np.array_equal(c.get_mt_state(), mt_before), "MT19937 state"
        tr = c.get_trace()
        lp_best, tau_best = cbind.logpost(cbind.onehot_to_idx(ref), gs[0], es[0], counts), ref.copy()
        for it in range(n):
            n_ref = _oracle_sweep(ref, gs[it], es[it], counts, cseed, 1 + it)
            assert np.array_equal(c.get_tau_at(it), ref) and tr["nchange"][it] == n_ref, it
            lp = cbind.logpost(cbind.onehot_to_idx(ref), gs[it], es[it], counts)
            assert tr["lp"][it] == pytest.approx(lp, rel=1e-12)
            assert tr["ll"][it] == pytest.approx(cbind.loglik(cbind.onehot_to_idx(ref), gs[it], es[it], counts), rel=1e-12)
            if lp > lp_best:
                lp_best, tau_best = lp, ref.copy()
        star = c.get_star()
        assert np.array_equal(star["tau"], tau_best) and star["lp"] == pytest.approx(lp_best, rel=1e-12)
        want.append(dict(_snapshot(c, n), lp_star=star["lp"]))
    cs = [_lib.Context(0) for _ in range(2)]
    try:
        for c, cseed in zip(cs, CTR_SEEDS[:2]):
            _load_philox(c, counts, tau0, gamma0, eta0, cseed)
            c.sample_tau()
        _lib.Context.batch_update_tau(cs, [gs, gs], [es, es])
        for k, c in enumerate(cs):
            assert c.counters() == (CTR_SEEDS[k], 1 + n)
            _assert_same_run(want[k], [_snapshot(c, n)])
            assert c.get_star()["lp"] == want[k]["lp_star"]
    finally:
        for c in cs:
            c.close()
