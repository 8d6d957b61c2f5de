"""The tau sweep at two samples per lane of a 32-lane group (48 < S <= 64: kernels_gibbs.hip, tau_shape) in its register-lean form
(tau_body: LEAN): the prefix of the rest mixture carried in fp32, the counts kept as (float)count, the rare fp64 step re-doing its links
h < g one candidate at a time.  Everything here is against the oracle's C sweep bit for bit (tau, change counts); log-probabilities to
the tolerance of tests/test_gpu_parity.py (rtol 1e-12, atol 1e-8: lane-parallel summation order + device log vs libm).

Shapes: S = 64 has no padded slot, S = 49 fifteen (one slot past what the 16 x 3 tile holds); V = 37 is no multiple of the eight positions
of a workgroup -- the last workgroup holds five, its third wavefront one live 32-lane group next to an idle one, its fourth none;
V = 101 (the fp64-step test) likewise ends in a part-filled workgroup."""
import numpy as np
import pytest

from desman_amd import _lib
from desman_amd.synth import synth_counts, random_state
from oracle import cbind

import test_gpu_parity as tp
import test_gpu_philox as tph
import test_gpu_batch as tb

pytestmark = pytest.mark.gpu
ctx = tp.ctx                                                     # the module-scoped context fixture of the parity tests

MT, PHILOX = _lib.RNG_MT19937, _lib.RNG_PHILOX
CSEED = tph.CTR_SEEDS[0]                                         # (both key words non-zero)
MT_SEED = 4242


@pytest.fixture
def lctx(ctx):
    """the shared context; whatever a test switches goes back to the defaults afterwards"""
    yield ctx
    ctx.set_tau_rng(MT)
    ctx.set_tau_screen(True)
    ctx.set_tau_neartie(-1)
    ctx.force_stats_spec(0)


def _load(c, counts, tau, gamma, eta, rng):
    """a fresh chain on either tau stream: both generators seeded (iteration counter 0), the screening words of a new context"""
    tph._load_philox(c, counts, tau, gamma, eta, CSEED, mt_seed=MT_SEED)
    c.set_tau_rng(rng)


class _Uniforms:
    """the uniforms the device's sweeps draw, sweep after sweep: the MT19937 stream carries over, Philox is keyed by the sweep's counter"""

    def __init__(self, rng, V, G):
        self.rng, self.V, self.G, self.k = rng, V, G, 0
        self.mt = cbind.MT19937(MT_SEED)

    def next(self):
        u = self.mt.uniform(self.V * self.G) if self.rng == MT else tph.tau_uniforms(CSEED, self.k, self.V, self.G)
        self.k += 1
        return u


def _overfitted(V, S, G, rare, floor, seed):
    """a table of len(live) strains under a state with G haplotypes: the spare ones at gamma ~ 1e-3 (rare) or at the 1e-6 floor in every
    sample, as tests/test_gpu_parity.py: test_tau_sweep_of_an_overfitted_chain_vs_oracle builds them.  The steps of a spare haplotype are
    near-ties the screening pass leaves to the fp64 code; those of the live ones, from a random tau, are wide races it settles."""
    spare = sorted(rare + floor)
    live = [g for g in range(G) if g not in spare]
    counts, _, _ = synth_counts(V, S, max(len(live), 2), seed=seed)
    tau, gamma, eta = random_state(V, S, G, seed=seed + 100)
    gamma = gamma.copy()
    rng = np.random.default_rng(seed)
    gamma[:, list(rare)] = rng.uniform(2.0e-4, 2.0e-3, size=(S, len(rare)))
    gamma[:, list(floor)] = 1.0e-6
    gamma[:, live] *= ((1.0 - gamma[:, spare].sum(axis=1)) / gamma[:, live].sum(axis=1))[:, None]
    gamma = np.ascontiguousarray(gamma / gamma.sum(axis=1)[:, None])
    return counts, tau, gamma, eta


def _sweeps_vs_oracle(c, counts, tau, gamma, eta, rng, n_loop=2):
    """two single sweeps (dsm_ctx_sample_tau: no epilogue) and n_loop sweeps of the tau-only loop (dsm_ctx_update_tau: the fused launch,
    whose finalize step keeps the step counts) from a fresh chain, each against the oracle's sweep; -> (the last tau, wavefront-steps of
    the loop's sweeps, of which left to the fp64 code)"""
    V, G = tau.shape[:2]
    _load(c, counts, tau, gamma, eta, rng)
    c.sweep_stats(reset=True)
    us = _Uniforms(rng, V, G)
    ref = tau.copy()
    for sweep in range(2):
        n_ref = cbind.sample_tau_u(ref, gamma, eta, counts, us.next())
        n = c.sample_tau()
        assert n == n_ref, sweep
        assert np.array_equal(c.get_state()[0], ref), sweep
    gs = np.ascontiguousarray(np.broadcast_to(gamma, (n_loop,) + gamma.shape))
    es = np.ascontiguousarray(np.broadcast_to(eta, (n_loop, 4, 4)))
    c.update_tau(gs, es)
    nch = c.get_trace()["nchange"]
    for it in range(n_loop):
        n_ref = cbind.sample_tau_u(ref, gamma, eta, counts, us.next())
        assert np.array_equal(c.get_tau_at(it), ref) and nch[it] == n_ref, it
    steps, exact = c.sweep_stats()
    return ref, steps, exact


# ---------------------------------------------------------------- the sweep against the oracle
@pytest.mark.parametrize("rng", [MT, PHILOX], ids=["mt19937", "philox"])
@pytest.mark.parametrize("G", [1, 2, 8])
@pytest.mark.parametrize("S", [49, 64])
def test_sweep_vs_oracle(lctx, S, G, rng):
    V = 37
    c = lctx
    counts, _, _ = synth_counts(V, S, max(G, 2), seed=V + S)
    tau, gamma, eta = random_state(V, S, G, seed=G)
    _, steps, exact = _sweeps_vs_oracle(c, counts, tau, gamma, eta, rng)
    assert steps > 0 and exact < steps, (steps, exact)            # (the screened path ran)


# ---------------------------------------------------------------- the fp64 step inside the lean form
@pytest.mark.parametrize("rng", [MT, PHILOX], ids=["mt19937", "philox"])
@pytest.mark.parametrize("S", [49, 64])
def test_fp64_steps_between_screened_steps(lctx, S, rng):
    """Haplotype 2 (gamma ~ 1e-3) sits between live ones: screened step, fp64 step -- which rebuilds the links h < g the fp32 prefix
    stands for -- screened step.  Haplotypes 5 (at the floor) and 6 (~ 1e-3) follow each other: the second fp64 step takes over the
    log-probability of the current configuration (have_cur / l_cur) and evaluates three candidates in the rotated order, each 32-lane
    group of the wavefront with its own current base."""
    V, G = 101, 8
    c = lctx
    counts, tau, gamma, eta = _overfitted(V, S, G, rare=[2, 6], floor=[5], seed=V + S + G)
    ref, steps, exact = _sweeps_vs_oracle(c, counts, tau, gamma, eta, rng)
    print("wavefront-steps %d, of which fp64 %d" % (steps, exact))
    assert 0 < exact < steps, (steps, exact)                      # both kinds of step occurred
    # the screen off: every step is an fp64 step, and the same haplotypes
    c.set_tau_screen(False)
    off, _, _ = _sweeps_vs_oracle(c, counts, tau, gamma, eta, rng)
    assert np.array_equal(off, ref)
    c.set_tau_screen(True)
    # with the log-probabilities asked for (every step fp64 as well): the oracle's, and the same draws
    _load(c, counts, tau, gamma, eta, rng)
    us = _Uniforms(rng, V, G)
    ref = tau.copy()
    for sweep in range(2):
        n_ref, logp_ref = cbind.sample_tau_u(ref, gamma, eta, counts, us.next(), want_logp=True)
        n, logp = c.sample_tau(want_logp=True)
        assert n == n_ref and np.array_equal(c.get_state()[0], ref), sweep
        np.testing.assert_allclose(logp, logp_ref, rtol=1e-12, atol=1e-8)


# ---------------------------------------------------------------- the other entry points of the same body, S = 64, V = 37, G = 8
_E = (37, 64, 8)


def test_neartie_instantiation_on_and_off(lctx):
    """tau_kernel_nt<32, 2> and tau_kernel<32, 2, true, true> in the Gibbs loop: the same chain, and its sweeps are the oracle's"""
    V, S, G = _E
    c = lctx
    counts, tau, gamma, eta = _overfitted(V, S, G, rare=[2, 6], floor=[5], seed=11)
    n_it = 3
    runs = {}
    for mode in (0, 1):
        _load(c, counts, tau, gamma, eta, MT)
        c.force_stats_spec(2)
        c.set_tau_neartie(mode)
        c.gibbs_update(n_it)
        runs[mode] = dict(tr=c.get_trace(), taus=[c.get_tau_at(i) for i in range(n_it)])
    for k in ("gamma", "eta", "ll", "lp", "nchange"):
        assert np.array_equal(runs[0]["tr"][k], runs[1]["tr"][k]), k
    assert all(np.array_equal(a, b) for a, b in zip(runs[0]["taus"], runs[1]["taus"]))
    mt = cbind.MT19937(MT_SEED)
    ref, eta_prev = tau.copy(), eta
    for it in range(n_it):                                        # tau_it from (tau_{it-1}, gamma_it, eta_{it-1})
        n_ref = cbind.sample_tau_u(ref, np.ascontiguousarray(runs[1]["tr"]["gamma"][it]), np.ascontiguousarray(eta_prev), counts, mt.uniform(V * G))
        assert np.array_equal(runs[1]["taus"][it], ref) and runs[1]["tr"]["nchange"][it] == n_ref, it
        eta_prev = runs[1]["tr"]["eta"][it]


def test_sweep_only_and_likelihood_only_launches_equal_the_fused_launch(lctx):
    """The fused launch (sweep + log-likelihood epilogue: dsm_ctx_update_tau) against the sweep without the epilogue (dsm_ctx_sample_tau)
    followed by the likelihood-only pass (dsm_ctx_loglik): the same haplotypes, and the same log-likelihood bit for bit -- the epilogue
    is one piece of code over the same integer counts (which the lean sweep loads a second time), the same workgroups, the same order."""
    V, S, G = _E
    n = 4
    c = lctx
    counts, _, _ = synth_counts(V, S, G, seed=80)
    tau0, gamma0, eta0 = random_state(V, S, G, seed=81)
    rng = np.random.default_rng(1)
    gs = np.ascontiguousarray(rng.dirichlet(np.ones(G), size=(n, S)))
    es = np.ascontiguousarray(np.stack([random_state(1, 1, 1, seed=k)[2] for k in range(n)]))
    _load(c, counts, tau0, gamma0, eta0, MT)
    c.update_tau(gs, es)
    tr = c.get_trace()
    fused = [c.get_tau_at(it) for it in range(n)]
    _load(c, counts, tau0, gamma0, eta0, MT)
    t = tau0
    mt = cbind.MT19937(MT_SEED)
    ref = tau0.copy()
    for it in range(n):
        c.set_state(t, gs[it], es[it])
        c.sample_tau()
        t = c.get_state()[0]
        cbind.sample_tau_u(ref, gs[it], es[it], counts, mt.uniform(V * G))
        assert np.array_equal(t, fused[it]) and np.array_equal(t, ref), it
        ll, lp = c.loglik()
        print("sweep %d: ll %.17g, fused %.17g" % (it, ll, tr["ll"][it]))
        assert ll == tr["ll"][it], it
        assert ll == pytest.approx(cbind.loglik(cbind.onehot_to_idx(ref), gs[it], es[it], counts), rel=1e-12)


def test_batch_of_two_equals_the_chains_run_singly():
    """tau_kernel_b<32, 2, true, true>: chain = blockIdx.y"""
    V, S, G = _E
    n_it = 4
    counts, _, _ = synth_counts(V, S, G, seed=500 + V)
    states = [random_state(V, S, G, seed=600 + k) for k in range(2)]
    single = []
    for k in range(2):
        a = tb._chain(counts, states[k], 1000 + k, 0xB47C4000 + k)
        a.gibbs_update(n_it)
        single.append(tb._snapshot(a))
        a.close()
    ctxs = [tb._chain(counts, states[k], 1000 + k, 0xB47C4000 + k) for k in range(2)]
    _lib.Context.batch_gibbs_update(ctxs, n_it)
    try:
        for k in range(2):
            tb._same(single[k], tb._snapshot(ctxs[k]))
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------- a short chain
@pytest.mark.parametrize("rng", [MT, PHILOX], ids=["mt19937", "philox"])
def test_short_chain_vs_oracle(lctx, rng):
    """ten iterations at (200, 64, 8), every piece of every iteration against the oracle: the chain parity tests of
    tests/test_gpu_parity.py and tests/test_gpu_philox.py at this tiling"""
    V, S, G, n_iter, spec = 200, 64, 8, 10, 2
    if rng == MT:
        tp.test_gibbs_update_is_self_consistent_with_oracle(lctx, V, S, G, n_iter, spec)
    else:
        tph.test_gibbs_update_in_philox_mode_against_the_oracle(lctx, V, S, G, n_iter, spec, CSEED)
