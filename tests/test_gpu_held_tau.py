"""The partly held chain on the GPU (dsm_ctx_sample_tau_held, dsm_ctx_gibbs_update_held_tau): one sweep and every
piece of every iteration against the oracle composition of tests/_heldtau.py, the two ends against the drivers they delegate to, the
stream accounting, recovery of a free strain and `desman-abund --novel`.
Run on an MI355X with:  python -m pytest tests/test_gpu_held_tau.py -m gpu
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fixtau as F  # noqa: E402
import _heldtau as H  # noqa: E402

from desman_amd import _lib  # noqa: E402
from desman_amd.synth import synth_counts, random_state  # noqa: E402
from oracle import cbind  # noqa: E402

pytestmark = pytest.mark.gpu
MT_SEED, CTR_SEED = 4242, 0xABCDEF0123456789           # the seeds of tests/test_gpu_parity.py: test_tau_sweep_vs_oracle and the Philox sweep


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


def _load(c, counts, tau, gamma, eta, rng=_lib.RNG_MT19937, mt_seed=MT_SEED, cseed=CTR_SEED, spec=0):
    c.set_counts(counts)
    c.set_state(tau, gamma, eta)
    c.seed(mt_seed, ctr_seed=cseed)
    c.set_tau_rng(rng)
    c.force_stats_spec(spec)


def _helds(G):
    return sorted({1, G // 2, G - 1})


# ---- 1. one sweep against the oracle composition -----------------------------------------------------------------------------------
VS, SS, GS = (1, 63, 65, 257), (1, 3, 16, 17, 33, 64, 65, 130), (2, 3, 5, 8, 12, 16)
WIDE_VS, WIDE_SS, WIDE_GS = (1, 63), (100, 200, 300, 400), (2, 3)       # the tilings SS leaves out: 64 x 2, 64 x 4, 64 x 6, 64 x 8
TILINGS = {(16, 1), (16, 2), (16, 3), (32, 2), (32, 3), (64, 2), (64, 3), (64, 4), (64, 6), (64, 8)}   # dsm_host.h: DSM_TAU_TILINGS


def test_the_sample_counts_reach_every_tiling_of_the_launcher():
    """the twin of tests/test_gpu_tau_pairs.py: test_the_shapes_reach_every_instantiation_of_the_launcher.  The held sweep has no hook of
    its own: k_held_sweep and k_pair_sweep take their tiling from the same tau_shape through the same sweep_tile_dispatch
    (dsm_sweep_tile.h), so the pair pass's pairtau_debug_path answers for both"""
    assert {_lib.pairtau_debug_path(S, 2) for S in SS + WIDE_SS} == TILINGS
    assert {_lib.pairtau_debug_path(S, 2) for S in WIDE_SS} == {(64, 2), (64, 4), (64, 6), (64, 8)}


@pytest.mark.parametrize("eta_kind", ["random", "identity", "zero-row"])
@pytest.mark.parametrize("rng", ["mt", "philox"])
@pytest.mark.parametrize("S", SS)
def test_one_held_sweep_is_the_oracle_composition(ctx, S, rng, eta_kind):
    """every V x G x n_held of the table in the issue at this S (one (lanes, samples per lane) class of tau_shape each: 16 x 1 for
    1 / 3 / 16, 16 x 2, 16 x 3, 32 x 2, 32 x 3, 64 x 3), tau array_equal and nchange equal"""
    mode = _lib.RNG_MT19937 if rng == "mt" else _lib.RNG_PHILOX
    try:
        for V in VS:
            for G in GS:
                counts, _, _ = synth_counts(V, S, max(G, 2), seed=V + S)
                tau, gamma, _ = random_state(V, S, G, seed=G)
                eta = H.etas(eta_kind, seed=G)
                for n_held in _helds(G):
                    _load(ctx, counts, tau, gamma, eta, rng=mode)
                    n = ctx.sample_tau_held(n_held)
                    got = ctx.get_state()[0]
                    Fr = G - n_held
                    u = cbind.MT19937(MT_SEED).uniform(V * Fr) if rng == "mt" else H.philox_free_uniforms(CTR_SEED, 0, V, G, n_held)
                    want, n_ref = H.held_sweep(tau, gamma, eta, counts, u, n_held)
                    where = "V=%d S=%d G=%d n_held=%d %s %s" % (V, S, G, n_held, rng, eta_kind)
                    assert np.array_equal(got[:, Fr:], tau[:, Fr:]), where
                    assert np.array_equal(got, want) and n == n_ref, where
                    assert ctx.counters() == (CTR_SEED, 1), where
    finally:
        ctx.set_tau_rng(_lib.RNG_MT19937)


@pytest.mark.parametrize("rng", ["mt", "philox"])
@pytest.mark.parametrize("S", WIDE_SS)
def test_one_held_sweep_on_the_wide_tilings(ctx, S, rng):
    """the check above on 64 x 2 / 4 / 6 / 8 (S = 100 / 200 / 300 / 400), at the smallest shapes where their grid-stride tail (V = 63: the
    last workgroup has groups beyond V), a lone group (V = 1) and their padded slots (every S here leaves some) can go wrong"""
    mode = _lib.RNG_MT19937 if rng == "mt" else _lib.RNG_PHILOX
    try:
        for V in WIDE_VS:
            for G in WIDE_GS:
                counts, _, _ = synth_counts(V, S, G, seed=V + S)
                tau, gamma, _ = random_state(V, S, G, seed=G)
                eta = H.etas("random", seed=G)
                for n_held in _helds(G):
                    _load(ctx, counts, tau, gamma, eta, rng=mode)
                    n = ctx.sample_tau_held(n_held)
                    got = ctx.get_state()[0]
                    Fr = G - n_held
                    u = cbind.MT19937(MT_SEED).uniform(V * Fr) if rng == "mt" else H.philox_free_uniforms(CTR_SEED, 0, V, G, n_held)
                    want, n_ref = H.held_sweep(tau, gamma, eta, counts, u, n_held)
                    where = "V=%d S=%d G=%d n_held=%d %s" % (V, S, G, n_held, rng)
                    assert np.array_equal(got[:, Fr:], tau[:, Fr:]), where
                    assert np.array_equal(got, want) and n == n_ref, where
                    assert ctx.counters() == (CTR_SEED, 1), where
    finally:
        ctx.set_tau_rng(_lib.RNG_MT19937)


# ---- 2. against the existing device sweep ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,S,G", [(257, 16, 5), (300, 64, 8), (130, 130, 12), (65, 33, 3)])
def test_philox_free_digits_are_those_of_the_full_device_sweep(ctx, ctx2, V, S, G):
    counts, _, _ = synth_counts(V, S, G, seed=V + S)
    tau, gamma, eta = random_state(V, S, G, seed=G)
    try:
        for n_held in _helds(G):
            _load(ctx, counts, tau, gamma, eta, rng=_lib.RNG_PHILOX)
            _load(ctx2, counts, tau, gamma, eta, rng=_lib.RNG_PHILOX)
            ctx.sample_tau_held(n_held)
            ctx2.sample_tau()
            full, (_, g2, e2) = ctx2.get_state()[0], ctx2.get_state()
            full[:, G - n_held:] = tau[:, G - n_held:]
            ctx2.set_state(full, g2, e2)                            # the held digits restored
            assert np.array_equal(ctx.get_state()[0], ctx2.get_state()[0]) and ctx.counters() == ctx2.counters()
    finally:
        ctx.set_tau_rng(_lib.RNG_MT19937); ctx2.set_tau_rng(_lib.RNG_MT19937)


# ---- 3. held digits never move ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", [_lib.RNG_MT19937, _lib.RNG_PHILOX])
@pytest.mark.parametrize("V,S,G,n_held", [(257, 17, 5, 2), (100, 65, 8, 7), (300, 3, 3, 1)])
def test_held_digits_never_move(ctx, V, S, G, n_held, rng):
    counts, _, _ = synth_counts(V, S, G, seed=70)
    tau, gamma, eta = random_state(V, S, G, seed=71)
    _load(ctx, counts, tau, gamma, eta, rng=rng)
    try:
        ctx.gibbs_update_held_tau(25, n_held)
    finally:
        ctx.set_tau_rng(_lib.RNG_MT19937)
    Fr = G - n_held
    assert np.array_equal(ctx.get_state()[0][:, Fr:], tau[:, Fr:]) and np.array_equal(ctx.get_star()["tau"][:, Fr:], tau[:, Fr:])
    assert all(np.array_equal(ctx.get_tau_at(it)[:, Fr:], tau[:, Fr:]) for it in range(-1, 25))
    assert ctx.get_trace()["nchange"].sum() > 0 and not np.array_equal(ctx.get_state()[0][:, :Fr], tau[:, :Fr])


# ---- 4. the ends --------------------------------------------------------------------------------------------------------------------
def _everything(c):
    tr, st, star = c.get_trace(), c.get_state(), c.get_star()
    out = [tr[k] for k in ("gamma", "eta", "ll", "lp", "nchange")] + list(st) + [star["tau"], star["gamma"], star["eta"], np.array([star["lp"], star["it"]])]
    return out + [c.get_mt_state(), np.array(c.counters(), dtype=np.uint64), c.get_tau_sum()] + [c.get_tau_at(it) for it in range(-1, len(tr["ll"]))]


@pytest.mark.parametrize("fix_eta", [0, 1])
@pytest.mark.parametrize("end", ["none held", "all held"])
def test_the_ends_are_the_drivers_they_delegate_to(ctx, ctx2, end, fix_eta):
    V, S, G, n = 257, 16, 4, 6
    counts, _, _ = synth_counts(V, S, G, seed=41)
    tau, gamma, eta = random_state(V, S, G, seed=42)
    _load(ctx, counts, tau, gamma, eta)
    _load(ctx2, counts, tau, gamma, eta)
    mt0 = ctx.get_mt_state()
    if end == "none held":
        ctx.gibbs_update_held_tau(n, 0, fix_eta=bool(fix_eta))
        ctx2.gibbs_update(n)
    else:
        ctx.gibbs_update_held_tau(n, G, fix_eta=bool(fix_eta))
        ctx2.gibbs_update_fixed_tau(n, fix_eta=bool(fix_eta), pool=0)
        assert np.array_equal(ctx.get_mt_state(), mt0)
    for a, b in zip(_everything(ctx), _everything(ctx2)):
        assert np.array_equal(a, b)
    # the single sweep's ends
    _load(ctx, counts, tau, gamma, eta)
    _load(ctx2, counts, tau, gamma, eta)
    if end == "none held":
        assert ctx.sample_tau_held(0) == ctx2.sample_tau() and np.array_equal(ctx.get_state()[0], ctx2.get_state()[0])
        assert np.array_equal(ctx.get_mt_state(), ctx2.get_mt_state())
    else:
        assert ctx.sample_tau_held(G) == 0 and np.array_equal(ctx.get_state()[0], tau) and np.array_equal(ctx.get_mt_state(), mt0)


# ---- 5. every piece of every iteration --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix_eta", [0, 1])
@pytest.mark.parametrize("spec", [1, 2, 3, 4])
@pytest.mark.parametrize("V,S,G,n_held", [(257, 16, 5, 2), (130, 65, 8, 7), (65, 3, 3, 1)])
def test_every_piece_of_every_iteration_against_the_oracle(ctx, V, S, G, n_held, spec, fix_eta):
    """the pattern of tests/test_gpu_parity.py: test_gibbs_update_is_self_consistent_with_oracle with the sweep replaced"""
    n_iter, Fr = 5, G - n_held
    counts, _, _ = synth_counts(V, S, G, seed=60)
    tau0, gamma0, eta0 = random_state(V, S, G, seed=61)
    cseed = 0x5EEDC0DE0000 + 16 * spec + fix_eta
    _load(ctx, counts, tau0, gamma0, eta0, mt_seed=123, cseed=cseed, spec=spec)
    try:
        ll0, lp0 = ctx.loglik()
        ctx.gibbs_update_held_tau(n_iter, n_held, fix_eta=bool(fix_eta))
    finally:
        ctx.force_stats_spec(0)
    tr, mt = ctx.get_trace(), cbind.MT19937(123)
    t_prev, g_prev, e_prev = tau0, gamma0, eta0
    lps, tau_sum = [lp0], np.zeros_like(tau0)
    assert np.array_equal(ctx.get_tau_at(-1), tau0)
    for it in range(n_iter):
        mu, E = F.stats(spec, cbind.onehot_to_idx(t_prev), g_prev, e_prev, counts, cseed, it)
        g_ref, e_ref, _ = cbind.dirichlet_counter(mu, E, cseed, it)
        np.testing.assert_allclose(tr["gamma"][it], g_ref, rtol=1e-13, atol=0)
        if fix_eta:
            assert np.array_equal(tr["eta"][it], eta0)
        else:
            np.testing.assert_allclose(tr["eta"][it], e_ref, rtol=1e-13, atol=0)
        g_it, e_it = np.ascontiguousarray(tr["gamma"][it]), np.ascontiguousarray(tr["eta"][it])
        # the sweep read the new gamma and the previous eta, and V F words of the GSL stream
        ref, n_ref = H.held_sweep(t_prev, g_it, e_prev, counts, mt.uniform(V * Fr), n_held)
        tau_it = ctx.get_tau_at(it)
        assert np.array_equal(tau_it, ref) and tr["nchange"][it] == n_ref
        idx = cbind.onehot_to_idx(tau_it)
        assert tr["ll"][it] == pytest.approx(cbind.loglik(idx, g_it, e_it, counts), rel=1e-12)
        assert tr["lp"][it] == pytest.approx(cbind.logpost(idx, g_it, e_it, counts), rel=1e-12)
        lps.append(tr["lp"][it]); tau_sum += tau_it
        t_prev, g_prev, e_prev = tau_it, g_it, e_it
    tau_f, gamma_f, eta_f = ctx.get_state()
    assert np.array_equal(tau_f, t_prev) and np.array_equal(gamma_f, tr["gamma"][-1]) and np.array_equal(eta_f, tr["eta"][-1])
    assert np.array_equal(ctx.get_tau_sum(), tau_sum) and lp0 == pytest.approx(cbind.logpost(cbind.onehot_to_idx(tau0), gamma0, eta0, counts), rel=1e-12)
    star, k = ctx.get_star(), int(np.argmax(lps))
    assert star["lp"] == lps[k]
    if k == 0:
        assert np.array_equal(star["tau"], tau0) and np.array_equal(star["gamma"], gamma0) and np.array_equal(star["eta"], eta0)
    else:
        assert np.array_equal(star["tau"], ctx.get_tau_at(k - 1)) and np.array_equal(star["gamma"], tr["gamma"][k - 1]) \
            and np.array_equal(star["eta"], tr["eta"][k - 1]) and star["it"] == k - 1
    # the relabel reductions read the same trace
    snd = ctx.trace_snd(_lib.SND_SELF)
    d = cbind.onehot_to_idx(ctx.get_tau_at(n_iter - 1)).astype(np.int64)
    assert np.array_equal(snd[-1], (d[:, :, None] != d[:, None, :]).sum(axis=0))


# ---- 6. accounting ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,S,G,n_held", [(257, 16, 5, 2), (63, 64, 8, 7)])
def test_the_gsl_stream_advances_by_n_V_F_words(ctx, V, S, G, n_held):
    n = 7
    counts, _, _ = synth_counts(V, S, G, seed=80)
    tau, gamma, eta = random_state(V, S, G, seed=81)
    _load(ctx, counts, tau, gamma, eta, mt_seed=55)
    ctx.gibbs_update_held_tau(n, n_held)
    after = ctx.debug_mt_fill(5)
    mt = cbind.MT19937(55)
    mt.raw(n * V * (G - n_held))
    assert np.array_equal(after, mt.raw(5)) and ctx.counters() == (CTR_SEED, n)
    _load(ctx, counts, tau, gamma, eta, mt_seed=55)
    ctx.sample_tau_held(n_held)
    mt = cbind.MT19937(55)
    mt.raw(V * (G - n_held))
    assert np.array_equal(ctx.debug_mt_fill(5), mt.raw(5))


@pytest.mark.parametrize("rng", [_lib.RNG_MT19937, _lib.RNG_PHILOX])
@pytest.mark.parametrize("fix_eta", [0, 1])
def test_two_calls_of_n_are_one_call_of_2n_and_runs_repeat(ctx, fix_eta, rng):
    V, S, G, n_held = 257, 16, 4, 1
    counts, _, _ = synth_counts(V, S, G, seed=41)
    tau, gamma, eta = random_state(V, S, G, seed=42)
    try:
        _load(ctx, counts, tau, gamma, eta, rng=rng)
        ctx.gibbs_update_held_tau(6, n_held, fix_eta=bool(fix_eta))
        one = _everything(ctx)
        tr_one = ctx.get_trace()
        _load(ctx, counts, tau, gamma, eta, rng=rng)
        ctx.gibbs_update_held_tau(6, n_held, fix_eta=bool(fix_eta))
        assert all(np.array_equal(a, b) for a, b in zip(one, _everything(ctx)))
        _load(ctx, counts, tau, gamma, eta, rng=rng)
        ctx.gibbs_update_held_tau(3, n_held, fix_eta=bool(fix_eta))
        a, ta = ctx.get_trace(), [ctx.get_tau_at(it) for it in range(3)]
        ctx.gibbs_update_held_tau(3, n_held, fix_eta=bool(fix_eta))
        b, tb = ctx.get_trace(), [ctx.get_tau_at(it) for it in range(3)]
    finally:
        ctx.set_tau_rng(_lib.RNG_MT19937)
    for key in ("gamma", "eta", "ll", "lp", "nchange"):
        assert np.array_equal(np.concatenate([a[key], b[key]]), tr_one[key]), key
    assert all(np.array_equal(x, y) for x, y in zip(ta + tb, one[-6:]))
    assert all(np.array_equal(x, y) for x, y in zip(ctx.get_state(), one[5:8])) and np.array_equal(ctx.get_mt_state(), one[12])


# ---- 6b. the seams of the one driver: the three forms share gibbs_update, the two single sweeps one body (api.hip) --------------------------
SEAM_SHAPE = (257, 16, 5)


def _seam_case():
    V, S, G = SEAM_SHAPE
    return synth_counts(V, S, G, seed=90)[0], random_state(V, S, G, seed=91)


@pytest.mark.parametrize("rng", [_lib.RNG_MT19937, _lib.RNG_PHILOX])
def test_forms_in_sequence_on_one_context_are_the_calls_run_alone(rng):
    """held (n_held = 2), full, fixed (pool = 0), held (n_held = 4) on one context, 7 / 7 / 3 / 7 iterations (7 sweeps cross the 1-, 2- and
    3-sweep chunks of SweepWords): after each call everything the context reports equals the same call run alone on a fresh context that was
    given the state, the MT19937 stream and the counters the first one had before the call -- nothing one form sets (words per sweep,
    tau_fixed_trace) reaches the next call"""
    counts, (tau, gamma, eta) = _seam_case()
    calls = [lambda c: c.gibbs_update_held_tau(7, 2), lambda c: c.gibbs_update(7),
             lambda c: c.gibbs_update_fixed_tau(3, pool=0), lambda c: c.gibbs_update_held_tau(7, 4)]
    a = _lib.Context(0)
    try:
        _load(a, counts, tau, gamma, eta, rng=rng)
        for i, call in enumerate(calls):
            before = a.checkpoint()
            call(a)
            b = _lib.Context(0)
            try:
                b.set_counts(counts)
                b.restore(before)
                b.set_tau_rng(rng)
                call(b)
                ea, eb = _everything(a), _everything(b)
                assert len(ea) == len(eb)
                for j, (x, y) in enumerate(zip(ea, eb)):
                    assert np.array_equal(x, y), "call %d, item %d" % (i, j)
            finally:
                b.close()
        assert a.counters() == (CTR_SEED, 24)
    finally:
        a.close()


@pytest.mark.parametrize("n_held", [0, 2, SEAM_SHAPE[2]])
def test_zero_iterations_are_gibbs_update_of_zero(ctx, ctx2, n_held):
    counts, (tau, gamma, eta) = _seam_case()
    _load(ctx, counts, tau, gamma, eta)
    _load(ctx2, counts, tau, gamma, eta)
    ctx.gibbs_update_held_tau(0, n_held)
    ctx2.gibbs_update(0)
    assert all(np.array_equal(x, y) for x, y in zip(ctx.get_state(), ctx2.get_state()))
    assert np.array_equal(ctx.get_mt_state(), ctx2.get_mt_state()) and np.array_equal(ctx.get_mt_state(), _lib.mt_seed_state(MT_SEED))
    sa, sb = ctx.get_star(), ctx2.get_star()
    assert sorted(sa) == sorted(sb) and all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert np.array_equal(sa["tau"], tau) and np.array_equal(sa["gamma"], gamma) and np.array_equal(sa["eta"], eta)
    assert ctx.counters() == (CTR_SEED, 0) and ctx2.counters() == (CTR_SEED, 0)


def test_single_sweeps_in_sequence_are_the_oracle_composition(ctx):
    """sample_tau_held(2), sample_tau(), sample_tau_held(2) on one seeded context: V (3 + 5 + 3) words of one GSL stream, in that order"""
    V, S, G = SEAM_SHAPE
    counts, (tau, gamma, eta) = _seam_case()
    _load(ctx, counts, tau, gamma, eta)
    mt = cbind.MT19937(MT_SEED)
    got = []
    n = ctx.sample_tau_held(2)
    got.append((ctx.get_state()[0], n))
    n = ctx.sample_tau()
    got.append((ctx.get_state()[0], n))
    n = ctx.sample_tau_held(2)
    got.append((ctx.get_state()[0], n))
    t1, n1 = H.held_sweep(tau, gamma, eta, counts, mt.uniform(V * 3), 2)
    t2 = t1.copy()
    n2 = cbind.sample_tau_u(t2, gamma, eta, np.ascontiguousarray(counts, dtype=np.int64), mt.uniform(V * 5))
    t3, n3 = H.held_sweep(t2, gamma, eta, counts, mt.uniform(V * 3), 2)
    want = [(t1, n1), (t2, n2), (t3, n3)]
    for i, ((tg, ng), (tw, nw)) in enumerate(zip(got, want)):
        assert np.array_equal(tg, tw) and ng == nw, "sweep %d" % i
    after = cbind.MT19937(MT_SEED)
    after.raw(V * (3 + 5 + 3))
    assert np.array_equal(ctx.debug_mt_fill(5), after.raw(5)) and ctx.counters() == (CTR_SEED, 3)


def test_error_codes():
    counts, _, _ = synth_counts(20, 3, 2, seed=1)
    c = _lib.Context(0)
    n = _lib.C.c_int(0)
    try:
        assert c.lib.dsm_ctx_gibbs_update_held_tau(c._h, 2, 1, 0) == -3              # DSM_ERR_STATE: no counts
        assert c.lib.dsm_ctx_sample_tau_held(c._h, 1, _lib.C.byref(n)) == -3
        c.set_counts(counts)
        assert c.lib.dsm_ctx_gibbs_update_held_tau(c._h, 2, 1, 0) == -3              # no state
        assert c.lib.dsm_ctx_sample_tau_held(c._h, 1, _lib.C.byref(n)) == -3
        tau, gamma, eta = random_state(20, 3, 2, seed=2)
        c.set_state(tau, gamma, eta)
        assert c.lib.dsm_ctx_gibbs_update_held_tau(c._h, -1, 1, 0) == -2             # DSM_ERR_ARG
        assert c.lib.dsm_ctx_gibbs_update_held_tau(c._h, 1, -1, 0) == -2 and c.lib.dsm_ctx_gibbs_update_held_tau(c._h, 1, 3, 0) == -2
        assert c.lib.dsm_ctx_sample_tau_held(c._h, -1, _lib.C.byref(n)) == -2 and c.lib.dsm_ctx_sample_tau_held(c._h, 3, _lib.C.byref(n)) == -2
        assert c.lib.dsm_ctx_gibbs_update_held_tau(c._h, 1, 1, 0) == -3              # MT19937 stream not seeded
        c.seed(1)
        c.gibbs_update_held_tau(0, 1)                                                # the entry state only
        assert c.get_star()["it"] == 0 and np.array_equal(c.get_star()["gamma"], gamma) and np.array_equal(c.get_state()[0], tau)
    finally:
        c.close()


def test_update_held_fills_the_samplers_stores():
    from desman_amd import sampletau
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    V, S, G, n = 120, 6, 3, 8
    counts, tau_true, _ = synth_counts(V, S, G, seed=8)
    sampletau.initRNG(); sampletau.setRNG(99)
    smp = HaploSNP_Sampler(counts, G, np.random.RandomState(2), fixed_tau=cbind.idx_to_onehot(tau_true), max_iter=n)
    smp.tau[:, 0] = cbind.idx_to_onehot(np.random.RandomState(3).randint(0, 4, size=(V, 1)))[:, 0]
    tau0 = smp.tau.copy()
    smp.update_held(2)
    assert np.array_equal(smp.tau[:, 1:], tau0[:, 1:]) and smp.nchange_store[:n].sum() > 0 and np.array_equal(smp.tau_star[:, 1:], tau0[:, 1:])
    assert np.array_equal(smp.gamma, smp.gamma_store[n - 1]) and np.array_equal(smp.eta, smp.eta_store[n - 1]) and smp.lp == smp.lp_store[n - 1]
    # the module's stream advanced by n V F words, F = 1
    assert np.array_equal(np.asarray(sampletau.getRNGState()), np.asarray(_mt_state_after(99, n * V)))


def _mt_state_after(seed, n_words):
    c = _lib.Context(0)
    try:
        c.seed(seed)
        c.debug_mt_fill(n_words)
        return c.get_mt_state()
    finally:
        c.close()


# ---- 7. recovery, end to end ------------------------------------------------------------------------------------------------------------
class _Spec2(_lib.Context):
    def set_counts(self, x):
        super().set_counts(x)
        self.force_stats_spec(H.RefCtx.spec)


def test_a_free_haplotype_recovers_the_third_strain():
    """300 positions x 12 samples, three true strains (synth_counts, each above 10 % in some sample), two of them held, one haplotype free
    from the random start of held_tau.novel_start, 60 iterations.  The restatement of tests/_heldtau.py (tests/test_held_tau_cpu.py, same
    table and seed) reaches 300 of 300 positions of the third strain in the free MAP haplotype; the GPU chain is that chain piece by piece
    (test 5) up to the 1e-13 of the gamma / eta draws, so it may leave the restatement's path at a near-tie: the bound is 285 of 300, a
    margin of 5 % of the positions below the restatement.  Measured on an MI355X: 300 of 300."""
    res, third = H.recovery_run(_Spec2)
    same = int((res["tau_star"][:, 0] == third).sum())
    print("GPU: free MAP haplotype equals the third strain in %d of %d positions" % (same, len(third)))
    assert same >= 285
    assert np.array_equal(res["tau_star"][:, 1:], H.recovery_case()[1][:, 1:])


# ---- 8. command line --------------------------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    df = pd.DataFrame(np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1), index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_desman_abund_novel(tmp_path):
    """a small synthetic run by hand (two of three strains as the run's haplotypes), then `desman-abund` with --posterior and with
    --posterior --novel 1 for four new samples that also carry the third strain"""
    from desman_amd import abund, fixed_tau, held_tau
    V, S, G = 120, 4, 3
    counts, tau, _ = synth_counts(V, S, G, seed=123)
    run = tmp_path / "run"
    run.mkdir()
    contigs, positions = ["contig%d" % (v // 50) for v in range(V)], np.arange(V) * 7 + 3
    eta = 0.96 * np.eye(4) + 0.01
    pd.DataFrame(eta).to_csv(run / "Eta_star.csv")
    held = tau[:, 1:].astype(np.int64)
    frame = pd.DataFrame(held_tau.onehot(held).reshape(V, -1), index=contigs)
    frame.insert(0, "Position", positions)
    frame.to_csv(run / "Filtered_Tau_star.csv")
    table = str(tmp_path / "new.freq")
    names = ["N0", "N1", "N2", "N3"]
    _write_freq(table, counts, names, contigs, positions)
    plain, novel = str(tmp_path / "plain"), str(tmp_path / "novel")
    common = [str(run), table, "--interval", "0.9", "--presence", "--posterior", "120", "--burn", "40", "--posterior-seed", "0x77"]
    abund.main(common + ["-o", plain])
    res = abund.main(common + ["-o", novel, "--novel", "1"])
    new = ["Novel_Gamma_posterior.csv", "Novel_Gamma_star.csv", "Novel_Tau_star.csv", "Novel_fit.csv", "Novel_haplotypes.csv"]
    assert sorted(os.listdir(novel)) == sorted(os.listdir(plain) + new)
    for name in os.listdir(plain):
        assert name.startswith("Projected_") and open(os.path.join(plain, name), "rb").read() == open(os.path.join(novel, name), "rb").read(), name
    t = pd.read_csv(os.path.join(novel, "Novel_Tau_star.csv"), header=0, index_col=0)
    inp = pd.read_csv(run / "Filtered_Tau_star.csv", header=0, index_col=0)
    assert np.array_equal(t.to_numpy()[:, 5:], inp.to_numpy()[:, 1:]) and np.array_equal(t["Position"].to_numpy(), positions)
    rt = dict(index_col=0, float_precision="round_trip")
    fit = pd.read_csv(os.path.join(novel, "Novel_fit.csv"), **rt)
    direct = fixed_tau.posterior_gamma(counts, held, eta, n_iter=120, burn=40, level=0.9, seed=0x77)
    assert list(fit.index) == [0, 1] and fit.loc[0, "deviance"] == -2.0 * direct["ll"].mean() and fit.loc[0, "lp_star"] == direct["lp_star"]
    assert fit.loc[0, "iters"] == 80 and fit.loc[1, "iters"] == 80
    assert fit.loc[1, "deviance"] < fit.loc[0, "deviance"]          # the samples carry a third strain: the free haplotype explains reads
    h = pd.read_csv(os.path.join(novel, "Novel_haplotypes.csv"), **rt)
    assert list(h.index) == ["novel0"] and h.loc["novel0", "distance"] > 0 and h.loc["novel0", "max_abundance"] > 0.05
    g = pd.read_csv(os.path.join(novel, "Novel_Gamma_posterior.csv"), **rt)
    assert list(g.index) == names and np.allclose(g[["%s_mean" % lab for lab in ("novel0", "0", "1")]].to_numpy().sum(axis=1), 1.0, atol=1e-12)
    assert np.array_equal(res["novel"]["tau_star"][:, 1:], held)
