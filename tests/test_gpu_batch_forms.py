"""Every batched kernel form of the Gibbs loop (dsm_batch_gibbs_update, dsm_batch_update_tau) against the chains run one by one, bit for
bit.  A batch does not run the kernels a single chain runs: every launch of the iteration has a twin that is compiled on its own and
reached only with g_batch.K > 0 (tau_kernel_b, stats_agg_kernel_b, stats_pat_kernel_b, stats_big_kernel_b, stats_stage2_kernel_b,
dirichlet_kernel_b, mt_fill_wide_kernel_b), and a batch changes the launch geometry around them (the persistent stage-1 grid divided
by K, the deferred-list segments sized from it, max(2, 16 / K) workgroups per deferred list, stage 2 never split over workgroups).  The
single-chain forms at these shapes are checked against the oracle elsewhere (test_gpu_parity.py, test_gpu_philox.py), so "the batch
equals the chains run alone" carries that authority to the batched forms; two sections below put the oracle on chain K - 1 directly.

Every comparison is exact (np.array_equal / ==): ll, lp, nchange, gamma and eta traces, tau of EVERY stored iteration, final state, MAP
record (lp, it, tau), MT19937 state and counters(), after a first call of n_iter iterations and again after a second call of 2
iterations on the same contexts.

Which dispatch rule a case is meant to reach is restated here in Python (_tau_tile, _agg_lpv, _ntab_rep, _spec_run) and asserted by the
case itself: a change of the rules then says which row of the matrix lost its case.

batched form                          launched by
tau_kernel_b<16,1|16,2|16,3|32,2|32,3|64,2|64,3|64,4|64,6|64,8>   test_tau_tiles_* (one S per tile, MT19937 and Philox uniforms)
stats_agg_kernel_b<16|32|64, 2|3>     test_stats_forms_lpv_by_spec (S = 10, 100 / 20 / 64), test_stats_forms_stage2_by_G, test_subset_table_in_copies
stats_pat_kernel_b<16|32|64>          test_stats_forms_lpv_by_spec (spec 4), test_spec4_asked_at_the_edge_of_its_range (G = 6, 7, 8)
stats_big_kernel_b<2|3>               test_deferred_lists_in_a_batch (lists longer than one round of two workgroups), test_pooled_counts_in_a_batch
stats_stage2_kernel_b<2|3>            test_stats_forms_stage2_by_G (G = 10, 11, 12, 16: 1024 threads; G = 9 runs the fused 256-thread form)
dirichlet_kernel_b, mt_fill_wide_kernel_b, prior / finalize riders     every case (mt_fill_wide_kernel_b: the MT19937 ones)
several stage-1 passes per wavefront  test_several_stage1_passes_per_wavefront
"""
import functools
import subprocess
import sys

import numpy as np
import pytest

from desman_amd import _lib
from desman_amd.synth import synth_counts, random_state
from oracle import cbind

import test_gpu_philox as tph
from test_gpu_batch import _chain, _snapshot, _same
from _deferred import first_rule, ntab_rep as _ntab_rep

pytestmark = pytest.mark.gpu

MT, PHILOX = _lib.RNG_MT19937, _lib.RNG_PHILOX
MAX_BATCH = 8                   # DSM_MAX_BATCH


# ---------------------------------------------------------------- the dispatch rules, restated (test data, not kernel code)
def _tau_tile(S):
    """kernels_gibbs.hip: tau_shape -- (lanes per position, sample slots per lane) of the sweep kernels"""
    if S <= 16:
        return 16, 1
    if S <= 32:
        return 16, 2
    if S <= 48:
        return 16, 3
    if S <= 64:
        return 32, 2
    if S <= 96:
        return 32, 3
    need = (S + 63) // 64
    assert need <= 8
    return 64, (need if need <= 4 else 6 if need <= 6 else 8)


def _agg_lpv(S):
    """kernels_stats.hip: stats_agg_lpv -- lanes per position of stage 1: the chunk that pads S least, ties to the larger"""
    best = 64
    for lpv in (32, 16):
        if -(-S // lpv) * lpv < -(-S // best) * best:
            best = lpv
    return best


def _spec_run(asked, G):
    """kernels_stats.hip: stats_spec with a specification forced, on an unsharded chain with G <= 16"""
    return (4 if G <= 8 else 2) if asked == 4 else asked


def _keys(K):
    """K counter-stream keys with both words set and different"""
    return [(tph.CTR_SEEDS[0] + k * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF for k in range(K)]


# ---------------------------------------------------------------- running and comparing
def _make(counts, state, mt_seed, key, rng, spec):
    c = _chain(counts, state, mt_seed, key)
    c.set_tau_rng(rng)
    c.force_stats_spec(spec)
    return c


def _full(c, key):
    """everything a call leaves behind: test_gpu_batch's snapshot + tau of every stored iteration, the whole MAP record, the counters"""
    out = _snapshot(c)
    n = len(out["ll"])
    star = c.get_star()
    out["taus"] = np.array([c.get_tau_at(it) for it in range(n)])
    out["star_it"], out["star_tau"] = star["it"], star["tau"]
    k, it = c.counters()
    assert k == key
    out["counters"] = np.array([k, it], dtype=np.uint64)
    return out


def _batch_vs_alone(counts, states, n_iter, spec, rng=MT, keys=None, want_spec=None, after_first=None):
    """K = len(states) chains alone (n_iter iterations, then 2 more) and as one batch: equal after either call.  after_first(ctxs, lp0):
    called on the batch's contexts after the first call, with the log-posterior of the last chain's entry state."""
    K = len(states)
    keys = keys or [0xB47C4000 + k for k in range(K)]
    want_spec = spec if want_spec is None else want_spec
    single = []
    for k in range(K):
        a = _make(counts, states[k], 1000 + k, keys[k], rng, spec)
        try:
            assert a.stats_spec() == want_spec
            a.gibbs_update(n_iter)
            first = _full(a, keys[k])
            a.gibbs_update(2)
            single.append((first, _full(a, keys[k])))
        finally:
            a.close()
    ctxs = [_make(counts, states[k], 1000 + k, keys[k], rng, spec) for k in range(K)]
    try:
        assert ctxs[-1].stats_spec() == want_spec
        lp0 = ctxs[-1].loglik()[1] if after_first else None
        _lib.Context.batch_gibbs_update(ctxs, n_iter)
        for k in range(K):
            _same(single[k][0], _full(ctxs[k], keys[k]))
            assert single[k][0]["counters"][1] == n_iter
        if after_first:
            after_first(ctxs, lp0)
        _lib.Context.batch_gibbs_update(ctxs, 2)
        for k in range(K):
            _same(single[k][1], _full(ctxs[k], keys[k]))
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------- 1. tau tiles, batched
# (S, tile, G, K): one S per tile tau_shape can return, ragged inside the tile's range; need = 5 and 7 leave whole sample slots idle
_TILES = [(9, (16, 1), 3, 2), (23, (16, 2), 8, 2), (41, (16, 3), 3, 2), (57, (32, 2), 8, 2), (81, (32, 3), 3, 8), (101, (64, 2), 8, 2),
          (150, (64, 3), 3, 2), (230, (64, 4), 8, 2), (290, (64, 6), 3, 8), (400, (64, 8), 3, 2), (512, (64, 8), 8, 2)]
# V = 3 (256 / LPV) + 1: four workgroups, the last with one position; and one case below one workgroup
_TILE_CASES = [(3 * (256 // tile[0]) + 1, S, G, K, tile) for S, tile, G, K in _TILES] + [(1, 150, 8, 2, (64, 3))]
_TILE_IDS = ["S%d-%dx%d-V%d" % (S, tile[0], tile[1], V) for V, S, G, K, tile in _TILE_CASES]
_ORACLE_ON_LAST = {(81, 8), (290, 8), (512, 2)}            # (S, K): Philox cases whose chain K - 1 is also put against the oracle


def _assert_tile(c, V, S, tile):
    assert _tau_tile(S) == tile, "tau_shape no longer gives %dx%d at S = %d: the tile has lost its case" % (tile + (S,))
    need = (S + 63) // 64
    assert tile[0] * tile[1] >= S and (tile != (64, 6) or need == 5) and (S != 400 or need == 7)
    # what the library launches: a sweep of V positions is ceil(V / (256 / LPV)) workgroups
    assert c.tau_launch_info()[0] == -(-V // (256 // tile[0])), "the library's sweep does not run %d lanes per position at S = %d" % (tile[0], S)


@pytest.mark.parametrize("rng", [MT, PHILOX], ids=["mt19937", "philox"])
@pytest.mark.parametrize("V,S,G,K,tile", _TILE_CASES, ids=_TILE_IDS)
def test_tau_tiles_in_a_gibbs_batch(V, S, G, K, tile, rng):
    """tau_kernel_b<LPV, NSL, true, true> at every tile, K = 2 or 8 (blockIdx.y up to DSM_MAX_BATCH - 1), under spec 2, with the MT19937
    words (mt_fill_wide_kernel_b) and with Philox uniforms, every chain under its own key; in three Philox cases chain K - 1 is also the
    oracle's, piece by piece (test_gpu_philox.py: _assert_chain_is_the_oracles)."""
    assert K <= MAX_BATCH
    counts, _, _ = tph._table(V, S, G, seed=40 + S)
    states = [random_state(V, S, G, seed=700 + k) for k in range(K)]
    keys = _keys(K) if rng == PHILOX else None
    n_iter = 4
    probe = _make(counts, states[0], 1, 2, rng, 2)
    try:
        _assert_tile(probe, V, S, tile)
    finally:
        probe.close()

    def oracle_on_last(ctxs, lp0):
        c = ctxs[-1]
        assert c.counters() == (keys[-1], n_iter)
        assert np.array_equal(c.get_mt_state(), _lib.mt_seed_state(1000 + K - 1)), "MT19937 state"
        tph._assert_chain_is_the_oracles(c, counts, states[-1], keys[-1], 0, n_iter, 2, lp0=lp0)
        ran.append(len(ctxs))

    ran = []
    hook = oracle_on_last if rng == PHILOX and (S, K) in _ORACLE_ON_LAST and V > 1 else None
    _batch_vs_alone(counts, states, n_iter, 2, rng=rng, keys=keys, after_first=hook)
    assert ran == ([K] if hook else [])


def test_the_oracle_cases_of_the_tile_sweep_exist():
    assert {(S, K) for V, S, G, K, tile in _TILE_CASES if V > 1} >= _ORACLE_ON_LAST


@pytest.mark.parametrize("rng", [MT, PHILOX], ids=["mt19937", "philox"])
@pytest.mark.parametrize("V,S,G,K,tile", _TILE_CASES, ids=_TILE_IDS)
def test_tau_tiles_in_batch_update_tau(V, S, G, K, tile, rng):
    """dsm_batch_update_tau (tau-only sweeps over stored (gamma, eta) rows, the sweep with the finalize rider) of two chains at every tile
    against dsm_ctx_update_tau chain by chain: tau of every sweep and the traces, over two calls on the same contexts"""
    K, n = 2, 5
    counts, _, _ = tph._table(V, S, G, seed=40 + S)
    rs = np.random.RandomState(S)
    stores = [(np.ascontiguousarray(rs.dirichlet(np.ones(G), size=(n, S))),
               np.ascontiguousarray(rs.dirichlet(np.ones(4), size=(n, 4)) * 0.08 + 0.92 * np.eye(4))) for _ in range(K)]
    states = [random_state(V, S, G, seed=710 + k) for k in range(K)]
    keys = _keys(K)
    singles = []
    for k in range(K):
        c = _make(counts, states[k], 70 + k, keys[k], rng, 0)
        try:
            _assert_tile(c, V, S, tile)
            c.update_tau(*stores[k])
            first = _full(c, keys[k])
            c.update_tau(*stores[k])
            singles.append((first, _full(c, keys[k])))
        finally:
            c.close()
    ctxs = [_make(counts, states[k], 70 + k, keys[k], rng, 0) for k in range(K)]
    try:
        for rnd in range(2):
            _lib.Context.batch_update_tau(ctxs, [g for g, _ in stores], [e for _, e in stores])
            for k in range(K):
                got = _full(ctxs[k], keys[k])
                assert got["taus"].shape[0] == n and got["counters"][1] == (rnd + 1) * n
                _same(singles[k][rnd], got)
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------- 2. the mu/E pass, batched
def _stats_case(V, S, G, spec, K=3, n_iter=4, want_lpv=None, want_rep=None, after_first=None):
    """MT19937, K = 3, n_iter = 4; after_first(ctxs, lp0, counts, states): see _batch_vs_alone"""
    counts, _, _ = synth_counts(V, S, G, seed=500 + V + G)
    states = [random_state(V, S, G, seed=600 + k) for k in range(K)]
    if want_lpv is not None:
        assert _agg_lpv(S) == want_lpv, "stats_agg_lpv no longer gives %d lanes at S = %d" % (want_lpv, S)
    if want_rep is not None:
        assert want_rep(_ntab_rep(V, S, G))
    hook = (lambda ctxs, lp0: after_first(ctxs, lp0, counts, states)) if after_first else None
    _batch_vs_alone(counts, states, n_iter, spec, want_spec=_spec_run(spec, G), after_first=hook)


@pytest.mark.parametrize("spec", [2, 3, 4])
@pytest.mark.parametrize("S,lpv", [(10, 16), (20, 32), (64, 64), (100, 16)])
def test_stats_forms_lpv_by_spec(S, lpv, spec):
    """stats_agg_kernel_b<LPV, 2 | 3> and stats_pat_kernel_b<LPV> at every lane-group width (S = 100: seven chunks of 16), stage 2 fused in
    dirichlet_kernel_b, stats_big_kernel_b<2 | 3> behind each"""
    assert -(-S // lpv) == {10: 1, 20: 1, 64: 1, 100: 7}[S]
    _stats_case(150, S, 5, spec, want_lpv=lpv)


@pytest.mark.parametrize("spec", [2, 3])
@pytest.mark.parametrize("G", [9, 10, 11, 12, 16])
def test_stats_forms_stage2_by_G(G, spec):
    """stage 2 of a batch: fused with 256 threads at G = 9, stats_stage2_kernel_b<2 | 3> with 1024 threads and one workgroup per sample from
    G = 10 -- against the single chain's unsplit (G = 10), 2-way (G = 11) and 4-way split launches (G >= 12); G = 16: the largest table"""
    V, S = (40, 7) if G == 16 else (150, 20)
    _stats_case(V, S, G, spec, want_lpv=_agg_lpv(S))


def test_stage2_batch_chain_K_minus_1_is_the_oracles():
    """S = 20, G = 12 under spec 3 again, and chain K - 1 of the batch (blockIdx.y = 2) against the oracle piece by piece on the GSL stream"""
    V, S, G, spec, K, n_iter = 150, 20, 12, 3, 3, 4
    ran = []

    def oracle_on_last(ctxs, lp0, counts, states):
        _assert_mt_chain_is_the_oracles(ctxs[-1], counts, states[-1], 1000 + K - 1, 0xB47C4000 + K - 1, n_iter, spec, lp0)
        ran.append(len(ctxs))

    _stats_case(V, S, G, spec, K=K, n_iter=n_iter, after_first=oracle_on_last)
    assert ran == [K]


def _assert_mt_chain_is_the_oracles(c, counts, start, mt_seed, cseed, n_iter, spec, lp0):
    """the n_iter iterations context c has just run from `start` (first call after dsm_ctx_seed(mt_seed, cseed)) against the oracle in the
    reference's order, as test_gpu_parity.py: test_gibbs_update_is_self_consistent_with_oracle does for a chain run alone: mu/E sums +
    gamma / eta draws (1e-13 relative: device log / pow vs libm), the sweep bit for bit on the GSL stream, ll / lp (1e-12), final state,
    tau sum, MAP record."""
    tau0, gamma0, eta0 = start
    V, G = tau0.shape[:2]
    tr = c.get_trace()
    g_prev, e_prev, t_prev = gamma0, eta0, tau0
    for it in range(n_iter):
        args = (cbind.onehot_to_idx(t_prev), np.ascontiguousarray(g_prev), np.ascontiguousarray(e_prev), counts, cseed, it)
        mu, E = cbind.stats_agg(*args, spec=spec) if spec >= 2 else cbind.stats_counter(*args)
        g_ref, e_ref, _ = cbind.dirichlet_counter(mu, E, cseed, it)
        np.testing.assert_allclose(tr["gamma"][it], g_ref, rtol=1e-13, atol=0)
        np.testing.assert_allclose(tr["eta"][it], e_ref, rtol=1e-13, atol=0)
        g_prev, e_prev, t_prev = tr["gamma"][it], tr["eta"][it], c.get_tau_at(it)
    mt = cbind.MT19937(mt_seed)
    tau_prev, eta_prev = tau0.copy(), np.array(eta0)
    lps = [lp0]
    tau_sum = np.zeros_like(tau0)
    for it in range(n_iter):
        tau_it = c.get_tau_at(it)
        ref = tau_prev.copy()
        n_ref = cbind.sample_tau_u(ref, np.ascontiguousarray(tr["gamma"][it]), eta_prev, counts, mt.uniform(V * G))
        assert np.array_equal(tau_it, ref) and tr["nchange"][it] == n_ref, it
        idx = cbind.onehot_to_idx(tau_it)
        g_it, e_it = np.ascontiguousarray(tr["gamma"][it]), np.ascontiguousarray(tr["eta"][it])
        assert tr["ll"][it] == pytest.approx(cbind.loglik(idx, g_it, e_it, counts), rel=1e-12)
        assert tr["lp"][it] == pytest.approx(cbind.logpost(idx, g_it, e_it, counts), rel=1e-12)
        np.testing.assert_allclose(g_it.sum(axis=1), 1.0, rtol=1e-12)
        lps.append(tr["lp"][it]); tau_sum += tau_it
        tau_prev, eta_prev = tau_it, e_it
    tau_f, gamma_f, eta_f = c.get_state()
    assert np.array_equal(tau_f, tau_prev) and np.array_equal(gamma_f, tr["gamma"][-1]) and np.array_equal(eta_f, tr["eta"][-1])
    assert np.array_equal(c.get_tau_sum(), tau_sum)
    star = c.get_star()
    k = int(np.argmax(lps))                                       # first strict maximum, entry state = slot 0
    assert star["lp"] == lps[k]
    if k == 0:
        assert np.array_equal(star["tau"], tau0) and np.array_equal(star["gamma"], gamma0)
    else:
        assert np.array_equal(star["tau"], c.get_tau_at(k - 1)) and np.array_equal(star["gamma"], tr["gamma"][k - 1]) \
            and np.array_equal(star["eta"], tr["eta"][k - 1]) and star["it"] == k - 1


@pytest.mark.parametrize("V,S,G,want", [(150, 20, 8, 4), (150, 20, 9, 2), (300, 33, 6, 4), (300, 33, 7, 4)])
def test_spec4_asked_at_the_edge_of_its_range(V, S, G, want):
    """spec 4 asked: it runs up to G = 8 and spec 2 runs at G = 9; G = 6: the word table's LDS form (pat_rep_lds_kernel), G = 7: its global
    form (pat_rep_kernel) -- each chain's pooling passes, then stats_pat_kernel_b over the chains' own word lists"""
    assert _spec_run(4, G) == want
    _stats_case(V, S, G, 4, want_lpv=_agg_lpv(S))


@pytest.mark.parametrize("spec", [2, 3])
def test_subset_table_in_copies(spec):
    """3 V / 2^G > 128: stage 1 adds to copy blockIdx.x mod rep of the subset table, stats_big_kernel_b to its own, stage 2 sums them"""
    _stats_case(2500, 12, 3, spec, want_lpv=16, want_rep=lambda rep: rep > 1)


# ---------------------------------------------------------------- 3. what only a batch does to stage 1
def _words(state):
    return len(np.unique(np.argmax(state[0], axis=2), axis=0))


@functools.lru_cache(maxsize=None)
def _compute_units():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process (once per session): in this process the
    library has opened the device through its own HIP runtime, and torch, coming second with the runtime it ships, finds no GPU"""
    code = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, timeout=120).stdout
    return int(out.split()[-1])


@pytest.mark.parametrize("spec", [2, 3, 4])
def test_several_stage1_passes_per_wavefront(spec):
    """The chains of a batch share the persistent stage-1 grid: max_waves = stats_grid 4 / K with stats_grid <= 6 workgroups per CU, so at
    K = 8 a chain has at most 3 CUs wavefronts.  S = 64 is one task per position (64 lanes per position, one chunk): with V > 3 CUs
    every batched wavefront that runs a second pass does so only in the batch -- the pass loop and the deferred-list segments sized
    from the smaller grid -- whatever the occupancy turns out to be.  Under spec 4 the tasks are the distinct tau words of the state."""
    cus = _compute_units()
    K, S, G, n_iter = MAX_BATCH, 64, 5, 3
    V = max(1600, 6 * cus + 37)
    assert V > 3 * cus and _agg_lpv(S) == 64
    counts, _, _ = synth_counts(V, S, G, seed=500 + V)
    states = [random_state(V, S, G, seed=600 + k) for k in range(K)]
    if spec == 4 and V == 1600:                                   # (788 ... 834 words in these eight start states)
        assert min(_words(st) for st in states) > 3 * cus
    _batch_vs_alone(counts, states, n_iter, spec)


def _deferred(counts, state, pooled=False):
    """bool [entries, S, 4] x 2: the items stage 1 defers from `state` by the mean of the rarer outcome (a lower bound), of kind 0"""
    return first_rule(counts, *state, pooled=pooled)


def _longest_sublist(deferred, kind0):
    """items on the longest of the 3 x 64 sub-lists when stage 1 runs one wavefront per position: workgroup = 4 positions, sub-list =
    kind x (workgroup mod 64)"""
    sub = (np.arange(deferred.shape[0]) // 4) % 64
    per = np.zeros((2, 64), dtype=np.int64)
    np.add.at(per[0], sub, kind0.sum(axis=(1, 2)))
    np.add.at(per[1], sub, (deferred & ~kind0).sum(axis=(1, 2)))
    return int(per.max())


@pytest.mark.parametrize("spec", [2, 3])
def test_deferred_lists_in_a_batch(spec):
    """stats_big_kernel_b<2 | 3> draining long deferred lists with max(2, 16 / 8) = 2 workgroups per list (a single chain has 16), the lists
    in segments sized from the batch's share of the grid: (V, S, G) = (400, 64, 8), the shape test_stats_stage1_matches_spec names for
    long lists, random start states, K = 8.  At the depth that test uses (depth_scale = 10) the rule restated in _deferred gives 24 611
    ... 31 605 deferred items per start state but at most 454 on one sub-list -- less than one round of two workgroups (512) -- so the
    depth is 20 x here: 38 318 ... 46 995 items per start state (of 102 400), 590 ... 746 of them on the longest sub-list of a chain
    (one wavefront per position: 100 workgroups on 64 sub-lists of each kind), i.e. a second round in every chain."""
    V, S, G, K = 400, 64, 8, MAX_BATCH
    counts, _, _ = synth_counts(V, S, G, seed=500 + V, depth_scale=20.0)
    states = [random_state(V, S, G, seed=600 + k) for k in range(K)]
    for st in states:
        d, k0 = _deferred(counts, st)
        assert d.sum() >= 1, "a start state without deferred items"
        assert _longest_sublist(d, k0) > 512, "no sub-list longer than one round of two workgroups"
    _batch_vs_alone(counts, states, 3, spec)


def test_pooled_counts_in_a_batch():
    """spec 4 on deep data: the deferred items carry pooled counts, which stats_big_kernel_b reads and clears (pat_x) -- (V, S, G) =
    (400, 64, 4), 10 x depth, K = 4 (four workgroups per list): 193 ... 200 words per start state, 18 829 ... 22 522 deferred items"""
    V, S, G, K = 400, 64, 4, 4
    counts, _, _ = synth_counts(V, S, G, seed=500 + V, depth_scale=10.0)
    states = [random_state(V, S, G, seed=600 + k) for k in range(K)]
    for st in states:
        d, _ = _deferred(counts, st, pooled=True)
        assert d.shape[0] == _words(st) < V and d.sum() >= 1, "a start state without deferred pooled items"
    _batch_vs_alone(counts, states, 3, 4)


# ---------------------------------------------------------------- 5. mixed sequences on the same contexts
@pytest.mark.parametrize("spec", [2, 4])
def test_batches_and_single_calls_mixed_on_the_same_contexts(spec):
    """A batch of three for 3 iterations; chain 1 alone for 2 and chains 0 and 2 as a batch of two for 2; all three batched again for 3 --
    against three contexts that ran 3 + 2 + 3 iterations alone.  Nothing a batch leaves behind may change what follows: the launchers'
    thread_local argument blocks (filled for K = 3, then K = 2), the parity of the word table's generation (spec 4), the persistent
    grid kept per specification, the deferred-list segments sized for another K."""
    V, S, G, K = 257, 81, 5, 3
    counts, _, _ = synth_counts(V, S, G, seed=500 + V)
    states = [random_state(V, S, G, seed=600 + k) for k in range(K)]
    keys = [0xB47C4000 + k for k in range(K)]
    calls = (3, 2, 3)
    alone = []
    for k in range(K):
        a = _make(counts, states[k], 1000 + k, keys[k], MT, spec)
        try:
            assert a.stats_spec() == spec
            snaps = []
            for n in calls:
                a.gibbs_update(n)
                snaps.append(_full(a, keys[k]))
            alone.append(snaps)
        finally:
            a.close()
    ctxs = [_make(counts, states[k], 1000 + k, keys[k], MT, spec) for k in range(K)]
    try:
        _lib.Context.batch_gibbs_update(ctxs, calls[0])
        for k in range(K):
            _same(alone[k][0], _full(ctxs[k], keys[k]))
        ctxs[1].gibbs_update(calls[1])
        _lib.Context.batch_gibbs_update([ctxs[0], ctxs[2]], calls[1])
        for k in range(K):
            _same(alone[k][1], _full(ctxs[k], keys[k]))
        _lib.Context.batch_gibbs_update(ctxs, calls[2])
        for k in range(K):
            got = _full(ctxs[k], keys[k])
            assert got["counters"][1] == sum(calls)
            _same(alone[k][2], got)
    finally:
        for c in ctxs:
            c.close()
