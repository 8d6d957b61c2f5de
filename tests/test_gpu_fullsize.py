"""Parity at BASELINE.json's full sizes (configs[2]: V=10k, S=64, G=8; configs[4]: V=50k, S=96, G=12):
the C oracle still finishes one tau sweep / one log-likelihood in seconds, so the integer outcome is
compared exactly; the per-read pass is checked through its size-independent invariants."""
import numpy as np
import pytest

from desman_amd import _lib
from desman_amd.synth import synth_counts, random_state
from oracle import cbind

pytestmark = pytest.mark.gpu


# (50000, 96, G) for G = 2, 4, 6, 10: the other legs of BASELINE config 5 (g in 2..12) at full V.  They take code the G = 12 leg does not:
# the subset table in 16-64 copies at few haplotypes (stats_ntab_rep), the stand-alone stage-2 launch at G = 10 / 11, and the
# register-lean sweep tau_kernel<32,3> with prefix lengths other than 12.
@pytest.mark.parametrize("V,S,G", [(10000, 64, 8), (50000, 96, 12), (50000, 96, 2), (50000, 96, 4), (50000, 96, 6), (50000, 96, 10)])
def test_full_size_sweep_loglik_and_stats_invariants(V, S, G):
    counts, _, _ = synth_counts(V, S, G, seed=1234)
    tau, gamma, eta = random_state(V, S, G, seed=5)
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    ctx.set_state(tau, gamma, eta)
    ctx.seed(31337, ctr_seed=42)
    # log-likelihood / log-posterior of the whole tensor
    ll, lp = ctx.loglik()
    idx = cbind.onehot_to_idx(tau)
    assert ll == pytest.approx(cbind.loglik(idx, gamma, eta, counts), rel=1e-12)
    assert lp == pytest.approx(cbind.logpost(idx, gamma, eta, counts), rel=1e-12)
    # one full tau sweep: bit-identical haplotypes and change count
    ref = tau.copy()
    n_ref = cbind.sample_tau_u(ref, gamma, eta, counts, cbind.MT19937(31337).uniform(V * G))
    n = ctx.sample_tau()
    got, _, _ = ctx.get_state()
    assert n == n_ref and np.array_equal(got, ref)
    # per-read pass: every read is assigned exactly once, observed-base totals are preserved,
    # identical (seed, iter) -> identical sums, different iter -> different sums
    mu, E = ctx.sample_stats(3)
    # full sizes run the aggregated sampler: over tau words where at most a quarter as many words as positions exist (spec 4) ...
    spec = ctx.stats_spec()
    cells = V * S
    by_rule = 4 if ((G <= 2 and cells >= 0.5e6) or (G == 3 and cells >= 1e6) or (4 <= G <= 8 and cells >= 2.5e6 and 64 * 2 ** G <= V)) else _lib.STATS_AGG
    assert spec == by_rule and _lib.STATS_AGG == cbind.STATS_AGG
    mu_ref, E_ref = cbind.stats_agg(cbind.onehot_to_idx(got), gamma, eta, counts, 42, 3, spec=spec)
    assert np.array_equal(mu, mu_ref) and np.array_equal(E, E_ref)   # ... bit for bit as restated in oracle/stats_agg.c
    assert int(mu.sum()) == int(counts.sum())
    assert np.array_equal(mu.sum(axis=1), counts.sum(axis=(0, 2)).astype(np.uint64))        # reads per sample
    assert np.array_equal(E.sum(axis=1), counts.sum(axis=(0, 1)).astype(np.uint64))         # reads per observed base
    mu2, E2 = ctx.sample_stats(3)
    assert np.array_equal(mu, mu2) and np.array_equal(E, E2)
    mu3, _ = ctx.sample_stats(4)
    assert not np.array_equal(mu, mu3)
    # expectation check (z-test on the S x G sums against the exact conditional mean)
    e_mu, v_mu, e_E = cbind.stats_expect(cbind.onehot_to_idx(got), gamma, eta, counts)
    z = (mu.astype(np.float64) - e_mu) / np.sqrt(v_mu + 1e-9)
    assert np.abs(z).max() < 5.5 and abs(z.mean()) < 0.5
    # a few full iterations keep every trace consistent with the oracle's likelihood; the first iteration's gamma / eta
    # are the oracle's draws from the oracle's sums (mu/E stage 2 runs fused in the Dirichlet launch for G < 10, as its
    # own 1024-thread launch above)
    ctx.seed(31337, ctr_seed=42)
    ctx.gibbs_update(3)
    tr = ctx.get_trace()
    mu0, E0 = cbind.stats_agg(cbind.onehot_to_idx(got), gamma, eta, counts, 42, 0, spec=spec)
    g0, e0, _ = cbind.dirichlet_counter(mu0, E0, 42, 0)
    np.testing.assert_allclose(tr["gamma"][0], g0, rtol=1e-13, atol=0)
    np.testing.assert_allclose(tr["eta"][0], e0, rtol=1e-13, atol=0)
    t, g, e = ctx.get_state()
    assert tr["ll"][-1] == pytest.approx(cbind.loglik(cbind.onehot_to_idx(t), g, e, counts), rel=1e-12)
    np.testing.assert_allclose(g.sum(axis=1), 1.0, rtol=1e-12)
    ctx.close()


# ---------------------------------------------------------------- A10/A11 at BASELINE sizes
# Init_NMFT.factorize (/root/reference/desman/Init_NMFT.py:98-115), div_update (:158-181), factorize_tau / div_update_tau
# (:134-149, :192-205), get_tau (:230-245) on tables that take the product path of configs 3-5: more than 128 workgroup
# partials (nmft_reduce_kernel + nmft_gamma_kernel as their own launches) and, above V = 12 288, the grid-stride loop of
# nmft_mfma_body.  V = 3000 crosses the 128-partial switch from above, V = 2000 sits right below it.
def _nmft_case(V, S, G, seed=1234):
    from oracle import ref_numpy as rn
    counts, _, _ = synth_counts(V, S, G, seed=seed)
    tau0, gam0 = rn.nmft_random_initialize(np.random.RandomState(seed + 1), V, S, G)
    return counts, tau0, gam0, cbind.nmft_freq(counts)


def _nmft_run(counts, tau0, gam0, fused, fix_gamma, max_iter=20, persist=0):
    c = _lib.Context(0)
    c.set_counts(counts)
    c.set_nmft_persist(persist)          # 0: the three-launch loop (whose reduce + gamma step `fused` selects), 1: one persistent launch
    c.set_nmft_fused(fused)
    c.nmft_set(tau0, gam0)
    n, tr = c.nmft_factorize(max_iter=max_iter, min_change=1e-5, fix_gamma=fix_gamma)
    tau, gam = c.nmft_get()
    onehot = c.nmft_get_tau()
    div = c.nmft_objective()
    c.close()
    return n, tr, tau, gam, onehot, div


def _nmft_two_calls(counts, tau0, gam0, fused):
    """factorize with an odd number of updates, then factorize_tau, on one context of the three-launch loop"""
    c = _lib.Context(0)
    c.set_counts(counts)
    c.set_nmft_persist(0)
    c.set_nmft_fused(fused)
    c.nmft_set(tau0, gam0)
    out = []
    for fix_gamma in (False, True):
        n, tr = c.nmft_factorize(max_iter=19, min_change=1e-5, fix_gamma=fix_gamma)
        tau, gam = c.nmft_get()
        out.append((n, tr, tau, gam, c.nmft_get_tau()))
    c.close()
    return out


@pytest.mark.parametrize("V,S,G", [(10000, 64, 8), (50000, 96, 12), (3000, 64, 8), (2000, 32, 5), (13000, 40, 3), (12288, 48, 12), (933, 64, 5),
                                   (97, 20, 2), (5000, 128, 8), (2500, 110, 12), (14001, 100, 3), (3000, 64, 16), (6000, 96, 13), (2000, 128, 15),
                                   (3000, 300, 8), (1001, 130, 3), (801, 512, 16), (2000, 200, 12), (1500, 260, 5), (37, 400, 2),
                                   (3000, 96, 8), (1500, 80, 12), (4096, 90, 3)])      # 65..96 samples, V <= 4096: the persistent loop's four-wavefront form
def test_full_size_nmft_factorize_matches_oracle(V, S, G):
    counts, tau0, gam0, F = _nmft_case(V, S, G)
    for fix_gamma in (False, True):
        tc, gc = tau0.copy(), gam0.copy()
        if fix_gamma:
            n_ref, tr_ref = cbind.nmft_factorize_tau(F, tc, gc, max_iter=20, min_change=1e-5)
        else:
            n_ref, tr_ref = cbind.nmft_factorize(F, tc, gc, max_iter=20, min_change=1e-5)
        runs = {f: _nmft_run(counts, tau0, gam0, f, fix_gamma) for f in (-1, 0, 1, 3)}
        n, tr, tau, gam, onehot, div = runs[-1]
        assert n == n_ref and (fix_gamma or n_ref == 20)           # factorize_tau may stop by itself (13 updates at 13000 x 40 x 3)
        np.testing.assert_allclose(tr, tr_ref, rtol=1e-9)                 # the whole objective trace
        np.testing.assert_allclose(tau, tc, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(gam, gc, rtol=1e-6, atol=1e-12)
        if fix_gamma:
            assert np.array_equal(gam, gam0)                              # factorize_tau never touches gamma
        # arg-max of the factor: the oracle's one-hot wherever the device's own factor is not within rounding of a tie
        ref_idx = cbind.nmft_get_tau(tc, G)
        own_idx = cbind.nmft_get_tau(tau, G)
        assert np.array_equal(onehot, cbind.idx_to_onehot(own_idx))       # get_tau of the device = get_tau of its own factor
        assert (own_idx != ref_idx).mean() < 1e-5
        assert div == pytest.approx(cbind.nmft_objective(F, tc, gc), rel=1e-9)
        # the forms of the gamma / control step -- a launch of its own, one launch with the reduction, the start of the update kernel
        # (round 6; large tables' default) --: the same bits, on either side of the size rule
        for f in (0, 1, 3):
            m, tr_f, tau_f, gam_f, onehot_f, div_f = runs[f]
            assert m == n and np.array_equal(tr_f, tr) and np.array_equal(tau_f, tau) and np.array_equal(gam_f, gam)
            assert np.array_equal(onehot_f, onehot) and div_f == div
        # the whole loop as ONE persistent launch (tables up to 12 288 positions, S <= 64; elsewhere the call is the three-launch
        # loop again): its workgroups publish the partial rows of the three-launch kernel, so every bit agrees
        m, tr_p, tau_p, gam_p, onehot_p, div_p = _nmft_run(counts, tau0, gam0, -1, fix_gamma, persist=1)
        assert m == n and np.array_equal(tr_p, tr) and np.array_equal(tau_p, tau) and np.array_equal(gam_p, gam)
        assert np.array_equal(onehot_p, onehot) and div_p == div
        if fix_gamma:
            assert np.array_equal(gam_p, gam0)
        else:
            # a second call on the context after the update kernel's own gamma step (3: where the shape allows it) ran an odd number
            # of updates, which leaves the current gamma in its second buffers: the same bits as with a launch of its own (0)
            gst, own = _nmft_two_calls(counts, tau0, gam0, 3), _nmft_two_calls(counts, tau0, gam0, 0)
            assert gst[0][0] == 19
            for x, y in zip(gst, own):
                assert x[0] == y[0] and all(np.array_equal(u, v) for u, v in zip(x[1:], y[1:]))


def test_full_size_nmft_stop_rule_fires_at_the_oracles_update():
    """the |delta div| <= min_change stop (Init_NMFT.py:106) on the two-launch control path: a loose threshold so
    that the loop stops by itself well before max_iter at V = 10 000."""
    counts, tau0, gam0, F = _nmft_case(10000, 64, 8, seed=77)
    tc, gc = tau0.copy(), gam0.copy()
    n_ref, tr_ref = cbind.nmft_factorize(F, tc, gc, max_iter=200, min_change=30.0)
    assert 3 < n_ref < 200
    for fused, persist in ((-1, 0), (0, 0), (1, 0), (3, 0), (-1, 1)):
        c = _lib.Context(0)
        c.set_counts(counts)
        c.set_nmft_persist(persist)
        c.set_nmft_fused(fused)
        c.nmft_set(tau0, gam0)
        n, tr = c.nmft_factorize(max_iter=200, min_change=30.0)
        assert n == n_ref and len(tr) == len(tr_ref)
        np.testing.assert_allclose(tr, tr_ref, rtol=1e-9)
        tau, gam = c.nmft_get()
        np.testing.assert_allclose(tau, tc, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(gam, gc, rtol=1e-6, atol=1e-12)
        c.close()


@pytest.mark.parametrize("V,S,G,K", [(10000, 64, 8, 3), (3000, 48, 5, 2), (13000, 96, 12, 2), (4000, 128, 9, 2), (3000, 40, 14, 2)])
def test_full_size_batched_nmft_equals_one_by_one_and_oracle(V, S, G, K):
    """dsm_batch_nmft_factorize above 128 workgroup partials (nmft_reduce_kernel_b / nmft_gamma_kernel_b and the
    grid-stride loop of nmft_mfma_kernel_b): chain k ends bit for bit where dsm_nmft_factorize leaves it, and chain 0
    agrees with the oracle."""
    from oracle import ref_numpy as rn
    counts, _, _ = synth_counts(V, S, G, seed=4321)
    starts = [rn.nmft_random_initialize(np.random.RandomState(100 + k), V, S, G) for k in range(K)]
    for fix_gamma in (False, True):
        singles = []
        for tau0, gam0 in starts:
            c = _lib.Context(0); c.set_counts(counts); c.nmft_set(tau0, gam0)
            n, tr = c.nmft_factorize(12, 1e-5, fix_gamma)
            singles.append((n, tr, c.nmft_get(), c.nmft_get_tau()))
            c.close()
        for fused in (-1, 1):
            ctxs = []
            for tau0, gam0 in starts:
                c = _lib.Context(0); c.set_counts(counts); c.nmft_set(tau0, gam0); c.set_nmft_fused(fused)
                ctxs.append(c)
            res = _lib.Context.batch_nmft_factorize(ctxs, 12, 1e-5, fix_gamma)
            for c, (n, tr), (n1, tr1, fac1, oh1) in zip(ctxs, res, singles):
                fac = c.nmft_get()
                assert n == n1 and np.array_equal(tr, tr1)
                assert np.array_equal(fac[0], fac1[0]) and np.array_equal(fac[1], fac1[1])
                assert np.array_equal(c.nmft_get_tau(), oh1)
                c.close()
        F = cbind.nmft_freq(counts)
        tc, gc = starts[0][0].copy(), starts[0][1].copy()
        fn = cbind.nmft_factorize_tau if fix_gamma else cbind.nmft_factorize
        n_ref, tr_ref = fn(F, tc, gc, max_iter=12, min_change=1e-5)
        assert singles[0][0] == n_ref
        np.testing.assert_allclose(singles[0][1], tr_ref, rtol=1e-9)
        np.testing.assert_allclose(singles[0][2][0], tc, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(singles[0][2][1], gc, rtol=1e-6, atol=1e-12)


def test_persistent_nmft_that_times_out_falls_back_to_the_three_launch_loop():
    """a persistent launch whose workgroups are not all resident never passes its first grid barrier: the polls are bounded, the
    factors saved before the launch are put back and the three-launch loop runs instead -- same result.  (Forced here by a barrier
    that waits for one arrival group too many; in a child process: the switch is read from the environment.)"""
    import os
    import subprocess
    import sys
    import tempfile
    code = r'''
import sys; sys.path.insert(0, %r)
import numpy as np
from desman_amd import _lib
from desman_amd.synth import synth_counts
from oracle import ref_numpy as rn
counts, _, _ = synth_counts(900, 32, 4, seed=3)
tau0, gam0 = rn.nmft_random_initialize(np.random.RandomState(4), 900, 32, 4)
c = _lib.Context(0); c.set_counts(counts); c.nmft_set(tau0, gam0)
n, tr = c.nmft_factorize(15, 1e-5)
t, g = c.nmft_get()
np.savez(sys.argv[1], n=n, tr=tr, t=t, g=g)
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        outs = []
        # the forcing switch exists only in the experiment build (make -C desman_amd/csrc ab: -DDSM_AB_SWITCHES)
        for env_extra in ({}, {"DESMAN_HIP_NMFT_FORCE_TIMEOUT": "1", "DESMAN_HIP_LIB": _lib.AB_LIB_PATH}):
            path = os.path.join(d, "o%d.npz" % len(outs))
            r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            if env_extra:
                assert "falling back to the three-launch loop" in r.stderr
            outs.append(np.load(path))
        a, b = outs
        assert int(a["n"]) == int(b["n"]) == 15 and np.array_equal(a["tr"], b["tr"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["g"], b["g"])


@pytest.mark.parametrize("shape", [(1000, 100, 4), (4000, 32, 4)])
@pytest.mark.parametrize("fix_gamma", [False, True])
def test_nmft_graph_replay_equals_the_eager_loop(fix_gamma, shape, monkeypatch):
    """DESMAN_HIP_NMFT_GRAPH=1 (desman_amd.chains sets it): batches of 64 updates of the three-launch loop captured once and replayed --
    the same launches, so the same factors, update count and objective trace as the eager loop; with gamma fixed an update is the
    update kernel + the one-wavefront objective / control launch (nmft_objctl_kernel).  S > 64: the persistent loop does not apply; the
    second shape (250 workgroup partials, the persistent loop switched off) replays the two-launch update whose kernel begins with the
    gamma / control step (round 6: the parity of a captured node's buffers and control slots is the same in every replay)."""
    from oracle import ref_numpy as rn
    V, S, G = shape
    counts, _, _ = synth_counts(V, S, G, seed=11)
    tau0, gam0 = rn.nmft_random_initialize(np.random.RandomState(12), V, S, G)
    outs = []
    for graph in ("0", "1"):
        monkeypatch.setenv("DESMAN_HIP_NMFT_GRAPH", graph)
        c = _lib.Context(0)
        c.set_counts(counts)
        c.set_nmft_persist(0)
        c.nmft_set(tau0, gam0)
        n, tr = c.nmft_factorize(max_iter=150, min_change=1e-5, fix_gamma=fix_gamma)
        t, g = c.nmft_get()
        outs.append((n, np.asarray(tr), t, g))
        c.close()
    (n0, tr0, t0, g0), (n1, tr1, t1, g1) = outs
    assert n0 == n1 and np.array_equal(tr0, tr1) and np.array_equal(t0, t1) and np.array_equal(g0, g1)
    F = cbind.nmft_freq(counts)
    tc, gc = tau0.copy(), gam0.copy()
    n_ref, tr_ref = (cbind.nmft_factorize_tau if fix_gamma else cbind.nmft_factorize)(F, tc, gc, max_iter=150, min_change=1e-5)
    assert n0 == n_ref
    np.testing.assert_allclose(tr0, tr_ref, rtol=1e-9)
    np.testing.assert_allclose(t0, tc, rtol=1e-6, atol=1e-12)


# ---- a chain's draws do not depend on how it is run (VERDICT r4 "weak" 1): nothing forced, BASELINE config-5 shapes where the rule gives
# the word-pooled mu/E pass (spec 4) to the lone chain -- rounds 2-4 ran spec 2 in every batch
@pytest.mark.parametrize("G", [2, 4, 8])
def test_full_size_batch_by_rule_equals_chains_one_by_one(G):
    V, S, K, n_iter = 50000, 96, 2, 4
    counts, _, _ = synth_counts(V, S, 6, seed=1234)                # six strains: few tau words
    states = [random_state(V, S, G, seed=40 + k) for k in range(K)]

    def chain(k):
        c = _lib.Context(0)
        c.set_counts(counts); c.set_state(*states[k]); c.seed(100 + k, ctr_seed=0xC0FFEE00 + k)
        return c
    single = []
    for k in range(K):
        a = chain(k)
        assert a.stats_spec() == 4
        a.gibbs_update(n_iter)
        single.append((a.get_trace(), a.get_state()))
        a.close()
    ctxs = [chain(k) for k in range(K)]
    _lib.Context.batch_gibbs_update(ctxs, n_iter)
    for k, c in enumerate(ctxs):
        tr, st = c.get_trace(), c.get_state()
        for key in ("ll", "lp", "nchange", "gamma", "eta"):
            assert np.array_equal(tr[key], single[k][0][key]), (G, k, key)
        assert all(np.array_equal(x, y) for x, y in zip(st, single[k][1]))
        c.close()


def test_full_size_sharded_chain_is_the_unsharded_chain_under_spec_2():
    """A chain sharded by positions runs the aggregated pass, spec 2 (representatives of the word-pooled pass would be per shard:
    kernels_stats.hip: stats_spec), whatever the rule gives the unsharded chain -- here spec 4.  Two shards of a BASELINE config-5
    table equal the unsharded chain that ASKS for spec 2 (dsm_ctx_force_stats_spec / DESMAN_HIP_STATS_SPEC=2) bit for bit; the
    unsharded chain by rule draws other variates of the same law (tests/test_gpu_parity.py: the law tests of every spec)."""
    import threading
    from desman_amd import vshard
    V, S, G, n_iter, shards = 50000, 96, 4, 3, 2
    counts, _, _ = synth_counts(V, S, 6, seed=1234)
    tau, gamma, eta = random_state(V, S, G, seed=77)
    seed, cseed = 5, 0xFEED5EED4321
    refs = {}
    for force in (0, _lib.STATS_AGG):
        c = _lib.Context(0)
        c.set_counts(counts); c.set_state(tau, gamma, eta); c.seed(seed, ctr_seed=cseed); c.set_tau_rng(_lib.RNG_PHILOX)
        c.force_stats_spec(force)
        assert c.stats_spec() == (4 if force == 0 else 2)
        c.gibbs_update(n_iter)
        refs[force] = (c.get_trace(), c.get_state()[0])
        c.close()
    b = vshard.shard_bounds(V, shards)
    ex = vshard.HostExchange(shards)
    chains = []
    for k in range(shards):
        ch = vshard.ShardedChain(counts[b[k]:b[k + 1]], b[k], V, G, seed, ctr_seed=cseed)
        ch.set_state(tau[b[k]:b[k + 1]], gamma, eta)
        chains.append(ch)
    errs = []

    def work(k):
        try:
            chains[k].update(n_iter, ex.for_shard(k))
        except BaseException as e:                           # noqa: BLE001
            errs.append(e)
            ex.bar.abort()
    th = [threading.Thread(target=work, args=(k,)) for k in range(shards)]
    [t.start() for t in th]
    [t.join(900) for t in th]
    assert not errs, errs
    tr2 = refs[_lib.STATS_AGG][0]
    for k, ch in enumerate(chains):
        tr = ch.trace()
        assert np.array_equal(tr["gamma"], tr2["gamma"]) and np.array_equal(tr["eta"], tr2["eta"]) and np.array_equal(tr["nchange"], tr2["nchange"])
    assert not np.array_equal(refs[0][0]["gamma"], tr2["gamma"])        # (spec 4's variates are others)
