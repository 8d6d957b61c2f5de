"""The launch of stats_big_kernel between stage 1 of the aggregated mu/E pass and the Dirichlet launch is a matter of speed only
(dsm_ctx_set_big_launch: 1 = always, the path every chain took before; 0 = never, the Dirichlet launch draws the deferred items
itself; -1 = while the lists were last seen non-empty).  Every mode must give the same chain bit for bit.

Tables (synth_counts, seed 7, started from the table's own tau / gamma and eta = 0.96 I + 0.01, so the chain fits):
  shallow  depth_scale 1: the rarer outcome of an item has a mean of a few reads, no item is handed over (mean <= 64);
  deep     depth_scale 40: depths of 1 600 ... 20 000 reads per cell, error rate ~0.03 -> means of 50 ... 600: many cells hand over
           in every iteration;
  mixed    (64, 17, 3) at depth_scale 4 (up to ~2 000 reads of a base) started with eta = 0.775 on the diagonal, 0.075 off it: at
           that matrix 735 items have a rarer-outcome mean above 64; at the matrix the chain settles at (error rate ~0.01) none
           has, so the first iteration(s) hand items over and the later ones do not.
Which iterations hand items over is worked out on the CPU from the states a chain stepped one iteration at a time passes
through, with stage 1's own rule (dsm_binom.h: s1_item -- x min(ws, wl) > 64 (ws + wl)), and asserted per table."""
import numpy as np
import pytest

from _deferred import handed_over as _handed_over

pytestmark = pytest.mark.gpu

SHAPES = [(48, 5, 2), (64, 17, 3), (40, 64, 8), (32, 70, 4)]          # (32, 70, 4): S > 64
SHALLOW, DEEP = 1.0, 40.0
MIXED = ((64, 17, 3), 4.0, 0.7)                                        # shape, depth_scale, diagonal of the starting eta
N_IT = 6


def _table(shape, scale, diag=0.96):
    from desman_amd.synth import synth_counts
    V, S, G = shape
    counts, tt, gg = synth_counts(V, S, G, 7, depth_scale=scale)
    tau = np.zeros((V, G, 4), dtype=np.int64)
    np.put_along_axis(tau, tt.astype(np.int64)[..., None], 1, axis=2)
    eta = diag * np.eye(4) + (1.0 - diag) / 4.0
    eta /= eta.sum(axis=1, keepdims=True)
    return counts, tau, np.ascontiguousarray(gg), eta


def _ctx(table, mode):
    from desman_amd import _lib
    counts, tau, gamma, eta = table
    c = _lib.Context(0)
    c.set_counts(counts)
    c.force_stats_spec(2)                    # (the shape rule gives tables this small the per-read pass)
    c.set_state(tau, gamma, eta)
    c.seed(99)
    c.set_big_launch(mode)
    return c


def _result(c):
    t, g, e = c.get_state()
    tr = c.get_trace()
    st = c.get_star()
    return dict(tau=t, gamma=g, eta=e, ll=tr["ll"], lp=tr["lp"], gtr=tr["gamma"], etr=tr["eta"], nch=tr["nchange"],
                s_tau=st["tau"], s_gamma=st["gamma"], s_eta=st["eta"], s_lp=np.float64(st["lp"]), s_it=np.int64(st["it"]))


def _same(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "%s: %s differs" % (what, k)


def _items_per_iteration(table):
    """[N_IT] items handed over in each iteration of the chain (CPU, from the states a stepped chain passes through)"""
    c = _ctx(table, 1)
    out = []
    for _ in range(N_IT):
        t, g, e = c.get_state()
        out.append(_handed_over(table[0], t, g, e))
        c.gibbs_update(1)
    c.close()
    return out


_cache = {}


def _reference(key, table):
    """the chain with the launch always made (the path before this choice existed), once per table"""
    if key not in _cache:
        c = _ctx(table, 1)
        c.gibbs_update(N_IT)
        assert c.get_timing()["stats_big"][1] == N_IT
        _cache[key] = _result(c)
        c.close()
    return _cache[key]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("depth", ["shallow", "deep"])
def test_chain_is_the_same_in_every_mode(shape, depth):
    table = _table(shape, SHALLOW if depth == "shallow" else DEEP)
    items = _items_per_iteration(table)
    print("items handed over per iteration", shape, depth, items)
    if depth == "shallow":
        assert max(items) == 0, items
    else:
        assert min(items) > 0, items
    ref = _reference((shape, depth), table)
    for mode in (0, -1):
        c = _ctx(table, mode)
        c.gibbs_update(N_IT)
        nz, seen = c.debug_big_lists()
        launches = c.get_timing()["stats_big"][1]
        _same(ref, _result(c), "mode %d" % mode)
        assert nz == 0
        if mode == 0:
            assert launches == 0
            assert seen == (0 if depth == "shallow" else N_IT)          # one closing of the lists per iteration that handed items over
        else:
            assert launches == N_IT                                      # the first call after set_state launches
        c.close()


def test_one_chain_takes_both_paths():
    shape, scale, diag = MIXED
    table = _table(shape, scale, diag)
    items = _items_per_iteration(table)
    print("items handed over per iteration (mixed)", items)
    n_with = sum(1 for n in items if n > 0)
    assert 0 < n_with < N_IT, items
    ref = _reference("mixed", table)
    c = _ctx(table, 0)
    c.gibbs_update(N_IT)
    _same(ref, _result(c), "mode 0")
    nz, seen = c.debug_big_lists()
    assert nz == 0 and seen == n_with
    c.close()


@pytest.mark.parametrize("shape", [(40, 64, 8), (32, 70, 4)])
def test_one_pass_without_the_launch_matches_the_oracle(shape):
    from oracle import cbind
    table = _table(shape, DEEP)
    counts, tau, gamma, eta = table
    assert _handed_over(counts, tau, gamma, eta) > 0
    c = _ctx(table, 0)
    ctr_seed = 0x0123456789ABCDEF
    c.seed(1, ctr_seed=ctr_seed)
    seen = 0
    for it in (0, 5):
        mu, E = c.sample_stats(it)
        assert c.get_timing()["stats_big"][1] == 0
        mu_ref, E_ref = cbind.stats_agg(cbind.onehot_to_idx(tau), gamma, eta, counts, ctr_seed, it)
        assert np.array_equal(mu, mu_ref) and np.array_equal(E, E_ref)      # every item drawn once: none lost, none twice
        assert int(mu.sum()) == int(counts.sum()) == int(E.sum())
        nz, seen = c.debug_big_lists()
        assert nz == 0
    assert seen == 2
    c.close()


def test_batched_chains_without_the_launch():
    from desman_amd import _lib
    shape = (40, 64, 8)
    table = _table(shape, DEEP)
    counts, tau, gamma, eta = table
    rng = np.random.default_rng(5)
    starts = [np.ascontiguousarray(rng.dirichlet(np.ones(shape[2]), size=shape[1])) for _ in range(3)]
    alone = []
    for k, g0 in enumerate(starts):
        c = _ctx((counts, tau, g0, eta), 1)
        c.seed(200 + k)
        c.gibbs_update(N_IT)
        alone.append(_result(c))
        c.close()
    ctxs = []
    for k, g0 in enumerate(starts):
        c = _ctx((counts, tau, g0, eta), 0)
        c.seed(200 + k)
        ctxs.append(c)
    _lib.Context.batch_gibbs_update(ctxs, N_IT)
    for k, c in enumerate(ctxs):
        _same(alone[k], _result(c), "chain %d of the batch" % k)
        nz, seen = c.debug_big_lists()
        assert nz == 0 and seen == N_IT
        c.close()


def test_automatic_mode_follows_the_lists():
    for depth, scale in (("deep", DEEP), ("shallow", SHALLOW)):
        c = _ctx(_table((40, 64, 8), scale), -1)
        c.gibbs_update(N_IT)                                  # first call after set_state: launched
        n0 = c.get_timing()["stats_big"][1]
        assert n0 == N_IT
        c.gibbs_update(N_IT)
        n1 = c.get_timing()["stats_big"][1] - n0
        assert n1 == (N_IT if depth == "deep" else 0), (depth, n1)
        c.close()
