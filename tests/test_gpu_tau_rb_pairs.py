"""The Rao-Blackwellised joint posterior of two haplotypes' bases from the resident traces (dsm_ctx_trace_rb_pairs; kernels_rbpair.hip;
DESIGN.md sec. 8l) on the GPU, against the numpy restatement tests/_tau_rb_pairs_ref.py.  The traces are planted (debug_set_trace,
debug_set_param_trace): no chain is needed except where the chain itself is the subject.  The conditionals are compared by the
tolerance the restatement derives from operation counts (k_bound), determinism by bits.
Run on an MI355X with:  python -m pytest tests/test_gpu_tau_rb_pairs.py -m gpu
"""
import os

import numpy as np
import pandas as pd
import pytest
from numpy.random import RandomState

from desman_amd import _lib, marginals
from desman_amd.synth import synth_counts, random_state
import _tau_rb_ref as R
import _tau_rb_pairs_ref as RP
from test_gpu_tau_pairs import INSTANTIATIONS

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = r"error -2: ", r"error -3: "
V37 = 37                                  # no multiple of any groups-per-workgroup (4, 8, 16)


@pytest.fixture()
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()
    _lib.rbpair_debug_set_chunk(0)


def _plant(c, x, taus, gammas, etas):
    """the table and a planted trace of len(taus) iterations; the resident state is iteration 0's"""
    c.set_counts(x)
    c.set_state(np.eye(4, dtype=np.int64)[taus[0]], gammas[0], etas[0])
    c.debug_set_trace(taus)
    c.debug_set_param_trace(gammas, etas)


def _same(a, b):
    return a["joint"].tobytes() == b["joint"].tobytes() and a["same_batch"].tobytes() == b["same_batch"].tobytes() and a["dead"] == b["dead"]


# (V, S, G, n): V = 37, n = 12 with S in {3, 16, 17, 40, 64, 65, 130} and G in {2, 3, 5, 8} -- every tiling boundary of tau_shape up to
# 130 samples, a padded last lane or slot at 3, 17, 40, 65, 130 -- then 100 / 200 / 300 / 400 samples for the instantiations those do not
# reach (64 lanes x 2 / 4 / 6 / 8 slots), and one shape at G = 32 (496 pairs, digits above bit 31 of the word)
SHAPES = [(V37, 3, 2, 12), (V37, 16, 8, 12), (V37, 17, 5, 12), (V37, 40, 3, 12), (V37, 64, 8, 12), (V37, 65, 3, 12), (V37, 130, 5, 12),
          (V37, 100, 2, 12), (V37, 200, 3, 12), (V37, 300, 2, 12), (V37, 400, 2, 12), (5, 16, 32, 4)]


def test_the_shapes_reach_every_instantiation_of_the_launcher():
    assert {_lib.rbpair_debug_path(S, G) for _, S, G, _ in SHAPES} == INSTANTIATIONS
    assert {3, 16, 17, 40, 64, 65, 130} <= {S for _, S, _, _ in SHAPES} and {2, 3, 5, 8, 32} == {G for _, _, G, _ in SHAPES}


# ---- 1. the device against the restatement, every instantiation ---------------------------------------------------------------------
@pytest.mark.parametrize("V,S,G,n", SHAPES)
def test_device_against_the_restatement(ctx, V, S, G, n):
    """counts 0..300 with a quarter of the cells zero, a smooth trace (mixture values <= 0.84), L = 2.  |dq| <= q K eps A + K eps per
    iteration, K = k_bound(S, G), summed over the used iterations.  Printed: the largest differences in units of their bounds."""
    rng = RandomState(1000 * S + G)
    x = R.sparse_counts(rng, V, S)
    taus, gammas, etas = R.smooth_trace(rng, n, V, S, G)
    _plant(ctx, x, taus, gammas, etas)
    want = RP.pairs(x, taus, gammas, etas, L=2)
    got = ctx.trace_rb_pairs(2)
    P = G * (G - 1) // 2
    assert (got["B"], got["N"], got["n_used"], got["dead"]) == (want["B"], n, n, 0) and want["dead"] == 0
    assert got["joint"].shape == (V, P, 4, 4) and got["same_batch"].shape == (n // 2, P) and got["pairs"].tolist() == [list(p) for p in RP.pair_list(G)]
    dj, ds = np.abs(got["joint"] - want["joint"]), np.abs(got["same_batch"] - want["same_batch"])
    print("S=%d G=%d: K=%.0f, max |d joint| / bound = %.3g, max |d same| / bound = %.3g"
          % (S, G, RP.k_bound(S, G), (dj / want["tol_joint"]).max(), (ds / want["tol_same"]).max()))
    assert np.all(np.isfinite(got["joint"])) and np.all(np.isfinite(got["same_batch"]))
    assert np.all(dj <= want["tol_joint"]) and np.all(ds <= want["tol_same"])
    assert np.abs(got["joint"].sum(axis=(2, 3)) - n).max() <= 16 * n * R.EPS


# ---- 2. the edges of the model ---------------------------------------------------------------------------------------------------------
def _edge_counts(rng, V, S):
    x = R.sparse_counts(rng, V, S, hi=40, zero_share=0.8)
    x[:5] = 0                                                       # positions without a read: flat
    return x


def test_zeros_in_eta_and_gamma_give_dead_pairs_and_nothing_nan(ctx):
    """S = 19 (16 lanes x 2 slots, thirteen of them padded).  eta row a supplies the bases a and a + 1 only -- exact zeros under the
    padded lanes --, one haplotype has abundance 0 everywhere, another in half of the samples, one sample has a zero row of gamma
    (and reads at some positions only): -inf candidates everywhere, pairs without a live state, pairs with one; the mixture values
    stay at or below 0.8, so the tolerance of the smooth case holds"""
    V, S, G, n = V37, 19, 4, 6
    rng = RandomState(77)
    x = _edge_counts(rng, V, S)
    x[20:, 7] = 0                                                   # sample 7, whose abundances are all zero, has reads at positions < 20 only
    taus = rng.randint(0, 4, size=(n, V, G)).astype(np.int64)
    taus[:, 5:12, :] = taus[:, 5:12, :1]
    gammas = rng.dirichlet(np.ones(G), size=(n, S))
    gammas[:, :, 1] = 0.0
    gammas[:, ::2, 3] = 0.0
    gammas /= gammas.sum(axis=2, keepdims=True)
    gammas[:, 7, :] = 0.0
    eta = np.zeros((4, 4))
    for a in range(4):
        eta[a, a], eta[a, (a + 1) % 4] = 0.8, 0.2
    etas = np.stack([eta] * n)
    _plant(ctx, x, taus, gammas, etas)
    want = RP.pairs(x, taus, gammas, etas, L=1)
    cells = n * V * 6
    assert 0 < want["dead"] < cells
    assert np.isneginf(np.stack([want["res"][t]["L"] for t in range(n)])).any()
    got = ctx.trace_rb_pairs(1)
    print("zeros: %d of %d (position, pair, iteration)s dead" % (got["dead"], cells))
    assert got["dead"] == want["dead"]
    assert np.all(np.isfinite(got["joint"])) and np.all(np.isfinite(got["same_batch"])) and np.all(got["joint"] >= 0)
    assert np.all(np.abs(got["joint"] - want["joint"]) <= want["tol_joint"])
    assert np.all(np.abs(got["same_batch"] - want["same_batch"]) <= want["tol_same"])
    assert np.array_equal(got["joint"][:5], np.full((5, 6, 4, 4), n * 0.0625))             # no read: all sixteen alike
    assert np.abs(got["joint"].sum(axis=(2, 3)) - n).max() <= 16 * n * R.EPS
    # a dead pair is the one-hot of the current pair: where every iteration of a (position, pair) is dead, joint counts the pairs
    alld = np.all(np.stack([want["res"][t]["dead"] for t in range(n)]), axis=0)
    assert alld.any()
    for v, pi in np.argwhere(alld):
        g, h = RP.pair_list(G)[pi]
        assert np.array_equal(got["joint"][v, pi].reshape(16), np.bincount(4 * taus[:, v, g] + taus[:, v, h], minlength=16).astype(np.float64))


def test_eta_identity(ctx):
    """eta = I: a haplotype supplies its own base and no other; mixture values reach 1, so the tolerance is the one without a floor"""
    V, S, G, n = V37, 5, 3, 4
    rng = RandomState(78)
    x = _edge_counts(rng, V, S)
    taus = rng.randint(0, 4, size=(n, V, G)).astype(np.int64)
    gammas = rng.dirichlet(np.ones(G), size=(n, S))
    etas = np.stack([np.eye(4)] * n)
    _plant(ctx, x, taus, gammas, etas)
    want = RP.pairs(x, taus, gammas, etas, L=1, no_floor=True)
    got = ctx.trace_rb_pairs(1)
    print("identity: %d dead" % got["dead"])
    assert got["dead"] == want["dead"] > 0
    assert np.all(np.isfinite(got["joint"])) and np.all(np.isfinite(got["same_batch"]))
    assert np.all(np.abs(got["joint"] - want["joint"]) <= want["tol_joint"])
    assert np.all(np.abs(got["same_batch"] - want["same_batch"]) <= want["tol_same"])


# ---- 3. the same bits: twice, and for every cut into chunks ----------------------------------------------------------------------------
def test_the_same_bits_call_to_call_and_for_every_chunk(ctx):
    V, S, G, n = V37, 20, 5, 8
    rng = RandomState(9)
    x = R.sparse_counts(rng, V, S)
    taus, gammas, etas = R.smooth_trace(rng, n, V, S, G)
    perm = np.stack([rng.permutation(G) for _ in range(n)]).astype(np.uint8)
    _plant(ctx, x, taus, gammas, etas)
    first = ctx.trace_rb_pairs(2, perm=perm)
    assert _same(first, ctx.trace_rb_pairs(2, perm=perm))
    for chunk in (1, 7, 16, 0):
        _lib.rbpair_debug_set_chunk(chunk)
        assert _same(first, ctx.trace_rb_pairs(2, perm=perm)), chunk
        for only in ("joint", "same_batch"):                        # an output that is not asked for changes neither the other nor the chunks' sums
            assert ctx.trace_rb_pairs(2, perm=perm, want=(only,))[only].tobytes() == first[only].tobytes(), (chunk, only)
    assert ctx.lib.dsm_ctx_trace_rb_pairs(ctx._h, None, 0, n, 1, 2, None, None, None) == 0           # every output NULL


# ---- 4. labels and stride --------------------------------------------------------------------------------------------------------------
def test_perm_and_stride_against_the_restatement(ctx):
    V, S, G, n = V37, 33, 4, 23
    rng = RandomState(23)
    x = R.sparse_counts(rng, V, S)
    taus, gammas, etas = R.smooth_trace(rng, n, V, S, G)
    perm = np.stack([rng.permutation(G) for _ in range(n)]).astype(np.uint8)
    _plant(ctx, x, taus, gammas, etas)
    got = ctx.trace_rb_pairs(1, perm=perm, stride=3)                  # iterations 0, 3, ..., 21: eight, B = 8
    want = RP.pairs(x, taus, gammas, etas, perm=perm, L=1, stride=3)
    assert (got["n_used"], got["B"], got["N"]) == (8, 8, 8) == (want["n_used"], want["B"], want["N"])
    assert np.all(np.abs(got["joint"] - want["joint"]) <= want["tol_joint"]) and np.all(np.abs(got["same_batch"] - want["same_batch"]) <= want["tol_same"])
    ident = ctx.trace_rb_pairs(1, stride=3)
    assert got["joint"].tobytes() != ident["joint"].tobytes()
    assert _same(ident, ctx.trace_rb_pairs(1, perm=np.tile(np.arange(G, dtype=np.uint8), (n, 1)), stride=3))
    # the batch rule on the taken iterations: stride 2 takes twelve, L = 5 uses the last ten of them (2, 4, ..., 22 -> 4 ... 22)
    got = ctx.trace_rb_pairs(5, perm=perm, stride=2)
    want = RP.pairs(x, taus, gammas, etas, perm=perm, L=5, stride=2)
    assert (got["n_used"], got["B"], got["N"]) == (12, 2, 10) == (want["n_used"], want["B"], want["N"])
    assert np.all(np.abs(got["joint"] - want["joint"]) <= want["tol_joint"]) and np.all(np.abs(got["same_batch"] - want["same_batch"]) <= want["tol_same"])
    # a row that is no permutation, in an iteration the stride does not take: DSM_ERR_ARG, and nothing is written
    bad = perm.copy(); bad[1] = (0, 1, 2, 2)
    joint, same = np.full((V, 6, 16), 7.0), np.full((8, 6), 7.0)
    dead = _lib.C.c_longlong(5)
    rc = ctx.lib.dsm_ctx_trace_rb_pairs(ctx._h, _lib._ptr(bad), 0, n, 3, 1, _lib._ptr(joint), _lib._ptr(same), _lib.C.byref(dead))
    assert rc == -2 and np.all(joint == 7.0) and np.all(same == 7.0) and dead.value == 5
    with pytest.raises(ValueError):
        ctx.trace_rb_pairs(1, perm=perm[:3], n_it=n)


# ---- 5. a real chain: only read -----------------------------------------------------------------------------------------------------------
def test_a_real_chain_continues_bit_for_bit(ctx):
    V, S, G, n = V37, 16, 3, 6
    counts, _, _ = synth_counts(V, S, G, seed=31)
    tau, gamma, eta = random_state(V, S, G, seed=32)
    twin = _lib.Context(0)
    try:
        for c in (ctx, twin):
            c.set_counts(counts); c.set_state(tau, gamma, eta); c.seed(4321, ctr_seed=0xABCDEF12345)
            c.set_tau_rng(_lib.RNG_MT19937)
            c.gibbs_update(n)
        got = ctx.trace_rb_pairs(1)
        assert _same(got, ctx.trace_rb_pairs(1))
        assert got["N"] == n and np.abs(got["joint"].sum(axis=(2, 3)) - n).max() <= 16 * n * R.EPS
        # the device read the triples dsm_ctx_trace_fit_stats reads: tau as get_tau_at(t) returns it, row t of the gamma and eta traces
        tr = ctx.get_trace()
        taus = np.stack([np.argmax(ctx.get_tau_at(t), axis=2) for t in range(n)])
        want = RP.pairs(counts, taus, tr["gamma"], tr["eta"], L=1, no_floor=True)        # (the chain's eta has a diagonal above 0.85)
        assert want["dead"] == got["dead"]
        assert np.all(np.abs(got["joint"] - want["joint"]) <= want["tol_joint"])
        assert np.array_equal(ctx.get_mt_state(), twin.get_mt_state()) and ctx.counters() == twin.counters()
        a, b = ctx.get_trace(), twin.get_trace()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        ctx.gibbs_update(n); twin.gibbs_update(n)
        a, b = ctx.get_trace(), twin.get_trace()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        for t in range(-1, n):
            assert ctx.get_tau_at(t).tobytes() == twin.get_tau_at(t).tobytes(), t
        for p, q in zip(ctx.get_state(), twin.get_state()):
            assert p.tobytes() == q.tobytes()
        sa, sb = ctx.get_star(), twin.get_star()
        assert sa["lp"] == sb["lp"] and sa["it"] == sb["it"] and np.array_equal(sa["tau"], sb["tau"])
        assert np.array_equal(ctx.get_mt_state(), twin.get_mt_state()) and ctx.counters() == twin.counters()
    finally:
        twin.close()


# ---- 6. error codes ---------------------------------------------------------------------------------------------------------------------
def test_error_codes_one_haplotype_the_empty_range_and_a_held_tau(ctx):
    x = R.sparse_counts(RandomState(1), 5, 3)
    taus, gammas, etas = R.smooth_trace(RandomState(2), 6, 5, 3, 2)
    with pytest.raises(_lib.DesmanHipError, match=ERR_STATE):
        ctx.trace_rb_pairs(1, n_it=0)
    ctx.set_counts(x)
    ctx.set_state(np.eye(4, dtype=np.int64)[taus[0]], gammas[0], etas[0])
    with pytest.raises(_lib.DesmanHipError, match=ERR_STATE + ".*no update has run"):
        ctx.trace_rb_pairs(1, n_it=0)
    ctx.debug_set_trace(taus)
    ctx.debug_set_param_trace(gammas, etas)
    for call in (lambda: ctx.trace_rb_pairs(4), lambda: ctx.trace_rb_pairs(1, n_it=1), lambda: ctx.trace_rb_pairs(0), lambda: ctx.trace_rb_pairs(-2),
                 lambda: ctx.trace_rb_pairs(0, n_it=0), lambda: ctx.trace_rb_pairs(1, stride=0), lambda: ctx.trace_rb_pairs(1, stride=-1),
                 lambda: ctx.trace_rb_pairs(2, stride=2),                 # three taken iterations are fewer than two batches of 2
                 lambda: ctx.trace_rb_pairs(1, it0=-1, n_it=2), lambda: ctx.trace_rb_pairs(1, it0=5, n_it=2),
                 lambda: ctx.trace_rb_pairs(1, it0=7, n_it=0), lambda: ctx.trace_rb_pairs(1, n_it=-1)):
        with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
            call()
    assert ctx.trace_rb_pairs(3)["N"] == 6 and ctx.trace_rb_pairs(1, stride=3)["N"] == 2      # the context stays usable
    joint = np.full((5, 1, 16), 7.0)
    dead = _lib.C.c_longlong(5)
    assert ctx.lib.dsm_ctx_trace_rb_pairs(ctx._h, None, 6, 0, 1, 2 ** 30, _lib._ptr(joint), None, _lib.C.byref(dead)) == 0
    assert not joint.any() and dead.value == 0                       # n_it = 0 writes zeros
    # one haplotype: no pair, success, nothing written
    one = _lib.Context(0)
    try:
        t1, g1, e1 = R.smooth_trace(RandomState(3), 4, 5, 3, 1)
        _plant(one, x, t1, g1, e1)
        r = one.trace_rb_pairs(1)
        assert r["joint"].shape == (5, 0, 4, 4) and r["same_batch"].shape == (4, 0) and r["pairs"].shape == (0, 2) and r["dead"] == 0
        dead = _lib.C.c_longlong(5)
        assert one.lib.dsm_ctx_trace_rb_pairs(one._h, None, 0, 4, 1, 1, None, None, _lib.C.byref(dead)) == 0 and dead.value == 5
        with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
            one.trace_rb_pairs(3)                                    # the arguments are checked all the same
    finally:
        one.close()
    # after an update that held tau every iteration is the held tau
    held = _lib.Context(0)
    try:
        counts, _, _ = synth_counts(V37, 8, 3, seed=5, depth_scale=0.05)
        tau, gamma, eta = random_state(V37, 8, 3, seed=6)
        held.set_counts(counts); held.set_state(tau, gamma, eta); held.seed(5, ctr_seed=99)
        held.gibbs_update_fixed_tau(4, pool=0)
        tr = held.get_trace()
        got = held.trace_rb_pairs(1)
        want = RP.pairs(counts, np.stack([np.argmax(tau, axis=2)] * 4), tr["gamma"], tr["eta"], L=1, no_floor=True)
        assert got["dead"] == want["dead"] and np.all(np.abs(got["joint"] - want["joint"]) <= want["tol_joint"])
        assert np.all(np.abs(got["same_batch"] - want["same_batch"]) <= want["tol_same"])
    finally:
        held.close()


# ---- 7. the command line ------------------------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_desman_marginal_pairs(tmp_path, caplog, monkeypatch):
    """a run with and without the flag (both with --relabel, for SND_posterior.csv): the files of the run without it are the same
    bytes, SND_rb.csv and Tau_pairs.csv are recomputed here from what Context.trace_rb_pairs returned to the run, and the expected
    distance agrees with the count distance of SND_posterior.csv within 4 of the larger of the two standard errors (the posterior sd
    over sqrt(iterations) there, the batch-means MCSE here)"""
    import logging
    from desman_amd import cli
    V, S, G, n = 200, 12, 3, 40
    # one per cent of the usual depth, about 23 reads per position over all samples (-m 0 keeps the shallow samples): a chain that keeps
    # moving.  On a deeper table no base flips in 40 iterations, the count distance has a standard error of 0 and only its 1 / n
    # resolution is left to compare against
    counts, _, _ = synth_counts(V, S, G, seed=123, depth_scale=0.01)
    freq = str(tmp_path / "fit.freq")
    _write_freq(freq, counts, ["S%d" % s for s in range(S)], ["contig%d" % (v // 50) for v in range(V)], np.arange(V) * 7 + 3)
    plain, both = str(tmp_path / "plain"), str(tmp_path / "both")
    args = [freq, "-g", str(G), "-i", str(n), "-s", "7", "-m", "0", "--relabel"]
    cli.main(args + ["-o", plain, "--marginals"])
    seen = []
    real = _lib.Context.trace_rb_pairs

    def spy(self, *a, **k):
        seen.append((a, k, real(self, *a, **k)))
        return seen[-1][2]
    monkeypatch.setattr(_lib.Context, "trace_rb_pairs", spy)
    with caplog.at_level(logging.INFO):
        cli.main(args + ["-o", both, "--marginals", "--marginal-pairs"])
    assert any("of kind phase" in r.getMessage() and "the closest pair is" in r.getMessage() for r in caplog.records)
    assert sorted(os.listdir(both)) == sorted(os.listdir(plain) + ["SND_rb.csv", "Tau_pairs.csv"])
    read = lambda d, name: open(os.path.join(d, name), "rb").read()
    for name in os.listdir(plain):                             # with the flag the other files are what they were
        if name != "log_file.txt":
            assert read(plain, name) == read(both, name), name
    assert len(seen) == 1
    (a, k, stats) = seen[0]
    assert a == (6,) and k["stride"] == 1 and k["perm"] is not None and stats["N"] == 36        # floor(sqrt(40)); 40 // max(50, 12) = 0 -> 1
    Gk = stats["pairs"].max() + 1                              # the chain may have merged identical haplotypes
    P = len(stats["pairs"])
    J = stats["joint"] / stats["N"]
    snd = pd.read_csv(os.path.join(both, "SND_rb.csv"))
    assert list(snd.columns) == ["g", "h", "dist", "dist_mcse", "differ", "star"] and len(snd) == P
    assert np.array_equal(snd[["g", "h"]].to_numpy(), stats["pairs"])
    means = stats["same_batch"] / 6.0
    assert np.allclose(snd["dist"], V - means.mean(axis=0), rtol=1e-12) and np.allclose(snd["dist_mcse"], means.std(axis=0, ddof=1) / np.sqrt(6), rtol=1e-9)
    psame = np.trace(J, axis1=2, axis2=3)
    assert np.allclose(snd["differ"], (psame < 0.5).mean(axis=0), rtol=1e-12)
    star = pd.read_csv(os.path.join(both, "Filtered_Tau_star.csv"), index_col=0).to_numpy()[:, 1:].reshape(V, Gk, 4).argmax(axis=2)
    assert np.array_equal(snd["star"], [(star[:, g] != star[:, h]).sum() for g, h in stats["pairs"]])
    post = pd.read_csv(os.path.join(both, "SND_posterior.csv"))
    assert np.array_equal(post[["g", "h"]].to_numpy(), stats["pairs"])
    se = np.maximum(post["sd"].to_numpy() / np.sqrt(n), snd["dist_mcse"].to_numpy())
    print("dist rb %s, counts %s, larger se %s" % (snd["dist"].to_numpy(), post["mean"].to_numpy(), se))
    assert np.all(np.abs(snd["dist"].to_numpy() - post["mean"].to_numpy()) <= 4 * se)
    # Tau_pairs.csv: the rows where a call of Tau_calls.csv is below 0.9, position-major
    calls = pd.read_csv(os.path.join(both, "Tau_calls.csv"))
    prob = calls["prob"].to_numpy().reshape(V, Gk)
    rows = pd.read_csv(os.path.join(both, "Tau_pairs.csv"))
    assert list(rows.columns) == ["Contig", "Position", "g", "h", "pair", "prob", "p_same", "swap", "mi", "kind"]
    want = [(v, pi) for v in range(V) for pi, (g, h) in enumerate(stats["pairs"]) if min(prob[v, g], prob[v, h]) < 0.9]
    assert len(rows) == len(want) > 0
    vv, pp = np.array(want).T
    assert np.array_equal(rows["Position"], vv * 7 + 3) and np.array_equal(rows[["g", "h"]].to_numpy(), stats["pairs"][pp])
    Jf = J[vv, pp]
    flat = Jf.reshape(-1, 16)
    assert list(rows["pair"]) == ["ACGT"[k >> 2] + "ACGT"[k & 3] for k in flat.argmax(axis=1)]
    assert np.allclose(rows["prob"], flat.max(axis=1), rtol=1e-12) and np.allclose(rows["p_same"], psame[vv, pp], rtol=1e-12, atol=1e-15)
    swap = sum(2 * np.minimum(Jf[:, a, b], Jf[:, b, a]) for a in range(4) for b in range(a + 1, 4))
    assert np.allclose(rows["swap"], swap, rtol=1e-12, atol=1e-15)
    with np.errstate(divide="ignore", invalid="ignore"):
        mi = np.where(Jf > 0, Jf * np.log(Jf / (Jf.sum(axis=2)[:, :, None] * Jf.sum(axis=1)[:, None, :])), 0.0).sum(axis=(1, 2))
    assert np.allclose(rows["mi"], np.maximum(mi, 0), rtol=1e-9, atol=1e-12)
    assert set(rows["kind"]) <= {"phase", "base"} and list(rows["kind"]) == list(marginals.pair_tables(Jf)["kind"])
