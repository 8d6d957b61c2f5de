"""Rao-Blackwellised tau marginals from the resident traces (dsm_ctx_trace_rb_marginals; kernels_rbtau.hip) on the GPU,
against the numpy restatement tests/_tau_rb_ref.py.  The traces are planted (debug_set_trace, debug_set_param_trace): no chain is
needed except where the chain itself is the subject.  The conditionals are compared by the tolerance DESIGN.md derives
(_tau_rb_ref.k_bound), the accumulation over iterations, labels and batches by bits.

A call always uses an even number of batches, so neither a single iteration nor a single batch can be asked for on its own.  Where a
test needs one, it plants the iterations TWICE in a row and halves the result: x + x and x^2 + x^2 are exact in binary floating point,
so half of the call's `sum` is the single batch sum and half of its `bsq` the square of it, to the bit.
Run on an MI355X with:  python -m pytest tests/test_gpu_tau_rb.py -m gpu
"""
import os

import numpy as np
import pandas as pd
import pytest
from numpy.random import RandomState

from desman_amd import _lib
from desman_amd.synth import synth_counts, random_state
import _tau_rb_ref as R

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = r"error -2: ", r"error -3: "
V37 = 37                                  # no multiple of any groups-per-workgroup (4, 8, 16)


@pytest.fixture()
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _plant(c, x, taus, gammas, etas, counts=True):
    """the table and a planted trace of len(taus) iterations; the resident state is iteration 0's"""
    if counts:
        c.set_counts(x)
        c.set_state(np.eye(4, dtype=np.int64)[taus[0]], gammas[0], etas[0])
    c.debug_set_trace(taus)
    c.debug_set_param_trace(gammas, etas)


# the smallest S of every instantiation tau_shape can return (S = 1 among them), and 70: no multiple of its 32 lanes per position
SIZES = [1, 17, 33, 49, 65, 70, 97, 129, 193, 257, 385]


def test_the_sizes_cover_every_instantiation():
    first = {}
    for S in range(1, 513):
        first.setdefault(_lib.rbtau_debug_path(S, 1), S)
    assert sorted(set(first.values()) | {70}) == SIZES and len(first) == 10
    assert _lib.rbtau_debug_path(70, 1) == (32, 3) and _lib.rbtau_debug_path(512, 32) == (64, 8)


# ---- 1. the device against the restatement, every instantiation ---------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2, 5, 12, 32])
@pytest.mark.parametrize("S", SIZES)
def test_device_against_the_restatement(ctx, S, G):
    """V = 37, n_it = 6, counts 0..300 with a quarter of the cells zero; L = 1 and L = 3.  |dq| <= q K eps A + K eps per iteration,
    K = k_bound(S, G), summed over the used iterations.  Printed: the largest difference in units of its bound."""
    rng = RandomState(1000 * S + G)
    x = R.sparse_counts(rng, V37, S)
    taus, gammas, etas = R.smooth_trace(rng, 6, V37, S, G)
    _plant(ctx, x, taus, gammas, etas)
    res = None
    for L in (1, 3):
        want = R.marginals(x, taus, gammas, etas, L=L, res=res)
        res = want["res"]
        assert want["pmax"] <= 0.85 and want["dead"] == 0 and want["N"] == 6
        got = ctx.trace_rb_marginals(L)
        assert (got["B"], got["N"], got["dead"]) == (want["B"], 6, 0)
        d = np.abs(got["sum"] - want["sum"])
        print("S=%d G=%d L=%d: K=%.0f, max |d sum| / bound = %.3g" % (S, G, L, R.k_bound(S, G), (d / want["tol"]).max()))
        assert np.all(np.isfinite(got["sum"])) and np.all(d <= want["tol"])
        # bsq: d(b^2) <= (2 b + db) db per batch, b <= L
        assert np.all(np.abs(got["bsq"] - want["bsq"]) <= (2.0 * L + want["tol"]) * want["tol"] + 6 * L * L * R.EPS)
        assert np.abs(got["sum"].sum(axis=2) - 6.0).max() <= 4 * 6 * R.EPS


# ---- 2. exact zeros ----------------------------------------------------------------------------------------------------------------
def test_zeros_in_eta_and_gamma_give_dead_cells_and_nothing_nan(ctx):
    """eta row a supplies the bases a and a + 1 only, one haplotype has abundance 0 everywhere, another in half of the samples: -inf
    candidates everywhere, cells without a live base (two seen bases that no single row supplies), cells with one; the mixture values
    stay at or below 0.8, so the tolerance of the smooth case holds"""
    V, S, G, n = V37, 19, 4, 6
    rng = RandomState(77)
    x = R.sparse_counts(rng, V, S, hi=40, zero_share=0.8)
    x[:5] = 0                                                       # positions without a read: flat
    taus = rng.randint(0, 4, size=(n, V, G)).astype(np.int64)
    taus[:, 5:12, :] = taus[:, 5:12, :1]                              # every haplotype the same base: the rest supplies two bases only
    gammas = rng.dirichlet(np.ones(G), size=(n, S))
    gammas[:, :, 1] = 0.0
    gammas[:, ::2, 3] = 0.0
    gammas /= gammas.sum(axis=2, keepdims=True)
    eta = np.zeros((4, 4))
    for a in range(4):
        eta[a, a], eta[a, (a + 1) % 4] = 0.8, 0.2
    etas = np.stack([eta] * n)
    _plant(ctx, x, taus, gammas, etas)
    want = R.marginals(x, taus, gammas, etas, L=1)
    cells = n * V * G
    assert 0 < want["dead"] < cells and want["pmax"] <= 0.85
    assert np.isneginf(np.stack([R.conditionals(x, taus[t], gammas[t], etas[t])["L"] for t in range(n)])).any()
    got = ctx.trace_rb_marginals(1)
    print("zeros: %d of %d cell-iterations dead" % (got["dead"], cells))
    assert got["dead"] == want["dead"]
    assert np.all(np.isfinite(got["sum"])) and np.all(np.isfinite(got["bsq"])) and np.all(got["sum"] >= 0)
    assert np.all(np.abs(got["sum"] - want["sum"]) <= want["tol"])
    assert np.array_equal(got["sum"][:5], np.full((5, G, 4), n * 0.25))
    assert np.abs(got["sum"].sum(axis=2) - n).max() <= 4 * n * R.EPS


# ---- 3. labels -----------------------------------------------------------------------------------------------------------------------
def test_perm_moves_the_columns_bit_for_bit(ctx):
    V, S, G, n = V37, 20, 5, 6
    rng = RandomState(9)
    x = R.sparse_counts(rng, V, S)
    taus, gammas, etas = R.smooth_trace(rng, n, V, S, G)
    perm = np.stack([rng.permutation(G) for _ in range(n)]).astype(np.uint8)
    _plant(ctx, x, taus, gammas, etas)
    got = ctx.trace_rb_marginals(1, perm=perm)
    ident = ctx.trace_rb_marginals(1)
    assert ctx.trace_rb_marginals(1, perm=np.tile(np.arange(G, dtype=np.uint8), (n, 1)))["sum"].tobytes() == ident["sum"].tobytes()
    # every iteration alone (planted twice, halved: see the module's docstring), permuted and added on the host in t order
    twice = np.repeat(np.arange(n), 2)
    _plant(ctx, x, taus[twice], gammas[twice], etas[twice], counts=False)
    s, b = np.zeros((V, G, 4)), np.zeros((V, G, 4))
    for t in range(n):
        one = ctx.trace_rb_marginals(1, it0=2 * t, n_it=2)
        q = one["sum"] / 2.0
        assert (one["bsq"] / 2.0).tobytes() == (q * q).tobytes()
        s[:, perm[t], :] = s[:, perm[t], :] + q
        b[:, perm[t], :] = b[:, perm[t], :] + q * q
    assert got["sum"].tobytes() == s.tobytes() and got["bsq"].tobytes() == b.tobytes()
    assert got["sum"].tobytes() != ident["sum"].tobytes()
    # a row that is no permutation, in a used and in a skipped iteration
    dup = perm[:n].copy(); dup[4] = (0, 1, 2, 3, 3)
    big = perm[:n].copy(); big[0] = (0, 1, 2, 3, 5)
    with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
        ctx.trace_rb_marginals(1, perm=dup, n_it=n)
    with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
        ctx.trace_rb_marginals(2, perm=np.concatenate([big, perm[:1]]), n_it=n + 1)       # row 0 is skipped at n_it = 7, L = 2
    with pytest.raises(ValueError):
        ctx.trace_rb_marginals(1, perm=perm[:3], n_it=n)


# ---- 4. batches ----------------------------------------------------------------------------------------------------------------------
def test_batches_skipped_iterations_null_outputs_and_the_empty_range(ctx):
    V, S, G, n, L = V37, 33, 3, 23, 5
    rng = RandomState(23)
    x = R.sparse_counts(rng, V, S)
    taus, gammas, etas = R.smooth_trace(rng, n, V, S, G)
    perm = np.stack([rng.permutation(G) for _ in range(n)]).astype(np.uint8)
    _plant(ctx, x, taus, gammas, etas)
    got = ctx.trace_rb_marginals(L, perm=perm)
    want = R.marginals(x, taus, gammas, etas, perm=perm, L=L)
    assert (got["B"], got["N"]) == (4, 20) == (want["B"], want["N"])
    assert np.all(np.abs(got["sum"] - want["sum"]) <= want["tol"])
    assert np.abs(got["sum"].sum(axis=2) - 20.0).max() <= 4 * 20 * R.EPS
    # the first three iterations are skipped: the call over the last twenty gives the same bits
    tail = ctx.trace_rb_marginals(L, perm=perm[3:], it0=3, n_it=20)
    assert tail["sum"].tobytes() == got["sum"].tobytes() and tail["bsq"].tobytes() == got["bsq"].tobytes()
    for only in ("sum", "bsq"):
        assert ctx.trace_rb_marginals(L, perm=perm, want=(only,))[only].tobytes() == got[only].tobytes()
    assert ctx.lib.dsm_ctx_trace_rb_marginals(ctx._h, None, 0, n, L, None, None, None) == 0         # every output NULL
    # error codes; the context stays usable
    for call in (lambda: ctx.trace_rb_marginals(12), lambda: ctx.trace_rb_marginals(6, n_it=11), lambda: ctx.trace_rb_marginals(1, n_it=1),
                 lambda: ctx.trace_rb_marginals(0), lambda: ctx.trace_rb_marginals(-2), lambda: ctx.trace_rb_marginals(0, n_it=0),
                 lambda: ctx.trace_rb_marginals(1, it0=-1, n_it=2), lambda: ctx.trace_rb_marginals(1, it0=22, n_it=2),
                 lambda: ctx.trace_rb_marginals(1, it0=24, n_it=0), lambda: ctx.trace_rb_marginals(1, n_it=-1)):
        with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
            call()
    assert ctx.trace_rb_marginals(11)["N"] == 22
    z = ctx.trace_rb_marginals(2 ** 30, it0=n, n_it=0)
    assert z["N"] == 0 and z["dead"] == 0 and not z["sum"].any() and not z["bsq"].any()
    buf = np.full((V, G, 4), 7.0)
    dead = _lib.C.c_longlong(5)
    assert ctx.lib.dsm_ctx_trace_rb_marginals(ctx._h, None, 0, 0, 1, _lib._ptr(buf), None, _lib.C.byref(dead)) == 0
    assert not buf.any() and dead.value == 0                         # n_it = 0 writes zeros
    # every batch alone: its five iterations planted twice in a row, the call over those ten halved
    used = np.arange(3, 23)
    twice = np.concatenate([np.tile(used[5 * k:5 * k + 5], 2) for k in range(4)])
    _plant(ctx, x, taus[twice], gammas[twice], etas[twice], counts=False)
    s, b = np.zeros((V, G, 4)), np.zeros((V, G, 4))
    for k in range(4):
        one = ctx.trace_rb_marginals(L, perm=perm[twice[10 * k:10 * k + 10]], it0=10 * k, n_it=10)
        assert one["B"] == 2
        bs = one["sum"] / 2.0
        assert (one["bsq"] / 2.0).tobytes() == (bs * bs).tobytes()
        s, b = s + bs, b + bs * bs
    assert got["sum"].tobytes() == s.tobytes() and got["bsq"].tobytes() == b.tobytes()


def test_no_update_has_run(ctx):
    x = R.sparse_counts(RandomState(1), 5, 3)
    taus, gammas, etas = R.smooth_trace(RandomState(2), 1, 5, 3, 2)
    with pytest.raises(_lib.DesmanHipError, match=ERR_STATE):
        ctx.trace_rb_marginals(1, n_it=0)
    ctx.set_counts(x)
    ctx.set_state(np.eye(4, dtype=np.int64)[taus[0]], gammas[0], etas[0])
    with pytest.raises(_lib.DesmanHipError, match=ERR_STATE + ".*no update has run"):
        ctx.trace_rb_marginals(1, n_it=0)


# ---- 5. a real chain: only read, the same bits twice -----------------------------------------------------------------------------------
def test_a_real_chain_continues_bit_for_bit(ctx):
    V, S, G, n = 64, 16, 3, 8
    counts, _, _ = synth_counts(V, S, G, seed=31)
    tau, gamma, eta = random_state(V, S, G, seed=32)
    twin = _lib.Context(0)
    try:
        for c in (ctx, twin):
            c.set_counts(counts); c.set_state(tau, gamma, eta); c.seed(4321, ctr_seed=0xABCDEF12345)
            c.set_tau_rng(_lib.RNG_MT19937)
            c.gibbs_update(n)
        before = ctx.trace_batch_stats(2)
        got = ctx.trace_rb_marginals(2)
        again = ctx.trace_rb_marginals(2)
        assert got["sum"].tobytes() == again["sum"].tobytes() and got["bsq"].tobytes() == again["bsq"].tobytes() and got["dead"] == again["dead"]
        assert got["N"] == n and np.abs(got["sum"].sum(axis=2) - n).max() <= 4 * n * R.EPS
        # the device read the triples dsm_ctx_trace_fit_stats reads: tau as get_tau_at(t) returns it, row t of the gamma and eta traces
        tr = ctx.get_trace()
        taus = np.stack([np.argmax(ctx.get_tau_at(t), axis=2) for t in range(n)])
        want = R.marginals(counts, taus, tr["gamma"], tr["eta"], L=2, data_floor=True)     # (the chain's eta has a diagonal above 0.85)
        assert want["pmax"] < 0.999 and want["dead"] == got["dead"]
        assert np.all(np.abs(got["sum"] - want["sum"]) <= want["tol"])
        after = ctx.trace_batch_stats(2)
        for k in ("sum", "first", "bsq", "flips"):
            assert before[k].tobytes() == after[k].tobytes(), k
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


# ---- 6. the command line ---------------------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_desman_marginals(tmp_path, caplog):
    import logging
    from desman_amd import cli
    V, S, G, n = 50, 8, 3, 40
    counts, _, _ = synth_counts(V, S, G, seed=123)
    freq = str(tmp_path / "fit.freq")
    _write_freq(freq, counts, ["S%d" % s for s in range(S)], ["contig%d" % (v // 20) for v in range(V)], np.arange(V) * 7 + 3)
    plain, marg, rel = (str(tmp_path / d) for d in ("plain", "marg", "rel"))
    args = [freq, "-g", str(G), "-i", str(n), "-s", "7"]
    cli.main(args + ["-o", plain])
    with caplog.at_level(logging.INFO):
        cli.main(args + ["-o", marg, "--marginals"])
    assert any("calls expected wrong" in r.getMessage() and "dead cell-iterations" in r.getMessage() for r in caplog.records)
    cli.main(args + ["-o", rel, "--marginals", "--relabel", "--diagnose", "4"])
    extra = ["Tau_Mean_rb.csv", "Tau_rb_MCSE.csv", "Tau_calls.csv"]
    assert sorted(os.listdir(marg)) == sorted(os.listdir(plain) + extra)
    read = lambda d, name: open(os.path.join(d, name), "rb").read()
    for name in os.listdir(plain):                             # with the flag the usual files are what they were
        if name != "log_file.txt":
            assert read(plain, name) == read(marg, name) == read(rel, name), name
    mean = pd.read_csv(os.path.join(plain, "Tau_Mean.csv"), index_col=0)
    rb = pd.read_csv(os.path.join(marg, "Tau_Mean_rb.csv"), index_col=0)
    mcse = pd.read_csv(os.path.join(marg, "Tau_rb_MCSE.csv"), index_col=0)
    Gk = (mean.shape[1] - 1) // 4                               # the chain may have merged identical haplotypes
    assert rb.shape == mean.shape == mcse.shape == (V, 1 + 4 * Gk)
    assert list(rb.index) == list(mean.index) and list(rb.columns) == list(mean.columns) and np.array_equal(rb["Position"], mean["Position"])
    p = rb.to_numpy()[:, 1:].astype(np.float64).reshape(V, Gk, 4)
    assert np.abs(p.sum(axis=2) - 1.0).max() <= 1e-12 and np.all(p >= 0)
    e = mcse.to_numpy()[:, 1:].astype(np.float64)
    assert np.all(np.isfinite(e)) and np.all(e >= 0) and np.all(e <= 0.5)
    calls = pd.read_csv(os.path.join(marg, "Tau_calls.csv"))
    assert list(calls.columns) == ["Contig", "Position", "haplotype", "call", "prob", "star", "agree", "entropy"] and len(calls) == V * Gk
    assert np.array_equal(calls["haplotype"], np.tile(np.arange(Gk), V)) and np.array_equal(calls["Position"], np.repeat(mean["Position"].to_numpy(), Gk))
    assert np.array_equal(calls["call"], p.argmax(axis=2).reshape(-1)) and np.allclose(calls["prob"], p.max(axis=2).reshape(-1), rtol=1e-12)
    star = pd.read_csv(os.path.join(plain, "Filtered_Tau_star.csv"), index_col=0).to_numpy()[:, 1:].reshape(V, Gk, 4).argmax(axis=2)
    assert np.array_equal(calls["star"], star.reshape(-1)) and np.array_equal(calls["agree"], (calls["call"] == calls["star"]).astype(int))
    assert np.all(calls["entropy"] >= 0) and np.all(calls["entropy"] <= np.log(4.0) + 1e-12)
    # under a relabelling the mean takes the suffix Tau_Mean.csv takes; the batch length is --diagnose's
    assert "Tau_Mean_rb_relabelled.csv" in os.listdir(rel) and "Tau_Mean_rb.csv" not in os.listdir(rel)
    assert {"Tau_rb_MCSE.csv", "Tau_calls.csv", "Tau_Mean_relabelled.csv", "Tau_MCSE.csv"} <= set(os.listdir(rel))
    pr = pd.read_csv(os.path.join(rel, "Tau_Mean_rb_relabelled.csv"), index_col=0).to_numpy()[:, 1:].astype(np.float64).reshape(V, Gk, 4)
    assert np.abs(pr.sum(axis=2) - 1.0).max() <= 1e-12
