"""dsm_fit_gamma on the MI355X: abundances of fitted haplotypes in samples that were not in the fit, against
the numpy restatement of tests/_abund_ref.py (checked on its own in tests/test_abund_cpu.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _abund_ref as R  # noqa: E402

from desman_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_G = 1e-12                  # gamma, absolute
TOL_L = 1e-12                  # loglik, deviance: relative to max(|L|, 1)
N50 = dict(max_iter=50, tol=0.0)


def _compare(got, counts, tau, eta, what, n_iter=50, presence=False):
    """every sample of `got` against the restatement after n_iter steps; returns the worst (gamma, L, deviance, lr) distances, the last
    three in units of max(|L|, 1)"""
    worst = np.zeros(4)
    for s in range(counts.shape[1]):
        ref = R.fit(counts[:, s], tau, eta, n_iter=n_iter)
        scale = max(abs(ref["loglik"]), 1.0) if np.isfinite(ref["loglik"]) else 1.0
        assert got["iters"][s] == ref["iters"] and got["converged"][s] == ref["converged"], (what, s)
        if not np.isfinite(ref["loglik"]):
            assert got["loglik"][s] == ref["loglik"] and not got["gamma"][s].any() and got["deviance"][s] == np.inf, (what, s)
            continue
        d = [np.abs(got["gamma"][s] - ref["gamma"]).max(), abs(got["loglik"][s] - ref["loglik"]) / scale,
             abs(got["deviance"][s] - ref["deviance"]) / scale, 0.0]
        if presence:
            G = tau.shape[1]
            want = np.array([R.lr_absent(counts[:, s], tau, eta, g, n_iter=n_iter) for g in range(G)])
            inf = np.isinf(want)
            assert np.array_equal(np.isinf(got["lr_absent"][s]), inf) and (got["lr_absent"][s] >= 0).all(), (what, s)
            if (~inf).any():
                d[3] = np.abs(got["lr_absent"][s][~inf] - want[~inf]).max() / scale
        worst = np.maximum(worst, d)
    print("%s: gamma %.2e, loglik %.2e, deviance %.2e, lr_absent %.2e (the last three / max(|L|, 1))" % ((what,) + tuple(worst)))
    assert worst[0] <= TOL_G and worst[1] <= TOL_L and worst[2] <= TOL_L and worst[3] <= TOL_L, (what, worst)
    return worst


# ---- 1. equality with the restatement ------------------------------------------------------------------------------------------
SHAPES = [(V, 8, 2) for V in (1, 63, 64, 65, 257, 1000)] + [(257, G, 2) for G in (1, 2, 3, 9, 16, 31, 32)] + [(257, 8, S) for S in (1, 65)] \
    + [(2049, 8, 2), (4100, 3, 2)]          # more positions than one LDS tile (2048): the streaming path, two and three tiles


@pytest.mark.parametrize("V,G,S", SHAPES, ids=["V%d-G%d-S%d" % t for t in SHAPES])
def test_fifty_steps_equal_the_restatement(V, G, S):
    """tol = 0, max_iter = 50: gamma within 1e-12, loglik, deviance and lr_absent within 1e-12 max(|L|, 1).  The presence fits run for
    the small sample counts (every grouping of the 1 + G fits)."""
    counts, tau, eta, _ = R.synth(V, S, G, depth=20, seed=100 + V + G + S)
    presence = S <= 2
    got = _lib.fit_gamma(counts, tau, eta, presence=presence, **N50)
    assert got["gamma"].shape == (S, G) and np.allclose(got["gamma"].sum(axis=1), 1.0, atol=1e-12)
    _compare(got, counts, tau, eta, "V=%d G=%d S=%d" % (V, G, S), presence=presence)


def test_sparse_tables_an_empty_sample_and_a_deep_cell():
    counts, tau, eta, _ = R.synth(257, 4, 8, depth=20, seed=7, zero_frac=0.3)
    assert (counts == 0).mean() > 0.3
    counts[:, 1, :] = 0                                                   # N = 0 next to normal samples
    counts[5, 2] = [2147483000, 300, 200, 100]                            # a depth just below 2^31 in one cell
    got = _lib.fit_gamma(counts, tau, eta, presence=True, **N50)
    assert np.array_equal(got["gamma"][1], np.full(8, 0.125)) and got["loglik"][1] == 0.0 and got["deviance"][1] == 0.0
    assert got["iters"][1] == 0 and got["converged"][1] == 1 and not got["lr_absent"][1].any()
    _compare(got, counts, tau, eta, "sparse", presence=True)


# ---- 2. masked fits ------------------------------------------------------------------------------------------------------------
def test_lr_absent_of_an_absent_a_dominant_and_a_duplicated_haplotype():
    """lr_absent against the restatement at 400 steps (1e-12 |L|), and "about 0" for either of a duplicate pair.  About 0, not 0 to
    rounding: without one duplicate the other takes its share, so both fits have the same maximum L*, but after 400 steps each is still
    below it (haplotype 1 is absent, and EM is slow at the boundary).  L is concave, so at any gamma of the simplex
    L* - L(gamma) <= max_g dL/dgamma_g - sum_g gamma_g dL/dgamma_g = N (max_g grad_g - 1), grad the KKT gradient over the allowed
    haplotypes.  The full fit is at most L*, hence lr_absent = 2 (L_full - L_restricted) <= 2 N (max grad - 1) at the restricted fit --
    taken at the restatement's point, plus the 1e-12 |L| to which the device's figure equals the restatement's.  (Here 1.2e-3, against
    0.027 for the haplotype that is truly absent; the figure itself is 5.6e-8 in the restatement as on the device.)"""
    V, G = 257, 4
    rs = np.random.RandomState(21)
    _, tau, eta, _ = R.synth(V, 1, G, seed=21)
    tau[:, 3] = tau[:, 2]                                                 # haplotypes 2 and 3 are duplicates
    gamma = np.array([[0.5, 0.0, 0.3, 0.2]])                              # 1 is truly absent, 0 carries half the reads
    p = np.einsum("sg,vgb->vsb", gamma, eta[tau])
    counts = np.array([[rs.multinomial(60, p[v, 0])] for v in range(V)], dtype=np.int64)
    got = _lib.fit_gamma(counts, tau, eta, presence=True, max_iter=400, tol=0.0)
    ref = R.fit(counts[:, 0], tau, eta, n_iter=400)
    want = np.array([R.lr_absent(counts[:, 0], tau, eta, g, n_iter=400) for g in range(G)])
    scale = abs(ref["loglik"])
    print("lr_absent", got["lr_absent"][0], "restatement", want, "gamma", got["gamma"][0])
    assert np.abs(got["lr_absent"][0] - want).max() <= TOL_L * scale
    assert want[0] > 1000.0 and want[1] < 5.0                             # the figures mean something
    N = counts.sum()
    for g in (2, 3):                                                      # either duplicate can go
        rest = R.fit(counts[:, 0], tau, eta, n_iter=400, mask=g)
        gap = N * (np.delete(R.kkt_gradient(counts[:, 0], tau, eta, rest["gamma"]), g).max() - 1.0)
        print("duplicate %d: lr_absent %.3e, bound 2 * %.3e" % (g, got["lr_absent"][0][g], gap))
        assert 0.0 <= got["lr_absent"][0][g] <= 2.0 * gap + TOL_L * scale and 2.0 * gap < 0.1 * want[1]
    assert abs(got["gamma"][0][2:].sum() - ref["gamma"][2:].sum()) <= TOL_G                                 # (their split is not compared)
    assert np.abs(got["gamma"][0][:2] - ref["gamma"][:2]).max() <= TOL_G


# ---- 3. convergence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,G,depth,seed", R.INTERIOR)
def test_default_settings_converge_on_interior_tables(V, G, depth, seed):
    counts, tau, eta, _ = R.synth(V, 2, G, depth=depth, seed=seed)
    got = _lib.fit_gamma(counts, tau, eta)
    for s in range(2):
        assert got["converged"][s] == 1 and 0 < got["iters"][s] < _lib.FIT_MAX_ITER
        ref = R.fit(counts[:, s], tau, eta, n_iter=int(got["iters"][s]))
        mine, theirs = R.kkt_residual(counts[:, s], tau, eta, got["gamma"][s]), R.kkt_residual(counts[:, s], tau, eta, ref["gamma"])
        print("V=%d G=%d sample %d: %d steps, KKT residual %.3e (restatement at that count %.3e)" % (V, G, s, got["iters"][s], mine, theirs))
        assert mine <= 2.0 * theirs
    # L along max_iter = 1, 2, 4 .. 64: non-decreasing -- up to the 1e-12 |L| to which a value of L is known at all
    ll = np.array([_lib.fit_gamma(counts, tau, eta, max_iter=n, tol=0.0)["loglik"] for n in (1, 2, 4, 8, 16, 32, 64)])
    print("V=%d G=%d: largest decrease of L along max_iter = 1 .. 64: %.2e |L|" % (V, G, max(0.0, (-np.diff(ll, axis=0) / np.abs(ll[:-1])).max())))
    assert (np.diff(ll, axis=0) >= -TOL_L * np.abs(ll[:-1])).all() and (ll[-1] > ll[0]).all()


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------
def _same(a, b, keys=("gamma", "loglik", "deviance", "iters", "converged")):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys)


@pytest.mark.parametrize("V,G", [(257, 8), (2100, 9)])
def test_results_are_bit_equal_across_runs_chunks_presence_and_entry_points(V, G):
    S = 5
    counts, tau, eta, _ = R.synth(V, S, G, depth=20, seed=31)
    kw = dict(max_iter=40, tol=1e-6)
    base = _lib.fit_gamma(counts, tau, eta, presence=True, **kw)
    assert _same(base, _lib.fit_gamma(counts, tau, eta, presence=True, **kw), keys=("gamma", "loglik", "deviance", "iters", "converged", "lr_absent"))
    assert _same(base, _lib.fit_gamma(counts, tau, eta, presence=False, **kw))
    try:
        for chunk in (1, 3):
            _lib.abund_debug_set_chunk(chunk)
            assert _same(base, _lib.fit_gamma(counts, tau, eta, presence=True, **kw), keys=("gamma", "loglik", "deviance", "iters", "converged", "lr_absent")), chunk
    finally:
        _lib.abund_debug_set_chunk(0)
    ctx = _lib.Context(0)
    try:
        ctx.set_counts(counts)
        assert _same(base, ctx.fit_gamma(eta, tau=tau, presence=True, **kw), keys=("gamma", "loglik", "deviance", "iters", "converged", "lr_absent"))
        onehot = np.zeros((V, G, 4), dtype=np.int64)
        np.put_along_axis(onehot, tau[..., None], 1, axis=2)
        ctx.set_state(onehot, np.full((S, G), 1.0 / G), eta)
        assert _same(base, ctx.fit_gamma(eta, presence=False, **kw))              # the resident tau
        _lib.abund_debug_set_chunk(2)
        assert _same(base, ctx.fit_gamma(eta, tau=onehot, **kw))                  # one-hot input, chunks of the resident tensor
    finally:
        _lib.abund_debug_set_chunk(0)
        ctx.close()


# ---- 5. degenerate operands ----------------------------------------------------------------------------------------------------
def test_exact_zeros_in_eta():
    V, G, S = 70, 3, 3
    rs = np.random.RandomState(4)
    tau = rs.randint(0, 4, size=(V, G))
    tau[0] = [0, 1, 2]
    gamma = rs.dirichlet(np.ones(G) * 3, size=S)
    counts = np.zeros((V, S, 4), dtype=np.int64)
    for v in range(V):
        for s in range(S):
            np.add.at(counts[v, s], tau[v], rs.multinomial(30, gamma[s]))        # reads of the bases the haplotypes carry: consistent
    counts[0, 1, 3] = 2                                                           # sample 1: two T where the haplotypes carry A, C, G
    eye = np.eye(4)
    got = _lib.fit_gamma(counts, tau, eye, presence=True, **N50)
    assert not got["gamma"][1].any() and got["loglik"][1] == -np.inf and got["deviance"][1] == np.inf
    assert got["converged"][1] == 0 and got["iters"][1] == 0 and np.isnan(got["lr_absent"][1]).all()
    keep = [0, 2]
    sub = {k: v[keep] for k, v in got.items()}
    _compare(sub, counts[:, keep], tau, eye, "identity eta, consistent counts", presence=True)
    assert np.isinf(sub["lr_absent"]).any()                                       # position 0: each haplotype alone explains its base
    alone = _lib.fit_gamma(counts[:, keep], tau, eye, presence=True, **N50)
    assert _same(sub, alone, keys=("gamma", "loglik", "deviance", "iters", "converged", "lr_absent"))      # the dead sample touches no other


def test_one_haplotype():
    counts, tau, eta, _ = R.synth(65, 3, 1, seed=9)
    got = _lib.fit_gamma(counts, tau, eta, presence=True)
    assert np.abs(got["gamma"] - 1.0).max() <= TOL_G and (got["converged"] == 1).all() and (got["iters"] == 1).all()
    assert np.isinf(got["lr_absent"]).all() and (got["lr_absent"] > 0).all()
    for s in range(3):
        ref = R.fit(counts[:, s], tau, eta, n_iter=1)
        assert abs(got["loglik"][s] - ref["loglik"]) <= TOL_L * abs(ref["loglik"])


# ---- 6. arguments ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_err_arg_and_leave_the_library_usable():
    counts, tau, eta, _ = R.synth(65, 2, 3, seed=2)
    good = _lib.fit_gamma(counts, tau, eta, **N50)
    lib = _lib.load()
    out = _lib._fit_out(2, 3, False)
    ptrs = [_lib._ptr(out[k]) for k in ("gamma", "loglik", "deviance", "iters", "converged")]

    def raw(x=counts, t=tau, e=eta, G=3, p=ptrs):
        return lib.dsm_fit_gamma(0, np.ascontiguousarray(x), 65, 2, G, np.ascontiguousarray(t), np.ascontiguousarray(e), 50, 0.0, 0, *p, None)
    neg = counts.copy(); neg[3, 1, 0] = -4
    bad_eta = eta.copy(); bad_eta[2, 2] = np.nan
    cases = dict(G0=dict(G=0), G33=dict(G=33, t=np.zeros((65, 33), dtype=np.int64)), negative=dict(x=neg), eta=dict(e=bad_eta),
                 null=dict(p=[None] * 5))
    for name, kw in cases.items():
        assert raw(**kw) == -2, name                                              # DSM_ERR_ARG
        assert lib.dsm_last_error()
        assert raw() == 0, name                                                   # the next valid call succeeds ...
        assert np.array_equal(out["gamma"], good["gamma"]) and np.array_equal(out["loglik"], good["loglik"]), name


# ---- 7. classes and command line -------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.arange(V)[:, None] * 7 + 3, counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=["contig%d" % (v // 50) for v in range(V)], columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)
    return df


def test_end_to_end_on_a_fitted_run(tmp_path):
    """A chain on a synthetic 240 x 12 table (G = 3, the generator of sec. 8a: mean depth 40 .. 500 by sample): fitGamma() on the chain's own counts with tau_star / eta_star lies
    within 5 posterior standard deviations of Gamma_mean in every entry (the distances are printed).  Then
    `desman` on ten of the samples and `desman-abund` for all twelve."""
    from numpy.random import RandomState
    from desman_amd import abund, cli, sampletau
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    from desman_amd.Init_NMFT import Init_NMFT
    from desman_amd.synth import synth_counts
    V, S, G = 240, 12, 3
    counts, _, _ = synth_counts(V, S, G, seed=123)
    rng = RandomState(7)
    sampletau.initRNG()
    sampletau.setRNG(7)
    try:
        nmft = Init_NMFT(counts, G, rng)
        nmft.factorize()
        chain = HaploSNP_Sampler(counts, G, rng, max_iter=100, ctx=nmft._ctx)
        chain.tau = np.copy(nmft.get_tau(), order='C')
        chain.updateTauIndices()
        chain.gamma = np.copy(nmft.get_gamma(), order='C')
        chain.update()
        chain.update()
    finally:
        sampletau.freeRNG()
    got = chain.fitGamma(presence=True)
    assert (got["converged"] == 1).all() and got["gamma"].shape == (S, chain.G)
    mean, sd = chain.gammaMean(), chain.gamma_store.std(axis=0, ddof=1)
    z = np.abs(got["gamma"] - mean) / sd
    print("fitGamma vs Gamma_mean: largest distance %.2f posterior sd (median %.2f), iters %d..%d, largest |difference| %.2e"
          % (z.max(), np.median(z), got["iters"].min(), got["iters"].max(), np.abs(got["gamma"] - mean).max()))
    assert (z <= 5.0).all()
    again = chain.fitGamma(snps=counts, presence=True)                            # the same samples as a new table
    assert _same(got, again, keys=("gamma", "loglik", "deviance", "iters", "converged", "lr_absent"))

    names = ["S%d" % s for s in range(S)]
    freq = str(tmp_path / "ten.freq")
    _write_freq(freq, counts[:, :10, :], names[:10])
    run = str(tmp_path / "run")
    cli.main([freq, "-g", str(G), "-i", "40", "-o", run, "-s", "7"])
    full = str(tmp_path / "all.freq")
    _write_freq(full, counts, names)
    out = str(tmp_path / "projected")
    abund.main([run, full, "-o", out, "--presence"])
    proj = pd.read_csv(os.path.join(out, "Projected_Gamma.csv"), index_col=0)
    star = pd.read_csv(os.path.join(run, "Gamma_star.csv"), index_col=0)
    assert list(proj.index) == names and list(proj.columns) == list(star.columns)
    assert np.allclose(proj.to_numpy().sum(axis=1), 1.0, atol=1e-9) and (proj.to_numpy() >= 0).all()
    fit = pd.read_csv(os.path.join(out, "Projected_fit.csv"), index_col=0)
    assert list(fit.index) == names and (fit["converged"] == 1).all() and (fit["deviance"] > 0).all() and (fit["reads"] > 0).all()
    pres = pd.read_csv(os.path.join(out, "Projected_presence.csv"), index_col=0)
    assert pres.shape == proj.shape and (pres.to_numpy() >= 0).all()
    print("desman-abund: projected - Gamma_star over the ten fitted samples: largest |difference| %.3e"
          % np.abs(proj.loc[list(star.index)].to_numpy() - star.to_numpy()).max())
    out2 = str(tmp_path / "new_only")
    abund.main([run, full, "-o", out2, "--only-new"])
    new = pd.read_csv(os.path.join(out2, "Projected_Gamma.csv"), index_col=0, float_precision="round_trip")
    assert list(new.index) == [n for n in names if n not in set(star.index)] and len(new) >= 2
    both = pd.read_csv(os.path.join(out, "Projected_Gamma.csv"), index_col=0, float_precision="round_trip")
    assert np.array_equal(new.to_numpy(), both.loc[list(new.index)].to_numpy())
