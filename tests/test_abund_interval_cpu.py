"""Profile-likelihood intervals of the projected abundances (dsm_fit_gamma_interval, `desman-abund --interval`): what can be checked
without a GPU -- the numpy restatement of tests/_abund_interval_ref.py against the definition (the threshold at the reported ends, a
constrained optimiser, coverage of the generating abundances, nesting of the levels), the interface, and the command line's file."""
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _abund_ref as R  # noqa: E402
import _abund_interval_ref as I  # noqa: E402

from desman_amd import _lib  # noqa: E402

Q95 = I.quantile(0.95)
CTOL = 1e-6
# The largest |l(default stop rule) - l(20 000 steps, tol 0)| at the reported ends of the three INTERIOR tables (sample 0; the first
# from the search's own inner fit, the second from ghat's free part): 6.8e-13 / 1.4e-11 / 7.3e-12 (measured; |L| = 1.1e3 .. 5.7e3, so this
# is the rounding of the sums -- the stop rule leaves a step below 1e-9 and L is flat to second order at the constrained maximum).
# DELTA is ten times the largest.
GAP_MEASURED = 1.4e-11
DELTA = 10.0 * GAP_MEASURED


def test_quantile_is_the_chi_square_quantile():
    assert abs(Q95 - 3.841458820694124) < 1e-12 and abs(I.quantile(0.99) - 6.6348966010212145) < 1e-11
    assert _lib.chi2_quantile(0.95) == Q95
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            _lib.chi2_quantile(bad)


def _long_profiles(x, E, ghat, gs, cs, steps=20000):
    """l_g(c) for many (g, c) at once with the inner fit run `steps` steps (tol = 0) from ghat's free part: the restatement's inner
    fit, rows batched so that 20 000 steps stay affordable"""
    x = np.asarray(x, dtype=np.float64)
    V, G = E.shape[0], E.shape[1]
    K = len(gs)
    Em = E.transpose(1, 0, 2).reshape(G, V * 4)
    xf = x.reshape(V * 4)
    pos = xf > 0
    free = np.ones((K, G), dtype=bool)
    free[np.arange(K), gs] = False
    c = np.asarray(cs, dtype=np.float64)[:, None]
    w = np.where(free, ghat[None, :], 0.0)
    w = w / w.sum(axis=1, keepdims=True)
    gam = np.where(free, (1.0 - c) * (0.999 * w + 0.001 / (G - 1)), c)
    for _ in range(steps if G > 2 else 0):
        p = gam @ Em
        q = np.where(pos, xf / np.where(pos, p, 1.0), 0.0)
        r = gam * (q @ Em.T)
        gam = np.where(free, (1.0 - c) * r / np.where(free, r, 0.0).sum(axis=1, keepdims=True), c)
    p = gam @ Em
    return (xf[pos] * np.log(p[:, pos])).sum(axis=1)


# ---- 1. the threshold at the reported ends ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,G,depth,seed", R.INTERIOR)
def test_reported_ends_sit_at_the_threshold(V, G, depth, seed):
    """l from a long inner fit (20 000 steps, tol 0): the deviance at a reported end is <= q + DELTA, one ctol further out >= q - DELTA"""
    counts, tau, eta, _ = R.synth(V, 2, G, depth=depth, seed=seed)
    x = counts[:, 0]
    E = R.emission(tau, eta)
    ghat = R.fit(x, tau, eta, max_iter=20000, tol=1e-9)["gamma"]
    trace = []
    lo, hi, flags = I.interval(x, tau, eta, ghat, Q95, ctol=CTOL, trace=trace)
    assert not flags.any() and (lo > 0).all() and (hi < 1).all()          # interior tables: no boundary, no fit at max_iter
    Lhat = trace[0][4]
    gs, cs = [], []
    for g in range(G):
        for c in (lo[g], lo[g] - CTOL, hi[g], hi[g] + CTOL):
            assert 0.0 <= c <= 1.0
            gs.append(g); cs.append(c)
    ll = _long_profiles(x, E, ghat, np.array(gs), cs)
    dev = (2.0 * (Lhat - ll)).reshape(G, 4)
    by_c = {(g, side, c): l for g, side, c, l, _ in trace}
    gap = max(abs(by_c[(g, side, c)] - ll[4 * g + 2 * side]) for g in range(G) for side, c in ((0, lo[g]), (1, hi[g])))
    print("V=%d G=%d: deviance - q at the ends %.3e .. %.3e, one ctol out %.3e .. %.3e; largest |l(default stop) - l(long)| %.3e"
          % (V, G, (dev[:, [0, 2]] - Q95).min(), (dev[:, [0, 2]] - Q95).max(), (dev[:, [1, 3]] - Q95).min(),
             (dev[:, [1, 3]] - Q95).max(), gap))
    assert (dev[:, [0, 2]] <= Q95 + DELTA).all()
    assert (dev[:, [1, 3]] >= Q95 - DELTA).all()


# ---- 2. an independent optimiser ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,G,depth,seed", R.INTERIOR)
def test_constrained_optimiser_finds_no_higher_profile(V, G, depth, seed):
    """SLSQP over the free haplotypes (their sum fixed at 1 - c) finds no l_g(c) above the restatement's beyond 1e-9 |L|: four c"""
    optimize = pytest.importorskip("scipy.optimize")
    counts, tau, eta, _ = R.synth(V, 2, G, depth=depth, seed=seed)
    x = counts[:, 0]
    E = R.emission(tau, eta)
    N = float(x.sum())
    ghat = R.fit(x, tau, eta, max_iter=20000, tol=1e-9)["gamma"]
    g = 1
    free = [h for h in range(G) if h != g]
    for c in (0.0, 0.5 * ghat[g], 0.5 * (ghat[g] + 1.0), 0.9):
        mine = I.profile(x, tau, eta, ghat, g, c)

        def full(f):
            gam = np.empty(G)
            gam[free] = np.maximum(f, 1e-300)
            gam[g] = c
            return gam
        fun = lambda f: -R.loglik(x, E, full(f)) / N
        jac = lambda f: -R.kkt_gradient(x, tau, eta, full(f))[free]
        best = -np.inf
        for f0 in (np.full(G - 1, (1.0 - c) / (G - 1)), (1.0 - c) * np.random.RandomState(1).dirichlet(np.ones(G - 1))):
            opt = optimize.minimize(fun, f0, jac=jac, method="SLSQP", bounds=[(0.0, 1.0)] * (G - 1),
                                    constraints=[dict(type="eq", fun=lambda f: f.sum() - (1.0 - c), jac=lambda f: np.ones(G - 1))],
                                    options=dict(maxiter=500, ftol=1e-15))
            f = np.clip(opt.x, 0.0, None)
            best = max(best, R.loglik(x, E, full(f * (1.0 - c) / f.sum())))
        assert best <= mine + 1e-9 * abs(mine), (c, best, mine)
        assert best >= mine - 1e-6 * abs(mine), (c, best, mine)          # ... and it does find the same hill


# ---- 3. coverage ---------------------------------------------------------------------------------------------------------------------
def test_intervals_cover_the_generating_abundances():
    """V = 65, G = 3, depth 20, 200 samples under the generating tau and eta: the 95 % intervals hold the generating gamma in at least
    90 % of the 600 (sample, haplotype) pairs.  Observed with this seed: 94.7 % (568 of 600)."""
    V, G, S = 65, 3, 200
    counts, tau, eta, truth = R.synth(V, S, G, depth=20, seed=5)
    inside = 0
    for s in range(S):
        ghat = R.fit(counts[:, s], tau, eta, max_iter=20000, tol=1e-9)["gamma"]
        lo, hi, _ = I.interval(counts[:, s], tau, eta, ghat, Q95, ctol=1e-4)
        inside += int(((lo <= truth[s]) & (truth[s] <= hi)).sum())
    print("coverage: %d of %d" % (inside, S * G))
    assert inside >= 0.9 * S * G


# ---- 4. nesting ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,G,depth,seed", R.INTERIOR)
def test_levels_nest_and_hold_the_estimate(V, G, depth, seed):
    counts, tau, eta, _ = R.synth(V, 2, G, depth=depth, seed=seed)
    for s in range(2):
        x = counts[:, s]
        ghat = R.fit(x, tau, eta, max_iter=20000, tol=1e-9)["gamma"]
        lo, hi = {}, {}
        for level in (0.90, 0.95, 0.99):
            lo[level], hi[level], _ = I.interval(x, tau, eta, ghat, I.quantile(level), ctol=CTOL)
            assert (lo[level] <= ghat).all() and (ghat <= hi[level]).all()
        assert (lo[0.99] <= lo[0.95]).all() and (lo[0.95] <= lo[0.90]).all()
        assert (hi[0.90] <= hi[0.95]).all() and (hi[0.95] <= hi[0.99]).all()


# ---- the restatement's special cases ---------------------------------------------------------------------------------------------
def test_restatement_degenerate_operands():
    counts, tau, eta, _ = R.synth(65, 1, 3, seed=3)
    x = counts[:, 0]
    ghat = R.fit(x, tau, eta, max_iter=20000, tol=1e-9)["gamma"]
    lo, hi, fl = I.interval(np.zeros_like(x), tau, eta, np.full(3, 1.0 / 3), Q95)
    assert np.array_equal(lo, np.zeros(3)) and np.array_equal(hi, np.ones(3)) and np.array_equal(fl, [3, 3, 3])
    lo, hi, fl = I.interval(x, tau, eta, np.zeros(3), Q95)
    assert np.isnan(lo).all() and np.isnan(hi).all() and not fl.any()
    lo, hi, fl = I.interval(x, tau[:, :1], eta, np.ones(1), Q95)
    assert lo[0] == 1.0 and hi[0] == 1.0 and fl[0] == 2
    lo, hi, fl = I.interval(x, tau, eta, ghat, Q95, max_iter=1)
    assert (fl & 4).all()                                                # every haplotype had an inner fit that ended at max_iter
    # an absent haplotype: the fit puts it at (nearly) 0 and the lower end is the boundary
    rs = np.random.RandomState(8)
    p = np.einsum("g,vgb->vb", np.array([0.6, 0.4, 0.0]), eta[tau])
    y = np.array([rs.multinomial(40, p[v]) for v in range(65)])
    gh = R.fit(y, tau, eta, max_iter=20000, tol=1e-9)["gamma"]
    lo, hi, fl = I.interval(y, tau, eta, gh, Q95)
    assert lo[2] == 0.0 and fl[2] & 1 and hi[2] < 0.1 and lo[0] > 0.4


# ---- the interface exists ----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_interval_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_fit_gamma_interval", "dsm_ctx_fit_gamma_interval"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(_lib.fit_gamma_interval) and callable(_lib.Context.fit_gamma_interval)
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    assert callable(HaploSNP_Sampler.fitGammaInterval)


def test_bad_interval_arguments_are_refused_before_any_device_work():
    counts = np.ones((5, 2, 4), dtype=np.int64)
    tau = np.zeros((5, 2), dtype=np.int64)
    eta = 0.96 * np.eye(4) + 0.01
    good = np.full((2, 2), 0.5)
    for kw, what in ((dict(q=0.0), "q="), (dict(q=-1.0), "q="), (dict(q=np.inf), "q="), (dict(q=np.nan), "q="), (dict(ctol=0.0), "ctol="),
                     (dict(ctol=1.0), "ctol="), (dict(ctol=np.nan), "ctol=")):
        with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*%s" % what):
            _lib.fit_gamma_interval(counts, tau, eta, good, **kw)
    for row, what in (([-0.1, 1.1], r"outside \[0, 1\]"), ([0.5, 0.6], "sums to"), ([0.5, np.nan], "outside"), ([0.3, 0.3], "sums to")):
        bad = good.copy(); bad[1] = row
        with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*%s" % what):
            _lib.fit_gamma_interval(counts, tau, eta, bad)
    with pytest.raises(ValueError):
        _lib.fit_gamma_interval(counts, tau, eta, np.full((2, 3), 1.0 / 3))          # gamma_hat is not [S, G]
    with pytest.raises(ValueError):
        _lib.fit_gamma_interval(counts, tau, eta, good, level=1.0)


# ---- desman_amd.abund --interval: argument handling and the file -------------------------------------------------------------------
from test_abund_cpu import _freq, _run_dir  # noqa: E402


@pytest.fixture
def fake_calls(monkeypatch):
    """both library calls replaced by recorders: parsing and writing need no GPU"""
    calls = []

    def fit(counts, tau, eta, max_iter=0, tol=0.0, presence=False, device=0):
        S, G = counts.shape[1], tau.shape[1]
        return dict(gamma=np.full((S, G), 1.0 / G), loglik=-np.arange(1.0, S + 1), deviance=np.arange(S) * 0.5,
                    iters=np.arange(S, dtype=np.int32) + 7, converged=np.ones(S, dtype=np.int32))

    def interval(counts, tau, eta, gamma_hat, level=0.95, q=None, max_iter=0, tol=0.0, ctol=0.0, device=0):
        calls.append(dict(gamma_hat=gamma_hat, level=level, max_iter=max_iter, tol=tol, ctol=ctol))
        S, G = gamma_hat.shape
        flags = np.zeros((S, G), dtype=np.int32); flags[1, 0] = 5; flags[0, 1] = 2
        return dict(lo=gamma_hat * 0.5, hi=gamma_hat * 1.5, flags=flags)
    monkeypatch.setattr(_lib, "fit_gamma", fit)
    monkeypatch.setattr(_lib, "fit_gamma_interval", interval)
    return calls


def test_cli_interval_file_layout_and_options(tmp_path, fake_calls, capsys):
    from desman_amd import abund
    run, model = _run_dir(tmp_path)
    freq, _ = _freq(tmp_path, ["N1", "N2"], model["contigs"], model["positions"])
    out = tmp_path / "out"
    abund.main([run, freq, "-o", str(out), "--interval"])
    (call,) = fake_calls
    assert call["level"] == 0.95 and call["ctol"] == abund.CTOL == _lib.FIT_CTOL and call["max_iter"] == abund.MAX_ITER and call["tol"] == abund.TOL
    assert open(out / "Projected_interval.csv").read() == \
        ",0_lo,0_hi,0_flag,1_lo,1_hi,1_flag\nN1,0.25,0.75,0,0.25,0.75,2\nN2,0.25,0.75,5,0.25,0.75,0\n"
    err = capsys.readouterr().err
    assert "N2" in err and "N1" not in err and "max-iter" in err        # the sample with flag bit 4 is named
    out2 = tmp_path / "out2"
    abund.main([run, freq, "-o", str(out2), "--interval", "0.9", "--ctol", "1e-4"])
    assert fake_calls[-1]["level"] == 0.9 and fake_calls[-1]["ctol"] == 1e-4
    out3 = tmp_path / "out3"
    abund.main([run, freq, "-o", str(out3)])
    assert len(fake_calls) == 2 and not os.path.exists(out3 / "Projected_interval.csv")
    for name in ("Projected_Gamma.csv", "Projected_fit.csv"):
        assert open(out / name, "rb").read() == open(out3 / name, "rb").read()
    with pytest.raises(SystemExit):
        abund.main([run, freq, "--interval", "1.5"])
