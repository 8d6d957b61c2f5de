"""Abundances of fitted haplotypes in samples that were not in the fit (dsm_fit_gamma, desman_amd.abund): what can be checked
without a GPU -- the numpy restatement of tests/_abund_ref.py against independent answers (the KKT conditions of the concave
problem, a constrained optimiser), its sensitivity to the order of the sums, and the command line's file handling."""
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _abund_ref as R  # noqa: E402

from desman_amd import _lib  # noqa: E402

# tables with an interior maximum: no duplicate haplotypes, depth >= 20
INTERIOR = R.INTERIOR


def _table(V, G, depth, seed, S=2):
    return R.synth(V, S, G, depth=depth, seed=seed)


@pytest.mark.parametrize("V,G,depth,seed", INTERIOR)
def test_restatement_reaches_the_kkt_point(V, G, depth, seed):
    """20 000 EM steps: gradient 1 on the support to 1e-10 (measured: at most 4.4e-16 -- the iteration contracts linearly and these tables
    reach a step of 1e-10 in under 300 steps, so what is left is the rounding of the sums), the maximiser interior"""
    counts, tau, eta, _ = _table(V, G, depth, seed)
    for s in range(counts.shape[1]):
        got = R.fit(counts[:, s], tau, eta, n_iter=20000)
        assert got["gamma"].min() > 1e-3 and abs(got["gamma"].sum() - 1.0) < 1e-12
        res = R.kkt_residual(counts[:, s], tau, eta, got["gamma"])
        print("V=%d G=%d sample %d: KKT residual %.3e" % (V, G, s, res))
        assert res < 1e-10


@pytest.mark.parametrize("V,G,depth,seed", INTERIOR)
def test_restatement_loglik_is_monotone(V, G, depth, seed):
    counts, tau, eta, _ = _table(V, G, depth, seed)
    got = R.fit(counts[:, 0], tau, eta, n_iter=300, trace=True)
    ll = np.array(got["ll_trace"])
    assert len(ll) == 301
    assert (np.diff(ll) >= -1e-13 * np.abs(ll[:-1])).all()              # non-decreasing up to the rounding of a sum of |L|
    assert ll[-1] > ll[0] + 1.0


@pytest.mark.parametrize("V,G,depth,seed", INTERIOR[:2])
def test_constrained_optimiser_finds_nothing_higher(V, G, depth, seed):
    """SLSQP on the simplex reaches no higher likelihood than EM, beyond 1e-9 |L|"""
    optimize = pytest.importorskip("scipy.optimize")     # no scipy: this independent check cannot run (the KKT test still does)
    counts, tau, eta, _ = _table(V, G, depth, seed)
    x = counts[:, 0]
    E = R.emission(tau, eta)
    em = R.fit(x, tau, eta, n_iter=20000)
    N = float(x.sum())
    fun = lambda g: -R.loglik(x, E, np.maximum(g, 1e-300)) / N
    jac = lambda g: -R.kkt_gradient(x, tau, eta, np.maximum(g, 1e-300))
    best = -np.inf
    for g0 in (R.start(G), np.random.RandomState(1).dirichlet(np.ones(G))):
        opt = optimize.minimize(fun, g0, jac=jac, method="SLSQP", bounds=[(0.0, 1.0)] * G,
                                constraints=[dict(type="eq", fun=lambda g: g.sum() - 1.0, jac=lambda g: np.ones(G))],
                                options=dict(maxiter=500, ftol=1e-15))
        g = np.clip(opt.x, 0.0, None)
        best = max(best, R.loglik(x, E, g / g.sum()))
    assert best <= em["loglik"] + 1e-9 * abs(em["loglik"])
    assert best >= em["loglik"] - 1e-6 * abs(em["loglik"])               # ... and it does find the same hill


def test_order_of_the_sums_moves_gamma_by_rounding_only():
    """forward against reversed position order at equal step counts: the room under the 1e-12 of the device comparison.  Bound: 1e-14
    = 100 ulp of a gamma near 1/2 -- each step's sums carry a few ulp, the iteration contracts, so the difference does not grow."""
    worst = 0.0
    for V, G, depth, seed in INTERIOR + [(1000, 8, 20, 14)]:
        counts, tau, eta, _ = _table(V, G, depth, seed)
        for n in (50, 400):
            a = R.fit(counts[:, 0], tau, eta, n_iter=n)
            b = R.fit(counts[:, 0], tau, eta, n_iter=n, reverse=True)
            worst = max(worst, np.abs(a["gamma"] - b["gamma"]).max())
            assert abs(a["loglik"] - b["loglik"]) <= 1e-13 * abs(a["loglik"])
    print("largest gamma difference forward / reversed: %.3e" % worst)
    assert worst <= 1e-14


def test_restatement_degenerate_operands():
    tau = np.array([[0, 1], [2, 2], [3, 0]])
    x = np.zeros((3, 4), dtype=np.int64)
    got = R.fit(x, tau, np.eye(4), n_iter=5)
    assert np.array_equal(got["gamma"], [0.5, 0.5]) and got["loglik"] == 0.0 and got["iters"] == 0 and got["converged"] == 1
    x[1] = [1, 0, 0, 0]                                                  # both haplotypes carry G there: an A cannot be
    got = R.fit(x, tau, np.eye(4), n_iter=5)
    assert not got["gamma"].any() and got["loglik"] == -np.inf and got["converged"] == 0
    x[1] = [0, 0, 4, 0]; x[0] = [3, 1, 0, 0]                             # consistent: 3 reads of haplotype 0, 1 of haplotype 1
    got = R.fit(x, tau, np.eye(4), n_iter=200)
    np.testing.assert_allclose(got["gamma"], [0.75, 0.25], atol=1e-12)
    assert R.lr_absent(x, tau, np.eye(4), 1, n_iter=50) == np.inf       # without haplotype 1 the C read is impossible
    assert R.lr_absent(x[:, :], tau[:, :1], np.eye(4), 0, n_iter=5) == np.inf          # G = 1


# ---- the interface exists --------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_fit_gamma():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_fit_gamma", "dsm_ctx_fit_gamma", "dsm_abund_debug_set_chunk"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(_lib.fit_gamma) and callable(_lib.Context.fit_gamma)
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    assert callable(HaploSNP_Sampler.fitGamma)


def test_bad_arguments_are_refused_before_any_device_work():
    counts = np.ones((5, 2, 4), dtype=np.int64)
    eta = 0.96 * np.eye(4) + 0.01
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*G=33"):
        _lib.fit_gamma(counts, np.zeros((5, 33), dtype=np.int64), eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*G=0"):
        _lib.fit_gamma(counts, np.zeros((5, 0), dtype=np.int64), eta)
    bad = counts.copy(); bad[3, 1, 2] = -1
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*count -1 at position 3, sample 1"):
        _lib.fit_gamma(bad, np.zeros((5, 2), dtype=np.int64), eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*tau\[2\]\[1\] = 4"):
        t = np.zeros((5, 2), dtype=np.int64); t[2, 1] = 4
        _lib.fit_gamma(counts, t, eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*eta"):
        _lib.fit_gamma(counts, np.zeros((5, 2), dtype=np.int64), eta * np.inf)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*tol"):
        _lib.fit_gamma(counts, np.zeros((5, 2), dtype=np.int64), eta, tol=-1.0)
    with pytest.raises(ValueError):
        _lib.fit_gamma(counts, np.zeros((4, 2), dtype=np.int64), eta)    # tau rows != positions
    with pytest.raises(ValueError):
        _lib.fit_gamma(counts[:, :, :3], np.zeros((5, 2), dtype=np.int64), eta)


# ---- desman_amd.abund: argument handling and file layouts ------------------------------------------------------------------
def _onehot_table(digits, contigs, positions):
    V, G = digits.shape
    oh = np.zeros((V, G, 4), dtype=np.int64)
    np.put_along_axis(oh, digits[..., None], 1, axis=2)
    df = pd.DataFrame(oh.reshape(V, G * 4), index=contigs)
    df["Position"] = positions
    order = df.columns.tolist()
    return df[order[-1:] + order[:-1]]


def _run_dir(tmp_path, fitted=("S0", "S1"), V=6, G=2, collated=False):
    d = tmp_path / "run"
    d.mkdir(exist_ok=True)
    rs = np.random.RandomState(5)
    pd.DataFrame(rs.dirichlet(np.ones(G), size=len(fitted)), index=list(fitted)).to_csv(d / "Gamma_star.csv")
    pd.DataFrame(0.96 * np.eye(4) + 0.01).to_csv(d / "Eta_star.csv")
    contigs = ["c%d" % (v // 2) for v in range(V)]
    positions = np.arange(V) * 3 + 1
    digits = rs.randint(0, 4, size=(V, G))
    _onehot_table(digits, contigs, positions).to_csv(d / "Filtered_Tau_star.csv")
    model = dict(contigs=contigs, positions=positions, digits=digits)
    if collated:                                        # the -r path: more positions than the filtered table
        c2 = contigs + ["c9", "c9"]; p2 = np.concatenate([positions, [5, 8]]); d2 = np.concatenate([digits, rs.randint(0, 4, size=(2, G))])
        _onehot_table(d2, c2, p2).to_csv(d / "Collated_Tau_star.csv")
        model["collated"] = dict(contigs=c2, positions=p2, digits=d2)
    return str(d), model


def _freq(tmp_path, names, contigs, positions, fname="new.freq", seed=6):
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    rs = np.random.RandomState(seed)
    data = np.concatenate([np.asarray(positions)[:, None], rs.poisson(6, size=(len(positions), 4 * len(names)))], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    path = str(tmp_path / fname)
    df.to_csv(path)
    return path, df


@pytest.fixture
def fake_fit(monkeypatch):
    """the library call replaced by a recorder that returns plausible arrays: parsing, matching and writing need no GPU"""
    calls = []

    def fit(counts, tau, eta, max_iter=0, tol=0.0, presence=False, device=0):
        calls.append(dict(counts=counts, tau=tau, eta=eta, max_iter=max_iter, tol=tol, presence=presence))
        S, G = counts.shape[1], tau.shape[1]
        out = dict(gamma=np.full((S, G), 1.0 / G), loglik=-np.arange(1.0, S + 1), deviance=np.arange(S) * 0.5,
                   iters=np.arange(S, dtype=np.int32) + 7, converged=np.ones(S, dtype=np.int32))
        if presence:
            out["lr_absent"] = np.arange(S * G, dtype=np.float64).reshape(S, G)
        return out
    monkeypatch.setattr(_lib, "fit_gamma", fit)
    return calls


def test_cli_matches_positions_by_contig_and_position(tmp_path, fake_fit):
    from desman_amd import abund
    run, model = _run_dir(tmp_path)
    # the table: the model's positions shuffled among rows the model does not know, one contig name shared with another position
    contigs = ["zz", "c0"] + model["contigs"][::-1] + ["c1"]
    positions = [1, 999] + list(model["positions"][::-1]) + [1]
    freq, df = _freq(tmp_path, ["S0", "N1", "N2"], contigs, positions)
    abund.main([run, freq, "-o", str(tmp_path / "out")])
    (call,) = fake_fit
    raw = df.to_numpy()[:, 1:].reshape(len(df), 3, 4)
    want = raw[2:2 + len(model["contigs"])][::-1]
    assert call["counts"].dtype == np.int64 and np.array_equal(call["counts"], want)
    assert np.array_equal(call["tau"], model["digits"]) and call["eta"].shape == (4, 4)
    assert call["max_iter"] == abund.MAX_ITER == _lib.FIT_MAX_ITER and call["tol"] == abund.TOL == _lib.FIT_TOL


def test_cli_missing_model_position_is_named(tmp_path, fake_fit):
    from desman_amd import abund
    run, model = _run_dir(tmp_path)
    freq, _ = _freq(tmp_path, ["N1"], model["contigs"][:-1], model["positions"][:-1])
    with pytest.raises(SystemExit) as e:
        abund.main([run, freq])
    assert "position c2,16 of the model" in str(e.value.code) and not fake_fit


def test_cli_only_new_leaves_out_the_fitted_samples(tmp_path, fake_fit):
    from desman_amd import abund
    run, model = _run_dir(tmp_path, fitted=("S0", "S1"))
    freq, df = _freq(tmp_path, ["N1", "S1", "N2", "S0"], model["contigs"], model["positions"])
    out = tmp_path / "out"
    abund.main([run, freq, "-o", str(out), "--only-new", "--presence"])
    raw = df.to_numpy()[:, 1:].reshape(len(df), 4, 4)
    assert np.array_equal(fake_fit[0]["counts"], raw[:, [0, 2], :]) and fake_fit[0]["presence"]
    assert list(pd.read_csv(out / "Projected_Gamma.csv", index_col=0).index) == ["N1", "N2"]
    freq2, _ = _freq(tmp_path, ["S1", "S0"], model["contigs"], model["positions"], fname="old.freq")
    with pytest.raises(SystemExit) as e:
        abund.main([run, freq2, "--only-new"])
    assert "no sample to fit" in str(e.value.code)


def test_cli_choice_of_the_tau_file(tmp_path, fake_fit):
    from desman_amd import abund
    run, model = _run_dir(tmp_path, collated=True)
    col = model["collated"]
    freq, _ = _freq(tmp_path, ["N1"], col["contigs"], col["positions"])
    abund.main([run, freq, "-o", str(tmp_path / "o1")])                  # the collated table wins over the filtered one
    assert np.array_equal(fake_fit[-1]["tau"], col["digits"])
    other = tmp_path / "mine.csv"
    _onehot_table(col["digits"][:3, ::-1].copy(), col["contigs"][:3], col["positions"][:3]).to_csv(other)
    abund.main([run, freq, "-o", str(tmp_path / "o2"), "--tau", str(other)])
    assert np.array_equal(fake_fit[-1]["tau"], col["digits"][:3, ::-1])
    os.remove(os.path.join(run, "Collated_Tau_star.csv"))
    abund.main([run, freq, "-o", str(tmp_path / "o3")])
    assert np.array_equal(fake_fit[-1]["tau"], model["digits"])
    os.remove(os.path.join(run, "Filtered_Tau_star.csv"))
    with pytest.raises(SystemExit) as e:
        abund.main([run, freq])
    assert "Filtered_Tau_star.csv" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        abund.main([run, freq, "--tau", str(tmp_path / "nothing.csv")])
    assert "nothing.csv" in str(e.value.code)


def test_cli_output_files_byte_layout(tmp_path, fake_fit):
    from desman_amd import abund
    run, model = _run_dir(tmp_path)
    freq, df = _freq(tmp_path, ["N1", "N2"], model["contigs"], model["positions"])
    out = tmp_path / "out"
    abund.main([run, freq, "-o", str(out), "--presence"])
    # Projected_Gamma.csv: the text Output_Results writes for Gamma_star.csv (DataFrame(gamma, index = sample names).to_csv)
    assert open(out / "Projected_Gamma.csv").read() == ",0,1\nN1,0.5,0.5\nN2,0.5,0.5\n"
    raw = df.to_numpy()[:, 1:].reshape(len(df), 2, 4)
    reads = raw.sum(axis=(0, 2))
    lines = open(out / "Projected_fit.csv").read().split("\n")
    assert lines[0] == ",reads,mean_depth,loglik,deviance,deviance_per_read,iters,converged" and lines[3] == ""
    assert lines[1] == "N1,%d,%s,-1.0,0.0,0.0,7,1" % (reads[0], repr(float(reads[0] / 6.0)))
    assert lines[2] == "N2,%d,%s,-2.0,0.5,%s,8,1" % (reads[1], repr(float(reads[1] / 6.0)), repr(float(0.5 / reads[1])))
    assert open(out / "Projected_presence.csv").read() == ",0,1\nN1,0.0,1.0\nN2,2.0,3.0\n"
    out2 = tmp_path / "out2"
    abund.main([run, freq, "-o", str(out2)])
    assert not os.path.exists(out2 / "Projected_presence.csv") and os.path.exists(out2 / "Projected_fit.csv")
