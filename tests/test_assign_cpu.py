"""Exact joint haplotype assignment (dsm_assign_tau, desman_amd.assign): what can be checked without a GPU.

The golden fixtures tests/golden/assign_tau_V*_S*_G*.npz come from the reference's own HaploSNP_Sampler.assignTau
(tests/golden/make_golden_assign.py).  ``assign_numpy`` below is a closed-form numpy restatement of the model
(include/desman_hip.h: dsm_assign_tau) -- checked here against the goldens, and the comparator of tests/test_gpu_assign.py on
shapes that have no golden."""
import glob
import os
import re

import numpy as np
import pandas as pd
import pytest

from desman_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "assign_tau_V*_S*_G*.npz")))
HAVE_GPU = _lib.device_count() > 0 if os.path.exists(_lib.LIB_PATH) else False


# ---- numpy restatement -------------------------------------------------------------------------------------------------
def digits_of(idx, G):
    """state index -> [.., G] digits, haplotype 0 the most significant (the order of itertools.product(range(4), repeat=G))"""
    idx = np.asarray(idx, dtype=np.int64)
    return (idx[..., None] >> (2 * (G - 1 - np.arange(G)))) & 3


def loglik_states(counts, gamma, eta, dig):
    """L[N][T] = sum_{s,b: x > 0} x ln sum_g gamma[s][g] eta[a_g][b] for the T states with digits dig [T][G]"""
    N, S, _ = counts.shape
    p = np.einsum("sg,tgb->tsb", gamma, eta[dig])                       # [T][S][4]
    with np.errstate(divide="ignore"):
        lp = np.log(p).reshape(len(dig), S * 4)
    X = counts.reshape(N, S * 4).astype(np.float64)
    dead = np.isinf(lp)
    L = X @ np.where(dead, 0.0, lp).T
    if dead.any():
        L[((X > 0).astype(np.float64) @ dead.T.astype(np.float64)) > 0] = -np.inf      # a read where p = 0
    return L


def loglik_at(counts, gamma, eta, state):
    """L of one given state [N][G] per position"""
    return np.array([loglik_states(counts[n:n + 1], gamma, eta, state[n:n + 1].astype(np.int64))[0, 0] for n in range(len(counts))])


def assign_numpy(counts, gamma, eta, chunk=4096, want_L=False):
    """dict of map_idx, map_state, conf, logz, marg (and L with want_L) by two passes over the 4^G states in chunks"""
    counts = np.asarray(counts, dtype=np.int64)
    gamma, eta = np.asarray(gamma, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    N, G, T = counts.shape[0], gamma.shape[1], 4 ** gamma.shape[1]
    M = np.full(N, -np.inf)
    arg = np.zeros(N, dtype=np.int64)
    Ls = []
    for t0 in range(0, T, chunk):
        dig = digits_of(np.arange(t0, min(T, t0 + chunk)), G)
        L = loglik_states(counts, gamma, eta, dig)
        if want_L:
            Ls.append(L)
        k = np.argmax(L, axis=1)                                        # first maximum of the chunk
        better = L[np.arange(N), k] > M                                 # strict: ties keep the lower index
        arg[better] = t0 + k[better]
        M[better] = L[np.arange(N), k][better]
    Z = np.zeros(N)
    marg = np.zeros((N, G * 4))
    live = np.isfinite(M)
    for t0 in range(0, T, chunk):
        dig = digits_of(np.arange(t0, min(T, t0 + chunk)), G)
        L = loglik_states(counts, gamma, eta, dig)
        with np.errstate(invalid="ignore"):
            w = np.where(live[:, None], np.exp(L - np.where(live, M, 0.0)[:, None]), 0.0)
        Z += w.sum(axis=1)
        onehot = np.zeros((len(dig), G * 4))
        onehot[np.arange(len(dig))[:, None], np.arange(G) * 4 + dig] = 1.0
        marg += w @ onehot
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dict(map_idx=np.where(live, arg, 0), conf=np.where(live, 1.0 / np.where(live, Z, 1.0), 0.0),
                   logz=np.where(live, M + np.log(np.where(live, Z, 1.0)), -np.inf),
                   marg=np.where(live[:, None], marg / np.where(live, Z, 1.0)[:, None], 0.0).reshape(N, G, 4),
                   lmax=M)
    out["map_state"] = digits_of(out["map_idx"], G).astype(np.uint8)
    if want_L:
        out["L"] = np.concatenate(Ls, axis=1)
    return out


def load_fixture(path):
    z = np.load(path)
    return dict(counts=z["counts"], gamma=z["gamma"], eta=z["eta"], G=int(z["G"]), conf=z["conf"], L=z["L"], ref_draw=z["ref_draw"],
                state_digits=z["state_digits"], names=[str(n) for n in z["names"]], positions=z["positions"],
                star_csv=str(z["star_csv"]), conf_csv=str(z["conf_csv"]), n_deep=int(z["n_deep"]))


# ---- the fixtures are worth testing against ------------------------------------------------------------------------------
def test_fixtures_are_shallow_enough_to_show_something():
    """with conf = 1.000 everywhere a comparison of conf / marginals / draws would show nothing"""
    assert len(FIXTURES) >= 3
    fx = [load_fixture(p) for p in FIXTURES]
    assert sum((f["conf"] < 0.99).mean() >= 0.30 for f in fx) >= 2
    gaps = []
    for f in fx:
        srt = np.sort(f["L"], axis=1)
        gaps.append((srt[:, -1] - srt[:, -2]).min())
        assert f["L"].shape == (f["counts"].shape[0], 4 ** f["G"])
        assert np.array_equal(f["state_digits"], digits_of(np.arange(4 ** f["G"]), f["G"]))      # the reference's tauStates order
    assert min(gaps) > 1.0e-6, gaps                                    # the MAP comparison is never decided by rounding
    deep = [f for f in fx if f["n_deep"] > 0]
    assert deep and max(np.abs(f["L"]).max() for f in deep) > 1.0e4    # large |L| is exercised too
    assert any((np.argmax(f["ref_draw"], axis=2) != f["state_digits"][np.argmax(f["L"], axis=1)]).any(axis=1).mean() > 0.1 for f in fx)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_numpy_restatement_reproduces_reference(path):
    f = load_fixture(path)
    got = assign_numpy(f["counts"], f["gamma"], f["eta"], chunk=300, want_L=True)
    scale = np.abs(f["L"]).max(axis=1)
    assert (np.abs(got["L"] - f["L"]) <= 1e-12 * scale[:, None]).all()
    assert np.array_equal(got["map_idx"], np.argmax(f["L"], axis=1))
    np.testing.assert_allclose(got["conf"], f["conf"], rtol=1e-12 * np.maximum(1.0, scale).max())
    np.testing.assert_allclose(got["marg"].sum(axis=2), 1.0, rtol=0, atol=1e-12)
    post = np.exp(f["L"] - got["logz"][:, None])
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-9)
    # exp(L - logz) carries the rounding of L - logz: 2^-53 |L| relative, far inside 2e-12 max(1, max_t |L|)
    want = np.array([[post[n, f["state_digits"][:, 0] == a].sum() for a in range(4)] for n in range(len(post))])
    assert (np.abs(got["marg"][:, 0, :] - want) <= 2e-12 * np.maximum(1.0, scale)[:, None]).all()


def test_numpy_restatement_edge_operands():
    gamma = np.array([[0.5, 0.5], [1.0, 0.0]])
    counts = np.zeros((3, 2, 4), dtype=np.int64)
    counts[1, 0] = [3, 0, 0, 1]                                         # reads of A and T in sample 0: needs {A, T} under the identity
    counts[2, 1] = [1, 1, 0, 0]                                         # sample 1 is haplotype 0 alone: A and C cannot both be it
    got = assign_numpy(counts, gamma, np.eye(4))
    assert got["map_idx"][0] == 0 and got["conf"][0] == 1.0 / 16 and np.allclose(got["marg"][0], 0.25) and got["logz"][0] == np.log(16.0)
    assert got["map_idx"][1] == 3 and got["conf"][1] == 0.5 and np.allclose(got["marg"][1, 0], [0.5, 0, 0, 0.5])     # (A,T) and (T,A)
    assert got["conf"][2] == 0.0 and got["logz"][2] == -np.inf and not got["marg"][2].any() and got["map_idx"][2] == 0


# ---- the interface exists --------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_assign():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_assign_tau", "dsm_ctx_assign_tau"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert int(re.search(r"#define\s+DSM_ASSIGN_MAX_G\s+(\d+)", hdr).group(1)) == _lib.ASSIGN_MAX_G == 10


def test_bad_arguments_are_refused_before_any_device_work():
    """shape and range errors come back as DSM_ERR_* codes with or without a GPU"""
    counts = np.ones((2, 3, 4), dtype=np.int64)
    eta = 0.96 * np.eye(4) + 0.01
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*G=11 exceeds DSM_ASSIGN_MAX_G=10"):
        _lib.assign_tau(counts, np.full((3, 11), 1.0 / 11), eta)
    bad = counts.copy(); bad[1, 2, 3] = -1
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*count -1 at position 1, sample 2"):
        _lib.assign_tau(bad, np.full((3, 2), 0.5), eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*gamma"):
        _lib.assign_tau(counts, np.array([[0.5, 0.5], [np.nan, 1.0], [0.5, 0.5]]), eta)
    with pytest.raises(ValueError):
        _lib.assign_tau(counts, np.full((4, 2), 0.5), eta)             # gamma rows != samples
    with pytest.raises(ValueError):
        _lib.assign_tau(counts[:, :, :3], np.full((3, 2), 0.5), eta)


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU failure mode")
def test_assign_fails_loudly_without_gpu():
    with pytest.raises(_lib.DesmanHipError, match="error -6"):
        _lib.assign_tau(np.ones((2, 3, 4), dtype=np.int64), np.full((3, 2), 0.5), 0.96 * np.eye(4) + 0.01)


# ---- desman_amd.assign: argument handling and file layouts ---------------------------------------------------------------------
def _run_dir(tmp_path, names, G=2, tag="star"):
    d = tmp_path / "run"
    d.mkdir(exist_ok=True)
    rs = np.random.RandomState(5)
    pd.DataFrame(rs.dirichlet(np.ones(G), size=len(names)), index=names).to_csv(d / ("Gamma_%s.csv" % tag))
    pd.DataFrame(0.96 * np.eye(4) + 0.01).to_csv(d / ("Eta_%s.csv" % tag))
    return str(d)


def _freq(tmp_path, names, N=5, fname="new.freq"):
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    rs = np.random.RandomState(6)
    data = np.concatenate([np.arange(N)[:, None] * 3 + 1, rs.poisson(4, size=(N, 4 * len(names)))], axis=1)
    df = pd.DataFrame(data, index=["c%d" % (n // 2) for n in range(N)], columns=cols)
    df.index.name = "Contig"
    path = str(tmp_path / fname)
    df.to_csv(path)
    return path, df


@pytest.fixture
def no_gpu_calls(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "assign_tau", boom)


def test_cli_missing_gamma_file_exits_before_the_gpu(tmp_path, no_gpu_calls):
    from desman_amd import assign
    run = _run_dir(tmp_path, ["S0", "S1"])
    freq, _ = _freq(tmp_path, ["S0", "S1"])
    os.remove(os.path.join(run, "Gamma_star.csv"))
    with pytest.raises(SystemExit) as e:
        assign.main([run, freq])
    assert "Gamma_star.csv" in str(e.value.code)
    with pytest.raises(SystemExit) as e:                                 # --mean reads the other pair
        assign.main([_run_dir(tmp_path, ["S0", "S1"]), freq, "--mean"])
    assert "Gamma_mean.csv" in str(e.value.code)


def test_cli_sample_missing_from_the_new_table_is_named(tmp_path, no_gpu_calls):
    from desman_amd import assign
    run = _run_dir(tmp_path, ["S0", "S1", "S7"])
    freq, _ = _freq(tmp_path, ["S1", "S0", "S3"])
    with pytest.raises(SystemExit) as e:
        assign.main([run, freq])
    assert e.value.code not in (0, None) and "'S7'" in str(e.value.code)


def test_cli_maps_sample_columns_by_name(tmp_path):
    from desman_amd import assign
    freq, df = _freq(tmp_path, ["S2", "S0", "extra", "S1"])
    got = assign.map_samples(pd.read_csv(freq, header=0, index_col=0), ["S0", "S1", "S2"])
    raw = df.to_numpy()[:, 1:].reshape(len(df), 4, 4)
    assert got.dtype == np.int64 and np.array_equal(got, raw[:, [1, 3, 0], :])


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_result_files_have_the_reference_layout(path, tmp_path):
    """the writer, fed the reference's own arrays, produces the text the reference's DataFrame steps (bin/desman:219-240) produce"""
    from desman_amd import assign
    f = load_fixture(path)
    N, G = f["counts"].shape[0], f["G"]
    state = np.argmax(f["ref_draw"], axis=2).astype(np.uint8)
    res = dict(map_state=state, conf=f["conf"], logz=np.arange(N) * -1.5, marg=f["ref_draw"].astype(np.float64) * 0.5 + 0.125)
    assign.write_results(str(tmp_path), f["names"], f["positions"], res)
    assert open(tmp_path / "Assigned_Tau_star.csv").read() == f["star_csv"]
    assert open(tmp_path / "Assigned_Tau_conf.csv").read() == f["conf_csv"]
    mean = pd.read_csv(tmp_path / "Assigned_Tau_mean.csv", index_col=0)
    assert list(mean.columns) == ["Position"] + [str(i) for i in range(4 * G)] and list(mean.index) == f["names"]
    assert np.array_equal(mean.to_numpy()[:, 1:].reshape(N, G, 4), res["marg"])
    assert open(tmp_path / "assign_fit.txt").read() == "Assign,%d,%d,%f\n" % (G, N, res["logz"].sum())
