"""dsm_fit_gamma_eta on the MI355X: the error matrix of new samples fitted with their abundances, against the
numpy restatement of tests/_abund_eta_ref.py (checked on its own in tests/test_abund_eta_cpu.py)."""
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _abund_ref as R  # noqa: E402
import _abund_eta_ref as E  # noqa: E402

from desman_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_G = 1e-12                  # gamma and eta, absolute: the fit's own (tests/test_gpu_abund.py)
TOL_L = 1e-12                  # loglik, loglik0, deviance, lr_eta: relative to max(|L|, 1)
N50 = dict(max_iter=50, tol=0.0)
ETA_GEN = E.random_eta(3)
START = E.diag_eta(0.99)
KEYS = ("gamma", "eta", "loglik", "loglik0", "deviance")
SCALARS = ("iters", "converged", "dead_rows", "lr_eta")


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in KEYS) \
        and all(np.array_equal(np.array([a[k]], dtype=np.float64).view(np.uint8), np.array([b[k]], dtype=np.float64).view(np.uint8)) for k in SCALARS)


def _compare(got, ref, what):
    """the call against the restatement; prints and returns the distances (gamma, eta absolute; loglik, loglik0, deviance per sample in
    units of max(|L_s|, 1); lr_eta in units of max(|sum L|, 1)) before it asserts"""
    assert got["iters"] == ref["iters"] and got["converged"] == ref["converged"] and got["dead_rows"] == ref["dead_rows"], \
        (what, got["iters"], got["converged"], got["dead_rows"], ref["iters"], ref["converged"], ref["dead_rows"])
    if np.isneginf(ref["loglik"]).any():                                  # the dead call
        assert not got["gamma"].any() and np.isneginf(got["loglik"]).all() and np.isposinf(got["deviance"]).all(), what
        assert np.array_equal(got["eta"], ref["eta"]) and np.isnan(got["lr_eta"]), what
        return None
    scale = np.maximum(np.abs(ref["loglik"]), 1.0)
    fin = np.isfinite(ref["loglik0"])
    assert np.array_equal(np.isfinite(got["loglik0"]), fin), what
    d = [np.abs(got["gamma"] - ref["gamma"]).max(), np.abs(got["eta"] - ref["eta"]).max(),
         (np.abs(got["loglik"] - ref["loglik"]) / scale).max(),
         (np.abs(got["loglik0"][fin] - ref["loglik0"][fin]) / scale[fin]).max() if fin.any() else 0.0,
         (np.abs(got["deviance"] - ref["deviance"]) / scale).max(),
         abs(got["lr_eta"] - ref["lr_eta"]) / max(abs(ref["loglik"].sum()), 1.0)]
    print("%s: gamma %.2e, eta %.2e, loglik %.2e, loglik0 %.2e, deviance %.2e, lr_eta %.2e (the last four / max(|L|, 1))" % ((what,) + tuple(d)))
    assert d[0] <= TOL_G and d[1] <= TOL_G and max(d[2:]) <= TOL_L, (what, d)
    return d


# ---- 1. equality with the restatement ------------------------------------------------------------------------------------------
# V: one lane, a lane wrap, the tile edge (2048) and more tiles than wavefronts; G: every padding class and its first member; S.
# (V, G, S, fraction of cells zeroed)
CASES = [(1, 3, 1, 0.0), (1, 1, 2, 0.0), (63, 4, 2, 0.0), (63, 32, 2, 0.05), (63, 3, 7, 0.0), (64, 5, 7, 0.0), (64, 17, 2, 0.0),
         (64, 1, 7, 0.05), (65, 8, 1, 0.0), (65, 9, 2, 0.05), (65, 16, 7, 0.0), (257, 9, 7, 0.0), (2048, 16, 1, 0.0),
         (2048, 3, 2, 0.05), (2049, 17, 1, 0.0), (2049, 4, 7, 0.05), (2049, 8, 2, 0.0), (4097, 5, 2, 0.0), (4097, 32, 1, 0.05),
         (4097, 9, 1, 0.0)]


@pytest.mark.parametrize("V,G,S,zf", CASES, ids=["V%d-G%d-S%d%s" % (v, g, s, "-sparse" if z else "") for v, g, s, z in CASES])
def test_fifty_steps_equal_the_restatement(V, G, S, zf):
    """tol = 0, max_iter = 50, depth 20: gamma and eta within 1e-12, loglik, loglik0, deviance and lr_eta within 1e-12 max(|L|, 1)"""
    counts, tau, _ = E.synth(V, S, G, ETA_GEN, depth=20, seed=300 + V + G + S, zero_frac=zf)
    got = _lib.fit_gamma_eta(counts, tau, START, **N50)
    assert got["gamma"].shape == (S, G) and got["eta"].shape == (4, 4)
    ref = E.fit(counts, tau, START, n_iter=50)
    _compare(got, ref, "V=%d G=%d S=%d" % (V, G, S))
    if np.isfinite(ref["loglik"]).all():
        assert np.allclose(got["eta"].sum(axis=1), 1.0, atol=1e-12)
        assert np.allclose(got["gamma"][counts.sum(axis=(0, 2)) > 0].sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("V,G,S", [(257, 8, 3), (2100, 9, 2)])
def test_loglik0_is_fit_gammas_loglik_bit_for_bit(V, G, S):
    counts, tau, _ = E.synth(V, S, G, ETA_GEN, depth=20, seed=5)
    for kw in (N50, dict(max_iter=300, tol=1e-7)):
        got = _lib.fit_gamma_eta(counts, tau, START, **kw)
        plain = _lib.fit_gamma(counts, tau, START, **kw)
        assert np.array_equal(got["loglik0"].view(np.uint8), plain["loglik"].view(np.uint8))
        assert got["lr_eta"] == max(0.0, 2.0 * (sum(got["loglik"].tolist()) - sum(got["loglik0"].tolist())))       # added in index order


# ---- 2. determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,G", [(257, 8), (2100, 9)])
def test_results_are_bit_equal_across_runs_batches_and_entry_points(V, G):
    S = 5
    counts, tau, _ = E.synth(V, S, G, ETA_GEN, depth=20, seed=31)
    for kw in (dict(max_iter=40, tol=0.0), dict()):                       # tol = 0, and the default stop rule
        base = _lib.fit_gamma_eta(counts, tau, START, **kw)
        assert base["iters"] == 40 or (base["converged"] == 1 and base["iters"] > 40)
        assert _same(base, _lib.fit_gamma_eta(counts, tau, START, **kw))
        try:
            for batch in (1, 3):
                _lib.abund_debug_set_eta_batch(batch)
                assert _same(base, _lib.fit_gamma_eta(counts, tau, START, **kw)), batch
        finally:
            _lib.abund_debug_set_eta_batch(0)
        ctx = _lib.Context(0)
        try:
            ctx.set_counts(counts)
            assert _same(base, ctx.fit_gamma_eta(START, tau=tau, **kw))
            onehot = np.zeros((V, G, 4), dtype=np.int64)
            np.put_along_axis(onehot, tau[..., None], 1, axis=2)
            ctx.set_state(onehot, np.full((S, G), 1.0 / G), START)
            assert _same(base, ctx.fit_gamma_eta(START, **kw))            # the resident tau
            _lib.abund_debug_set_eta_batch(3)
            assert _same(base, ctx.fit_gamma_eta(START, tau=onehot, **kw))          # one-hot input
        finally:
            _lib.abund_debug_set_eta_batch(0)
            ctx.close()


# ---- 3. degenerate operands ----------------------------------------------------------------------------------------------------
def test_a_sample_without_reads_among_others():
    counts, tau, _ = E.synth(257, 4, 8, ETA_GEN, depth=20, seed=7, zero_frac=0.3)
    counts[:, 1, :] = 0
    got = _lib.fit_gamma_eta(counts, tau, START, **N50)
    assert np.array_equal(got["gamma"][1], np.full(8, 0.125)) and got["loglik"][1] == 0.0 and got["deviance"][1] == 0.0
    assert got["loglik0"][1] == 0.0
    _compare(got, E.fit(counts, tau, START, n_iter=50), "a sample without reads")
    keep = [0, 2, 3]                                                      # ... it adds nothing to M: the others' fit without it
    alone = _lib.fit_gamma_eta(counts[:, keep], tau, START, **N50)
    assert np.array_equal(alone["eta"], got["eta"]) and np.array_equal(alone["gamma"], got["gamma"][keep])


def test_a_base_no_haplotype_carries_keeps_its_row():
    rs = np.random.RandomState(2)
    V, S, G = 130, 3, 4
    tau = rs.randint(0, 3, size=(V, G))                                   # no haplotype carries base 3
    gamma = rs.dirichlet(np.ones(G) * 3, size=S)
    p = np.einsum("sg,vgb->vsb", gamma, ETA_GEN[tau])
    counts = np.array([[rs.multinomial(25, p[v, s]) for s in range(S)] for v in range(V)], dtype=np.int64)
    eta0 = E.diag_eta(0.97)
    got = _lib.fit_gamma_eta(counts, tau, eta0, **N50)
    assert got["dead_rows"] == 8 and np.array_equal(got["eta"][3], eta0[3]) and np.abs(got["eta"][:3] - eta0[:3]).max() > 1e-3
    _compare(got, E.fit(counts, tau, eta0, n_iter=50), "base 3 absent from tau")


def test_a_haplotype_that_reaches_zero_and_zeros_of_eta0_that_stay():
    """identity eta0, reads only of the bases haplotype 0 carries, haplotype 1 differs from it everywhere: after the first step
    gamma_1 = 0 exactly and stays, the fit goes on with haplotype 0, the zeros of eta0 stay zeros"""
    rs = np.random.RandomState(3)
    V, S = 70, 2
    tau = np.zeros((V, 2), dtype=np.int64)
    tau[:, 0] = rs.randint(0, 4, size=V)
    tau[:, 1] = (tau[:, 0] + 1 + rs.randint(0, 3, size=V)) % 4
    counts = np.zeros((V, S, 4), dtype=np.int64)
    counts[np.arange(V), :, tau[:, 0]] = rs.poisson(20, size=(V, S)) + 1
    got = _lib.fit_gamma_eta(counts, tau, np.eye(4), **N50)
    assert np.abs(got["gamma"][:, 0] - 1.0).max() <= TOL_G and not got["gamma"][:, 1].any() and np.array_equal(got["eta"], np.eye(4))
    assert got["iters"] == 50 and np.abs(got["loglik"]).max() <= TOL_L
    _compare(got, E.fit(counts, tau, np.eye(4), n_iter=50), "a haplotype at 0")
    # zeros the counts do not contradict, off the identity: base a is read as a or as a + 1 only
    eta0 = 0.95 * np.eye(4) + 0.05 * np.roll(np.eye(4), 1, axis=1)
    counts2, tau2, _ = E.synth(257, 3, 5, 0.9 * np.eye(4) + 0.1 * np.roll(np.eye(4), 1, axis=1), depth=20, seed=12)
    got = _lib.fit_gamma_eta(counts2, tau2, eta0, **N50)
    assert np.array_equal(got["eta"] == 0.0, eta0 == 0.0) and np.abs(got["eta"] - eta0).max() > 1e-2
    _compare(got, E.fit(counts2, tau2, eta0, n_iter=50), "zeros of eta0 that stay")


def test_zeros_of_eta0_that_the_counts_contradict_kill_the_call():
    rs = np.random.RandomState(4)
    V, G, S = 70, 3, 3
    tau = rs.randint(0, 4, size=(V, G))
    tau[0] = [0, 1, 2]
    gamma = rs.dirichlet(np.ones(G) * 3, size=S)
    counts = np.zeros((V, S, 4), dtype=np.int64)
    for v in range(V):
        for s in range(S):
            np.add.at(counts[v, s], tau[v], rs.multinomial(30, gamma[s]))
    good = _lib.fit_gamma_eta(counts, tau, np.eye(4), **N50)
    assert good["converged"] == 0 and np.isfinite(good["loglik"]).all() and np.array_equal(good["eta"], np.eye(4))
    counts[0, 1, 3] = 2                                                   # sample 1: two T where the haplotypes carry A, C, G
    got = _lib.fit_gamma_eta(counts, tau, np.eye(4), **N50)
    assert not got["gamma"].any() and np.isneginf(got["loglik"]).all() and np.isposinf(got["deviance"]).all()
    assert got["converged"] == 0 and got["iters"] == 0 and np.array_equal(got["eta"], np.eye(4)) and np.isnan(got["lr_eta"])
    assert np.isneginf(got["loglik0"][1]) and np.array_equal(got["loglik0"][[0, 2]], good["loglik0"][[0, 2]])
    _compare(got, E.fit(counts, tau, np.eye(4), n_iter=50), "contradicted zeros")
    none = _lib.fit_gamma_eta(counts, tau, np.eye(4), max_iter=0, tol=0.0)          # met in the evaluation pass alone
    assert not none["gamma"].any() and np.isneginf(none["loglik"]).all() and none["iters"] == 0


def test_one_haplotype_and_no_step():
    counts, tau, _ = E.synth(65, 3, 1, ETA_GEN, seed=9)
    got = _lib.fit_gamma_eta(counts, tau, START, **N50)
    assert np.abs(got["gamma"] - 1.0).max() <= TOL_G and np.abs(got["eta"] - START).max() > 1e-3
    _compare(got, E.fit(counts, tau, START, n_iter=50), "G = 1")
    counts, tau, _ = E.synth(65, 3, 4, ETA_GEN, seed=10)
    got = _lib.fit_gamma_eta(counts, tau, START, max_iter=0, tol=1e-9)
    assert np.array_equal(got["eta"], START) and np.array_equal(got["gamma"], np.full((3, 4), 0.25))
    assert got["iters"] == 0 and got["converged"] == 0 and got["dead_rows"] == 0 and got["lr_eta"] == 0.0
    _compare(got, E.fit(counts, tau, START, n_iter=0), "max_iter = 0")


# ---- 4. arguments ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_library_usable():
    counts, tau, _ = E.synth(65, 2, 3, ETA_GEN, seed=2)
    good = _lib.fit_gamma_eta(counts, tau, START, **N50)
    lib = _lib.load()

    def raw(e=START, x=counts):
        out, scal, ptrs = _lib._fit_eta_out(2, 3)
        rc = lib.dsm_fit_gamma_eta(0, np.ascontiguousarray(x), 65, 2, 3, np.ascontiguousarray(tau), np.ascontiguousarray(e), 50, 0.0, *ptrs)
        return rc, _lib._fit_eta_result(out, scal)
    loose = START.copy(); loose[1, 1] -= 1e-6
    assert raw(e=loose)[0] == -2 and b"row 1 of eta0" in lib.dsm_last_error()     # DSM_ERR_ARG
    assert raw(e=START * 0.5)[0] == -2
    rc, again = raw()
    assert rc == 0 and _same(good, again)
    try:
        _lib.abund_debug_set_eta_stage_max(65 * 2 * 16 - 1)               # the check itself, with the bound lowered below this table
        assert raw()[0] == -4                                             # DSM_ERR_UNSUPPORTED
        _lib.abund_debug_set_eta_stage_max(65 * 2 * 16)
        rc, again = raw()
        assert rc == 0 and _same(good, again)
    finally:
        _lib.abund_debug_set_eta_stage_max(0)


# ---- 5. the default stop rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,S,G,depth,seed", [(65, 2, 3, 20, 41), (257, 6, 3, 50, 42), (120, 3, 5, 40, 43)])
def test_default_settings_converge_as_the_restatement_does(V, S, G, depth, seed):
    counts, tau, _ = E.synth(V, S, G, ETA_GEN, depth=depth, seed=seed)
    got = _lib.fit_gamma_eta(counts, tau, START)
    ref = E.fit(counts, tau, START, max_iter=_lib.FIT_MAX_ITER, tol=_lib.FIT_TOL)
    print("V=%d S=%d G=%d: %d steps (restatement %d), lr_eta %.3f" % (V, S, G, got["iters"], ref["iters"], got["lr_eta"]))
    assert got["converged"] == 1 and got["iters"] == ref["iters"] and 0 < got["iters"] < _lib.FIT_MAX_ITER
    ll = np.array([_lib.fit_gamma_eta(counts, tau, START, max_iter=n, tol=0.0)["loglik"].sum() for n in range(1, 65)])
    print("V=%d S=%d G=%d: largest decrease of L along max_iter = 1 .. 64: %.2e |L|" % (V, S, G, max(0.0, (-np.diff(ll) / np.abs(ll[:-1])).max())))
    assert (np.diff(ll) >= -TOL_L * np.abs(ll[:-1])).all() and ll[-1] > ll[0]


# ---- 6. classes and command line -------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_end_to_end_on_a_fitted_run(tmp_path):
    """`desman` on a synthetic 240 x 12 table (G = 3), then `desman-abund --fit-eta` for four samples drawn from the run's haplotypes
    under ANOTHER error matrix (8-12 % off-diagonal mass per row against the run's 3 %): Projected_Eta.csv is closer to the generating
    matrix than Eta_star.csv is, in max-norm, and lr_eta > 0; --interval runs with the fitted matrix."""
    from desman_amd import abund, cli
    from desman_amd.synth import synth_counts
    V, S, G = 240, 12, 3
    counts, _, _ = synth_counts(V, S, G, seed=123)
    names = ["S%d" % s for s in range(S)]
    freq = str(tmp_path / "fit.freq")
    _write_freq(freq, counts, names, ["contig%d" % (v // 50) for v in range(V)], np.arange(V) * 7 + 3)
    run = str(tmp_path / "run")
    cli.main([freq, "-g", str(G), "-i", "40", "-o", run, "-s", "7"])
    contigs, positions, digits, eta_star = abund.load_model(run)
    eta_gen = E.random_eta(17, lo=0.08, hi=0.12)
    rs = np.random.RandomState(5)
    gamma = rs.dirichlet(np.full(digits.shape[1], 4.0), size=4)
    p = np.einsum("sg,vgb->vsb", gamma, eta_gen[digits])
    new = np.array([[rs.multinomial(60, p[v, s]) for s in range(4)] for v in range(len(digits))], dtype=np.int64)
    table = str(tmp_path / "new.freq")
    _write_freq(table, new, ["N0", "N1", "N2", "N3"], contigs, positions)
    out = str(tmp_path / "projected")
    res = abund.main([run, table, "-o", out, "--fit-eta", "--interval"])
    rt = dict(index_col=0, float_precision="round_trip")
    eta_hat = pd.read_csv(os.path.join(out, "Projected_Eta.csv"), **rt).to_numpy()
    one = pd.read_csv(os.path.join(out, "Projected_eta_fit.csv"), float_precision="round_trip")
    d_hat, d_star = np.abs(eta_hat - eta_gen).max(), np.abs(eta_star - eta_gen).max()
    print("max |eta - eta_gen|: Projected_Eta %.3e, Eta_star %.3e; lr_eta %.1f, %d steps" % (d_hat, d_star, one["lr_eta"][0], one["iters"][0]))
    assert d_hat < d_star and one["lr_eta"][0] > 0 and one["converged"][0] == 1 and one["dead_rows"][0] == 0
    assert np.allclose(eta_hat.sum(axis=1), 1.0, atol=1e-12)
    proj = pd.read_csv(os.path.join(out, "Projected_Gamma.csv"), **rt)
    assert list(proj.index) == ["N0", "N1", "N2", "N3"] and np.allclose(proj.to_numpy().sum(axis=1), 1.0, atol=1e-9)
    fit = pd.read_csv(os.path.join(out, "Projected_fit.csv"), **rt)
    assert (fit["loglik"] >= fit["loglik_eta0"]).all() and one["loglik"][0] == fit["loglik"].sum()
    iv = pd.read_csv(os.path.join(out, "Projected_interval.csv"), **rt)
    g = proj.to_numpy()
    assert (iv[["%d_lo" % k for k in range(g.shape[1])]].to_numpy() <= g).all() and (g <= iv[["%d_hi" % k for k in range(g.shape[1])]].to_numpy()).all()
    direct = _lib.fit_gamma_eta(new, digits, eta_star)
    assert np.array_equal(direct["eta"], eta_hat) and np.array_equal(direct["gamma"], res["gamma"])
