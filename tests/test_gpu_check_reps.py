"""Posterior predictive p-values from replicate tables on the device (dsm_ctx_trace_ppc) against the numpy restatement
of the definition (tests/_ppc_ref.py), against dsm_ctx_trace_fit_stats -- whose X column is the observed side and whose exact E and W the
replicates must reproduce --, and through `desman --check --check-reps`.

Tolerances: a cell's p, X_obs and, on the read-by-read path, X_rep are the restatement's bits and the sums T run in one stated order, so
1e-12 relative on sums of non-negative terms is generous; the counts ge are compared exactly.  The law tests use the exact moments only:
|z| < 5 on means whose standard error comes from W, and a chi-square band at 1 - 1e-6 on the pooled variance of the sample sums (T_s adds
400 cells: the normal theory behind the band holds; T_v adds 8, so the positions' variances are not pooled)."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.stats as st
from numpy.random import RandomState

import _ppc_ref as ref
from desman_amd import _lib, check
from desman_amd.synth import synth_counts, random_state

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = r"error -2: ", r"error -3: ", r"error -4: "
TOL = 1e-12
KEY = 0xABCDEF0100000077
OUT = ("ge_sample", "ge_position", "rep_sample", "rep_position", "obs_sample", "obs_position")


@pytest.fixture()
def ctx():
    c = _lib.Context(0)
    yield c
    _lib.ppc_debug_set_parts(0)
    _lib.ppc_debug_set_chunk(0, 0)
    _lib.fit_debug_set_parts(0)
    c.close()


def _plant(c, V, S, G, n, seed=0, depth=30, deep=False):
    """counts (an all-zero sample and an all-zero position among them), planted tau, gamma and eta traces of n iterations"""
    rs = RandomState(9100 + 31 * V + 7 * S + G + seed)
    digits = rs.randint(0, 4, size=(n, V, G))
    gamma = rs.dirichlet(np.ones(G), size=(n, S))
    eta = 0.9 * np.eye(4) + 0.1 * rs.dirichlet(np.ones(4), size=(n, 4))
    # the table is a draw from iteration 0's parameters, so that iteration's comparisons go both ways (the others fit badly: ge = 0);
    # reads per cell up to 4 (depth - 1) <= C, or -- deep -- from a handful to about 5000, on both sides of C
    N = rs.randint(0, 4 * (depth - 1) + 1, size=(V, S))
    if deep:
        N = np.exp(rs.uniform(np.log(8.0), np.log(5000.0), size=(V, S))).astype(np.int64)
    p0 = ref.cell_p(digits[0], gamma[0], eta[0])
    counts = np.stack([rs.multinomial(N[v, s], p0[v, s] / p0[v, s].sum()) for v in range(V) for s in range(S)]).reshape(V, S, 4)
    counts = counts.astype(np.int64)
    counts[rs.random_sample((V, S)) < 0.05] = 0
    if S > 1:
        counts[:, 1] = 0
    counts[V // 2] = 0
    c.set_counts(counts)
    tau, gamma0, eta0 = random_state(V, S, G, seed=5 + seed)
    c.set_state(tau, gamma0, eta0)
    c.seed(11, ctr_seed=KEY)
    c.debug_set_trace(digits)
    c.debug_set_param_trace(gamma, eta)
    return counts, digits, gamma, eta


def _same_bits(a, b, what):
    for k in OUT:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def _close(got, want, what):
    for k in OUT:
        g, w = got[k], want[k]
        assert g.shape == w.shape and not np.isnan(g).any(), (what, k)
        if k.startswith("ge_"):
            assert g.dtype == np.int64 and np.array_equal(g, w), (what, k, int((g != w).sum()))
        else:
            assert np.array_equal(np.isinf(g), np.isinf(w)), (what, k)
            fin = np.isfinite(w)
            assert (np.abs(g[fin] - w[fin]) <= TOL * np.abs(w[fin])).all(), (what, k, float(np.abs(g[fin] - w[fin]).max()))


# ---- 1. the observed side is dsm_ctx_trace_fit_stats' X -------------------------------------------------------------------------------------
def test_observed_side_equals_fit_stats_and_infinite_cells(ctx):
    V, S, G, n = 70, 5, 2, 3
    counts, digits, gamma, eta = _plant(ctx, V, S, G, n, deep=True)
    eta[1] = np.eye(4)                                           # iteration 1: p_b = 0 for every base no haplotype carries
    ctx.debug_set_param_trace(gamma, eta)
    for it0, n_it in ((0, n), (1, 1), (2, 1)):
        fit = ctx.trace_fit_stats(it0=it0, n_it=n_it, want=("sample", "position"))
        got = ctx.trace_ppc(3, it0=it0, n_it=n_it)
        for kind in ("sample", "position"):
            x, o = fit[kind][:, 0], got["obs_" + kind]
            assert np.array_equal(np.isinf(x), np.isinf(o)) and not np.isnan(o).any(), (it0, kind)
            fin = np.isfinite(x)
            assert (np.abs(o[fin] - x[fin]) <= TOL * np.abs(x[fin])).all(), (it0, kind)
            assert np.isfinite(got["rep_" + kind]).all(), (it0, kind)          # a base with p = 0 is never drawn
            if n_it == 1:
                assert (got["ge_" + kind][np.isinf(o)] == 0).all(), (it0, kind)
        if it0 == 1:
            assert np.isinf(got["obs_position"]).any() and np.isinf(got["obs_sample"]).any()


# ---- 2. bit parity on the read-by-read path: every instantiation --------------------------------------------------------------------------
#          V    S   G  nsl lpv
SHAPES = [(64, 5, 1, 1, 8), (37, 20, 3, 1, 32), (33, 40, 8, 1, 64), (20, 70, 3, 2, 64), (9, 130, 8, 4, 64), (5, 300, 3, 8, 64),
          (1, 1, 1, 1, 1)]


def test_shapes_cover_every_instantiation():
    assert {s[3] for s in SHAPES} == {1, 2, 4, 8}


@pytest.mark.parametrize("V,S,G,nsl,lpv", SHAPES)
def test_parity_read_by_read(ctx, V, S, G, nsl, lpv):
    n, R = 3, 4
    counts, digits, gamma, eta = _plant(ctx, V, S, G, n)
    path = ctx.ppc_debug_path(n, R)
    assert (path["nsl"], path["lpv"], path["C"]) == (nsl, lpv, ref.READS) and counts.sum(axis=2).max() <= path["C"]
    assert ref.tiling(S) == (lpv, nsl)
    got = ctx.trace_ppc(R)
    assert got["n_used"] == n and (V < 20 or (got["ge_position"] > 0).sum() > 1)                # not only the empty position
    _close(got, ref.ppc(counts, digits, gamma, eta, range(n), R, KEY), (V, S, G))
    if S > 1:
        assert got["obs_sample"][1] == 0 and (got["rep_sample"][1] == 0).all() and got["ge_sample"][1] == n * R     # 0 >= 0
    assert got["obs_position"][V // 2] == 0 and got["ge_position"][V // 2] == n * R


# ---- 3. invariance ------------------------------------------------------------------------------------------------------------------------
def test_invariance_parts_chunks_replicates_stride_salt(ctx):
    V, S, G, n, R = 150, 9, 3, 6, 4
    _plant(ctx, V, S, G, n, deep=True)
    base = ctx.trace_ppc(R)
    for parts in (1, 2, 7):
        _lib.ppc_debug_set_parts(parts)
        assert ctx.ppc_debug_path(n, R)["parts"] == min(parts, ctx.ppc_debug_path(n, R)["ct"])
        _same_bits(ctx.trace_ppc(R), base, ("parts", parts))
    _lib.ppc_debug_set_parts(0)
    for ct, cr in ((1, 0), (2, 0), (4, 0), (0, 1), (0, 3), (5, 2)):
        _lib.ppc_debug_set_chunk(ct, cr)
        path = ctx.ppc_debug_path(n, R)
        assert path["cr"] == (cr or R) and path["ct"] == (1 if 0 < cr < R else (ct or path["ct"]))
        _same_bits(ctx.trace_ppc(R), base, ("chunk", ct, cr))
    _lib.ppc_debug_set_parts(2)
    _lib.ppc_debug_set_chunk(4, 0)
    _same_bits(ctx.trace_ppc(R), base, "parts and chunks")
    _lib.ppc_debug_set_parts(0)
    _lib.ppc_debug_set_chunk(0, 0)
    # replicate r of an iteration is the same draw whatever R is: over one iteration the sums of R = k and R = k - 1 differ by replicate
    # k - 1's T and T^2, and the counts by its comparison
    runs = [ctx.trace_ppc(k, it0=0, n_it=1) for k in range(1, 9)]
    assert 0 < runs[7]["ge_position"].sum() < 8 * V
    for kind in ("sample", "position"):
        prev_rep, prev_ge = np.zeros_like(runs[0]["rep_" + kind]), np.zeros_like(runs[0]["ge_" + kind])
        for k, run in enumerate(runs):
            d, dge = run["rep_" + kind] - prev_rep, run["ge_" + kind] - prev_ge
            assert ((dge == 0) | (dge == 1)).all(), (kind, k)
            assert (np.abs(d[:, 1] - d[:, 0] ** 2) <= 1e-9 * np.maximum(run["rep_" + kind][:, 1], 1.0)).all(), (kind, k)
            if k == 3:                                           # R = 4 against the first four replicates of R = 8
                four = run
            prev_rep, prev_ge = run["rep_" + kind], run["ge_" + kind]
        assert (four["ge_" + kind] <= runs[7]["ge_" + kind]).all() and (four["rep_" + kind] <= runs[7]["rep_" + kind]).all()
    # stride 2 is the matching iterations of stride 1
    strided = ctx.trace_ppc(R, it0=0, n_it=n, stride=2)
    assert strided["n_used"] == 3
    singles = [ctx.trace_ppc(R, it0=t, n_it=1) for t in (0, 2, 4)]
    for k in OUT:
        tot = np.zeros_like(singles[0][k])
        for one in singles:
            tot = tot + one[k]
        assert tot.tobytes() == strided[k].tobytes(), k
    odd = ctx.trace_ppc(R, it0=1, n_it=n - 1, stride=2)
    assert np.array_equal(odd["ge_position"] + strided["ge_position"], base["ge_position"])
    assert np.array_equal(odd["ge_sample"] + strided["ge_sample"], base["ge_sample"])
    # another salt, other draws; the observed side does not move
    salted = ctx.trace_ppc(R, salt=12345)
    assert salted["obs_position"].tobytes() == base["obs_position"].tobytes()
    assert (salted["rep_position"][:, 0] != base["rep_position"][:, 0]).mean() > 0.9       # (the planted trace fits badly: ge is 0 either way)
    assert (salted["rep_sample"][[0] + list(range(2, S)), 0] != base["rep_sample"][[0] + list(range(2, S)), 0]).all()
    _same_bits(ctx.trace_ppc(R, salt=0), base, "salt 0")


# ---- 4. the law of the replicates on both draw paths: the exact E and W of dsm_ctx_trace_fit_stats ----------------------------------------
def test_replicates_reproduce_exact_mean_and_variance(ctx):
    V, S, G, n, R = 400, 8, 3, 2, 200
    counts, _, _, _ = _plant(ctx, V, S, G, n, deep=True)
    N = counts.sum(axis=2)
    assert (N[N > 0] <= ref.READS).mean() > 0.2 and (N > ref.READS).mean() > 0.2 and N.max() > 3000
    fit = ctx.trace_fit_stats(want=("sample", "position"))
    got = ctx.trace_ppc(R)
    for kind in ("sample", "position"):
        E, W = fit[kind][:, 2] / n, fit[kind][:, 3] / n              # per-iteration means of the exact mean and variance of T
        mean = got["rep_" + kind][:, 0] / (n * R)
        live = W > 0
        z = (mean[live] - E[live]) / np.sqrt(W[live] / (n * R))
        print("%s: largest |z| of the replicate mean against E: %.3f" % (kind, np.abs(z).max()))
        assert (np.abs(z) < 5).all(), (kind, float(np.abs(z).max()))
        assert (mean[~live] == 0).all()
    q, dof = 0.0, 0
    for t in range(n):
        one = ctx.trace_ppc(R, it0=t, n_it=1, want=("rep_sample",))["rep_sample"]
        W = ctx.trace_fit_stats(it0=t, n_it=1, want=("sample",))["sample"][:, 3]
        live = W > 0
        q += float(((one[live, 1] - one[live, 0] ** 2 / R) / W[live]).sum())
        dof += int(live.sum()) * (R - 1)
    lo, hi = st.chi2.ppf(5e-7, dof), st.chi2.ppf(1.0 - 5e-7, dof)
    print("pooled variance of T_s^rep over the exact W: %.1f on %d degrees of freedom, band %.1f .. %.1f" % (q, dof, lo, hi))
    assert lo < q < hi


# ---- 5. calibration and power: the cases and seeds of tests/test_check_reps_cpu.py --------------------------------------------------------
@pytest.mark.parametrize("spoiled", [False, True])
def test_calibration_and_power(ctx, spoiled):
    counts, digits, gamma, eta = ref.known_case(spoiled=spoiled)
    ctx.set_counts(counts)
    tau = np.eye(4, dtype=np.int64)[digits[0]]
    ctx.set_state(tau, gamma[0], eta[0])
    ctx.seed(3, ctr_seed=ref.CASE_KEY)
    ctx.debug_set_trace(digits)
    ctx.debug_set_param_trace(gamma, eta)
    got = ctx.trace_ppc(ref.CASE_R)
    p = got["ge_sample"] / float(ref.CASE_R)
    print("sample p-values:", p)
    if spoiled:
        assert p[ref.SPOILED] < 0.01 and (np.delete(p, ref.SPOILED) > 0.05).all(), p
    else:
        pv, share, lo, hi = ref.calibration_figures(got["ge_position"], ref.CASE_R)
        print("ten-bin chi-square p-value %.3g; share below 0.05: %.4f, band %.4f .. %.4f" % (pv, share, lo, hi))
        assert pv > 1e-6 and lo <= share <= hi


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors_and_empty_range(ctx):
    counts, _, _ = synth_counts(30, 4, 2, seed=3)
    tau, gamma, eta = random_state(30, 4, 2, seed=4)
    ctx.set_counts(counts); ctx.set_state(tau, gamma, eta)
    with pytest.raises(_lib.DesmanHipError, match=ERR_STATE):
        ctx.trace_ppc(2)
    ctx.seed(5, ctr_seed=99)
    ctx.gibbs_update(4)
    for kw in (dict(it0=3, n_it=2), dict(it0=-1, n_it=1), dict(stride=0), dict(it0=5, n_it=0)):
        with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
            ctx.trace_ppc(2, **kw)
    with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
        ctx.trace_ppc(0)
    with pytest.raises(_lib.DesmanHipError, match=ERR_UNSUPPORTED):
        ctx.trace_ppc(1025)
    empty = ctx.trace_ppc(2, it0=4, n_it=0)
    assert empty["n_used"] == 0 and all((empty[k] == 0).all() for k in OUT)
    only = ctx.trace_ppc(2, want=("ge_sample",))
    assert set(only) == {"ge_sample", "n_used", "R"} and np.array_equal(only["ge_sample"], ctx.trace_ppc(2)["ge_sample"])


# ---- 7. the chain is only read; a fixed-tau trace -----------------------------------------------------------------------------------------
def _chain(c, counts, tau, gamma, eta, n):
    c.set_counts(counts); c.set_state(tau, gamma, eta); c.seed(4321, ctr_seed=0xABCDEF12345)
    c.set_tau_rng(_lib.RNG_MT19937)
    c.gibbs_update(n)


def test_chain_is_only_read_and_continues_bit_for_bit(ctx):
    V, S, G, n = 130, 6, 3, 12
    counts, _, _ = synth_counts(V, S, G, seed=31)
    tau, gamma, eta = random_state(V, S, G, seed=32)
    twin = _lib.Context(0)
    try:
        _chain(ctx, counts, tau, gamma, eta, n)
        _chain(twin, counts, tau, gamma, eta, n)
        got = ctx.trace_ppc(5, stride=2)
        fit = ctx.trace_fit_stats(want=("sample",))
        assert got["n_used"] == 6 and (got["ge_position"] <= 30).all()
        _same_bits(ctx.trace_ppc(5, stride=2), got, "call to call")
        assert np.all(got["obs_sample"] <= fit["sample"][:, 0])
        assert np.array_equal(ctx.get_mt_state(), twin.get_mt_state()) and ctx.counters() == twin.counters()
        a, b = ctx.get_trace(), twin.get_trace()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        for x, y in zip(ctx.get_state(), twin.get_state()):
            assert x.tobytes() == y.tobytes()
        ctx.gibbs_update(5); twin.gibbs_update(5)
        a, b = ctx.get_trace(), twin.get_trace()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        for t in range(-1, 5):
            assert ctx.get_tau_at(t).tobytes() == twin.get_tau_at(t).tobytes(), t
        for x, y in zip(ctx.get_state(), twin.get_state()):
            assert x.tobytes() == y.tobytes()
        assert np.array_equal(ctx.get_mt_state(), twin.get_mt_state()) and ctx.counters() == twin.counters()
        sa, sb = ctx.get_star(), twin.get_star()
        assert sa["lp"] == sb["lp"] and sa["it"] == sb["it"] and np.array_equal(sa["tau"], sb["tau"])
    finally:
        twin.close()


def test_fixed_tau_trace_uses_the_held_tau(ctx):
    V, S, G, n, R = 60, 5, 3, 4, 3
    counts = RandomState(8).randint(0, 30, size=(V, S, 4)).astype(np.int64)
    tau, gamma, eta = random_state(V, S, G, seed=42)
    ctx.set_counts(counts); ctx.set_state(tau, gamma, eta); ctx.seed(5, ctr_seed=KEY)
    ctx.gibbs_update_fixed_tau(n, pool=0)
    tr = ctx.get_trace()
    _close(ctx.trace_ppc(R), ref.ppc(counts, np.argmax(tau, axis=2), tr["gamma"], tr["eta"], range(n), R, KEY), "fixed tau")


# ---- 8. command line ------------------------------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_desman_check_reps(tmp_path, caplog):
    import logging
    from desman_amd import cli
    caplog.set_level(logging.INFO)
    V, S, G, n = 200, 8, 3, 40
    counts, _, _ = synth_counts(V, S, G, seed=123)
    freq = str(tmp_path / "fit.freq")
    names = ["S%d" % s for s in range(S)]
    contigs, positions = ["contig%d" % (v // 50) for v in range(V)], np.arange(V) * 7 + 3
    _write_freq(freq, counts, names, contigs, positions)
    plain, reps = str(tmp_path / "plain"), str(tmp_path / "reps")
    args = [freq, "-g", str(G), "-i", str(n), "-s", "7", "--check"]
    cli.main(args + ["-o", plain])
    caplog.clear()
    cli.main(args + ["-o", reps, "--check-reps", "5", "--relabel"])
    new = ["Fit_samples_ppp.csv", "Fit_positions_ppp.csv"]
    assert set(os.listdir(reps)) >= set(os.listdir(plain)) | set(new) and not set(new) & set(os.listdir(plain))
    read = lambda d, name: open(os.path.join(d, name), "rb").read()
    for name in ("Fit_samples.csv", "Fit_positions.csv"):
        assert read(plain, name) == read(reps, name), name
    fs = pd.read_csv(os.path.join(reps, new[0]))
    fp = pd.read_csv(os.path.join(reps, new[1]))
    assert list(fs.columns) == ["sample"] + list(check.PPP_COLUMNS) and list(fs["sample"]) == names
    assert list(fp.columns) == ["Contig", "Position"] + list(check.PPP_COLUMNS) + ["q"] and len(fp) == V
    assert list(fp["Contig"]) == contigs and np.array_equal(fp["Position"], positions)
    for frame in (fs, fp):
        assert ((frame["p"] >= 0) & (frame["p"] <= 1)).all() and (frame["T_rep"] >= 0).all() and (frame["T_rep_sd"] >= 0).all()
        k = frame["p"].to_numpy() * (40 * 5)                          # stride 1: 40 iterations x 5 replicates
        assert (np.abs(k - np.round(k)) < 1e-9).all()
    assert ((fp["q"] >= fp["p"]) & (fp["q"] <= 1)).all() and np.allclose(fp["q"], check.bh_qvalues(fp["p"].to_numpy()))
    assert "Fit_samples_ppp.csv / Fit_positions_ppp.csv written" in caplog.text and "p < 0.01" in caplog.text
