"""Position-marginal predictive density from the resident traces (dsm_ctx_trace_predictive; kernels_pred.hip) on the GPU, against the
numpy restatement tests/_predictive_ref.py, and `desman --predictive` end to end.  Tolerance: that of tests/test_gpu_assign.py for logz --
1e-12 relative with delta = 1e-12 max|L| as absolute floor -- carried through to lppd and mean (both are contractions of the logz
column: the largest tolerance of the column); var to 1e-9 relative plus delta^2.  Worst fraction of that tolerance seen on an MI355X
over this file: 0.00049; the bits of logz equal Context.assign_tau's at G = 10.  The host side alone is tests/test_predictive_cpu.py.
Run on an MI355X with:  python -m pytest tests/test_gpu_predictive.py -m gpu
"""
import math
import os

import numpy as np
import pandas as pd
import pytest
from numpy.random import RandomState

import _predictive_ref as ref
from desman_amd import _lib, predictive
from desman_amd.synth import synth_counts, random_state

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = r"error -2: ", r"error -3: ", r"error -4: "
KEYS = ("lppd", "mean", "var", "logz_it")
WORST = [0.0]


@pytest.fixture()
def ctx():
    c = _lib.Context(0)
    yield c
    _lib.pred_debug_set_chunk(0)
    _lib.pred_debug_set_parts(0)
    c.close()


def _close(got, want, what):
    """every output within its tolerance; -inf / +inf exactly where the reference has them, NaN nowhere"""
    lz, labs = want["logz_it"], want["labs"]
    delta = 1e-12 * np.maximum(labs, 1.0)
    with np.errstate(invalid="ignore"):
        tol_tv = np.maximum(1e-12 * np.abs(np.where(np.isfinite(lz), lz, 0.0)), delta)
    tol_v, d2 = tol_tv.max(axis=0), delta.max(axis=0) ** 2
    assert got["n_used"] == want["n_used"], what
    for k in KEYS:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == np.float64 and not np.isnan(g).any() and not np.isnan(w).any(), (what, k)
        assert np.array_equal(g[~np.isfinite(w)], w[~np.isfinite(w)]) and np.array_equal(np.isfinite(g), np.isfinite(w)), (what, k)
        fin = np.isfinite(w)
        tol = tol_tv if k == "logz_it" else (1e-9 * np.abs(w) + d2 if k == "var" else tol_v)
        err = np.abs(g[fin] - w[fin])
        frac = float((err / tol[fin]).max()) if err.size else 0.0
        WORST[0] = max(WORST[0], frac)
        assert frac <= 1.0, (what, k, frac)
    print("%s: worst fraction of the tolerance so far %.3g" % (what, WORST[0]))


def _same_bits(a, b, what):
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _plant(c, V, S, G, n, seed=0, depth=30):
    rs = RandomState(8000 + 31 * V + 7 * S + G + seed)
    counts = rs.randint(0, depth, size=(V, S, 4)).astype(np.int64)
    counts[rs.random_sample((V, S, 4)) < 0.3] = 0
    counts[rs.random_sample((V, S)) < 0.05] = 0
    c.set_counts(counts)
    tau, gamma0, eta0 = random_state(V, S, G, seed=5 + seed)
    c.set_state(tau, gamma0, eta0)
    gamma = rs.dirichlet(np.ones(G), size=(n, S))
    eta = 0.9 * np.eye(4) + 0.1 * rs.dirichlet(np.ones(4), size=(n, 4))
    c.debug_set_trace(rs.randint(0, 4, size=(n, V, G)))
    c.debug_set_param_trace(gamma, eta)
    return counts, gamma, eta


# ---- 1. planted traces against the reference: every path of the kernel, strides, offsets, chunkings, parts ----------------------------------
#          V   S   G  n
SHAPES = [(3, 1, 1, 1), (5, 3, 2, 3), (4, 5, 3, 4), (6, 7, 4, 5), (3, 4, 6, 3), (2, 3, 7, 2), (3, 65, 3, 2), (2, 130, 4, 2)]


@pytest.mark.parametrize("V,S,G,n", SHAPES, ids=["V%d_S%d_G%d_n%d" % s for s in SHAPES])
def test_shapes_against_numpy(ctx, V, S, G, n):
    counts, gamma, eta = _plant(ctx, V, S, G, n)
    it0 = min(1, n - 1)
    for kw in (dict(stride=1), dict(stride=2), dict(it0=it0, n_it=n - it0, stride=1)):
        want = ref.trace_predictive(counts, gamma, eta, **kw)
        _lib.pred_debug_set_chunk(0); _lib.pred_debug_set_parts(0)
        got = ctx.trace_predictive(want=KEYS, **kw)
        _close(got, want, (V, S, G, n, kw))
        if want["n_used"] == 1:
            assert not got["var"].any()
        for chunk, parts in ((1, 1), (1, 2), (1, n), (0, 2), (2, n)):
            _lib.pred_debug_set_chunk(chunk); _lib.pred_debug_set_parts(parts)
            _same_bits(ctx.trace_predictive(want=KEYS, **kw), got, (kw, chunk, parts))


def test_G10_against_assign_tau(ctx):
    """Both calls run the same arithmetic in the same order; whether the bits agree is printed (recorded in DESIGN.md sec. 8h)."""
    counts, gamma, eta = _plant(ctx, 2, 4, 10, 2, depth=8)
    got = ctx.trace_predictive(want=KEYS)
    per_it = np.stack([ctx.assign_tau(gamma[t], eta[t])["logz"] for t in range(2)])
    assert np.isfinite(per_it).all()
    tol = 1e-12 * np.maximum(np.abs(per_it), 1.0)      # |logz| itself as the scale: no larger than max|L|, so no looser than the issue's
    err = np.abs(got["logz_it"] - per_it)
    print("G = 10: logz bits equal to assign_tau's: %s; worst error / tolerance %.3g"
          % (got["logz_it"].tobytes() == per_it.tobytes(), float((err / tol).max())))
    assert (err <= tol).all()
    lppd, mean, var = ref.stats(per_it)
    assert (np.abs(got["lppd"] - lppd) <= tol.max(axis=0)).all() and (np.abs(got["mean"] - mean) <= tol.max(axis=0)).all()
    assert (np.abs(got["var"] - var) <= 1e-9 * var + tol.max(axis=0) ** 2).all()


def test_external_counts(ctx):
    V, S, G, n = 9, 5, 4, 3
    counts, gamma, eta = _plant(ctx, V, S, G, n)
    res = ctx.trace_predictive(want=KEYS)
    _same_bits(ctx.trace_predictive(counts=counts.copy(), want=KEYS), res, "a copy of the resident table")
    other = RandomState(3).randint(0, 12, size=(V + 4, S, 4)).astype(np.int64)
    other[2] = 0
    for chunk in (0, 3):
        _lib.pred_debug_set_chunk(chunk)
        _close(ctx.trace_predictive(counts=other, stride=2, want=KEYS), ref.trace_predictive(other, gamma, eta, stride=2), ("other", chunk))
    assert ctx.trace_predictive(counts=other[:0])["lppd"].shape == (0,)
    with pytest.raises(ValueError):
        ctx.trace_predictive(counts=other[:, :2])
    _same_bits(ctx.trace_predictive(want=KEYS), res, "the resident table afterwards")


def test_degenerate_operands(ctx):
    V, S, G, n = 4, 2, 2, 3
    counts = np.zeros((V, S, 4), dtype=np.int64)
    counts[0, 0] = [1, 1, 0, 0]          # A and C in a sample that is haplotype 0 alone: impossible under the identity eta
    counts[1, 1] = [3, 0, 0, 2]
    counts[3] = [[2, 0, 1, 0], [0, 4, 0, 1]]
    ctx.set_counts(counts)
    tau, g0, e0 = random_state(V, S, G, seed=1)
    ctx.set_state(tau, g0, e0)
    ctx.debug_set_trace(np.zeros((n, V, G), dtype=np.int64))
    soft = 0.94 * np.eye(4) + 0.02
    gamma = np.stack([np.array([[1.0, 0.0], [0.5, 0.5]])] * n)
    eta = np.stack([soft, np.eye(4), soft])           # iteration 1 contradicts position 0 (and position 3: C and T next to A, G)
    ctx.debug_set_param_trace(gamma, eta)
    got, want = ctx.trace_predictive(want=KEYS), ref.trace_predictive(counts, gamma, eta)
    _close(got, want, "one iteration contradicts")
    assert got["logz_it"][1, 0] == -np.inf and np.isfinite(got["logz_it"][[0, 2], 0]).all()
    assert np.isfinite(got["lppd"][0]) and got["var"][0] == np.inf and got["mean"][0] == -np.inf
    assert (got["logz_it"][:, 2] == pytest.approx(G * math.log(4.0), rel=1e-15)) and got["var"][2] == 0.0      # the position without reads
    eta = np.stack([np.eye(4)] * n)                    # every iteration contradicts it
    ctx.debug_set_param_trace(gamma, eta)
    got = ctx.trace_predictive(want=KEYS)
    _close(got, ref.trace_predictive(counts, gamma, eta), "every iteration contradicts")
    assert got["lppd"][0] == -np.inf and got["mean"][0] == -np.inf and got["var"][0] == np.inf
    assert np.isfinite(got["lppd"][1]) and not any(np.isnan(got[k]).any() for k in KEYS)
    pw = predictive.pointwise(got, counts, G)
    assert pw["elpd_waic"][0] == -np.inf and not any(np.isnan(pw[k]).any() for k in ("lppd", "p_waic", "elpd_waic"))


def test_error_codes_and_edge_calls(ctx):
    V, S, G, n = 7, 3, 3, 4
    rs = RandomState(9)
    counts = rs.randint(0, 30, size=(V, S, 4)).astype(np.int64)
    with pytest.raises(_lib.DesmanHipError, match=ERR_STATE):
        ctx.trace_predictive(n_it=0)                      # no table
    ctx.set_counts(counts)
    tau, g0, e0 = random_state(V, S, G, seed=3)
    ctx.set_state(tau, g0, e0)
    for call in (lambda: ctx.trace_predictive(n_it=0), lambda: ctx.trace_predictive(n_it=2)):
        with pytest.raises(_lib.DesmanHipError, match=ERR_STATE + ".*no update has run"):
            call()
    counts, gamma, eta = _plant(ctx, V, S, G, n)
    full = ctx.trace_predictive(want=KEYS)
    assert set(ctx.trace_predictive()) == {"lppd", "mean", "var", "n_used"}
    for want in ((), ("lppd",), ("var", "logz_it"), ("mean",)):
        part = ctx.trace_predictive(want=want)
        assert set(part) == set(want) | {"n_used"} and all(part[k].tobytes() == full[k].tobytes() for k in want), want
    assert ctx.lib.dsm_ctx_trace_predictive(ctx._h, None, 0, 0, n, 1, None, None, None, None) == 0
    for it0 in (0, 2, n):                                 # n_it = 0 succeeds and writes nothing
        out = np.full(V, 7.0)
        assert ctx.lib.dsm_ctx_trace_predictive(ctx._h, None, 0, it0, 0, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data, None) == 0
        assert (out == 7.0).all() and ctx.trace_predictive(it0=it0, n_it=0)["n_used"] == 0
    bad = counts.copy()
    bad[3, 1, 2] = -1
    deep = counts.copy()
    deep[0, 0] = [2 ** 30, 2 ** 30, 5, 0]
    cases = [lambda: ctx.trace_predictive(it0=-1, n_it=2), lambda: ctx.trace_predictive(it0=3, n_it=2), lambda: ctx.trace_predictive(it0=n + 1, n_it=0),
             lambda: ctx.trace_predictive(n_it=-1), lambda: ctx.trace_predictive(n_it=n + 1), lambda: ctx.trace_predictive(stride=0),
             lambda: ctx.trace_predictive(stride=-3), lambda: ctx.trace_predictive(counts=bad), lambda: ctx.trace_predictive(counts=deep),
             lambda: _lib.pred_debug_set_chunk(-1), lambda: _lib.pred_debug_set_parts(-1)]
    for k, call in enumerate(cases):
        with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
            call()
        assert ctx.trace_predictive()["lppd"].tobytes() == full["lppd"].tobytes(), k
    with pytest.raises(ValueError):
        ctx.trace_predictive(want=("lppd", "logz"))
    # G = 11: a context whose state, and planted trace, have eleven haplotypes
    big = _lib.Context(0)
    try:
        _plant(big, 2, 2, 11, 2)
        with pytest.raises(_lib.DesmanHipError, match=ERR_UNSUPPORTED + ".*DSM_ASSIGN_MAX_G"):
            big.trace_predictive()
    finally:
        big.close()


def _chain(c, counts, tau, gamma, eta, n):
    c.set_counts(counts); c.set_state(tau, gamma, eta); c.seed(4321, ctr_seed=0xABCDEF12345)
    c.set_tau_rng(_lib.RNG_MT19937)
    c.gibbs_update(n)


def test_real_chain_is_only_read(ctx):
    V, S, G, n = 40, 6, 3, 6
    counts, _, _ = synth_counts(V, S, G, seed=31, depth_scale=0.1)
    tau, gamma, eta = random_state(V, S, G, seed=32)
    twin = _lib.Context(0)
    try:
        _chain(ctx, counts, tau, gamma, eta, n)
        _chain(twin, counts, tau, gamma, eta, n)
        tr = ctx.get_trace()
        got = ctx.trace_predictive(want=KEYS)
        _close(got, ref.trace_predictive(counts, tr["gamma"], tr["eta"]), "real chain")
        _close(ctx.trace_predictive(it0=1, n_it=5, stride=2, want=KEYS), ref.trace_predictive(counts, tr["gamma"], tr["eta"], 1, 5, 2), "strided")
        _same_bits(ctx.trace_predictive(want=KEYS), got, "again")
        assert np.array_equal(ctx.get_mt_state(), twin.get_mt_state()) and ctx.counters() == twin.counters()
        a, b = ctx.get_trace(), twin.get_trace()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        sa, sb = ctx.get_star(), twin.get_star()
        assert sa["lp"] == sb["lp"] and sa["it"] == sb["it"] and np.array_equal(sa["tau"], sb["tau"])
        ctx.gibbs_update(4); twin.gibbs_update(4)
        a, b = ctx.get_trace(), twin.get_trace()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        for x, y in zip(ctx.get_state(), twin.get_state()):       # tau, gamma, eta
            assert x.tobytes() == y.tobytes()
        assert np.array_equal(ctx.get_mt_state(), twin.get_mt_state())
    finally:
        twin.close()


def test_fixed_tau_trace(ctx):
    V, S, G, n = 30, 5, 4, 5
    counts, _, _ = synth_counts(V, S, G, seed=41, depth_scale=0.1)
    tau, gamma, eta = random_state(V, S, G, seed=42)
    ctx.set_counts(counts); ctx.set_state(tau, gamma, eta); ctx.seed(5, ctr_seed=99)
    ctx.gibbs_update_fixed_tau(n, pool=0)
    tr = ctx.get_trace()
    for parts, kw in ((0, dict()), (2, dict(stride=2)), (3, dict(it0=2, n_it=3))):
        _lib.pred_debug_set_parts(parts)
        _close(ctx.trace_predictive(want=KEYS, **kw), ref.trace_predictive(counts, tr["gamma"], tr["eta"], **kw), (parts, kw))


# ---- 2. command line -----------------------------------------------------------------------------------------------------------------------
TABLE = dict(V=200, S=12, G=3, seed=2024, depth_scale=0.15)      # three haplotypes, 6 - 75 reads per sample and position
RUN = ["-r", "120", "-i", "30", "-s", "11", "-m", "0"]


def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def _table():
    counts, tau, gamma = synth_counts(TABLE["V"], TABLE["S"], TABLE["G"], seed=TABLE["seed"], depth_scale=TABLE["depth_scale"])
    return counts, tau, gamma, 0.96 * np.eye(4) + 0.01


def _collapses(gamma):
    """the three two-haplotype collapses of a three-haplotype gamma: haplotypes g and h merged into one"""
    return [np.stack([gamma[:, g] + gamma[:, h], gamma[:, 3 - g - h]], axis=1) for g, h in ((0, 1), (0, 2), (1, 2))]


def precondition(heldout):
    """The held-out positions scored by the reference under the generating (gamma, eta) with three haplotypes and under its best
    two-haplotype collapse: (total difference, its paired standard error).  The model comparison below can only be asked of the
    chains if the table itself tells the two apart."""
    _, _, gamma, eta = _table()
    const = predictive.log_multinomial(heldout)
    three = ref.logz_one(heldout, gamma, eta)[0] + const - 3 * math.log(4.0)
    twos = [ref.logz_one(heldout, g2, eta)[0] + const - 2 * math.log(4.0) for g2 in _collapses(gamma)]
    best = max(twos, key=lambda x: x.sum())
    d = three - best
    return float(d.sum()), float(math.sqrt(d.size * d.var(ddof=1)))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from desman_amd import cli
    root = tmp_path_factory.mktemp("predictive")
    counts, _, _, _ = _table()
    V, S = counts.shape[:2]
    freq = str(root / "t.freq")
    names = ["S%02d" % s for s in range(S)]
    contigs, positions = ["contig%d" % (v // 70) for v in range(V)], np.arange(V) * 7 + 3
    _write_freq(freq, counts, names, contigs, positions)
    dirs = {k: str(root / k) for k in ("plain3", "pred3", "pred2")}
    cli.main([freq, "-g", "3", "-o", dirs["plain3"]] + RUN)
    cli.main([freq, "-g", "3", "-o", dirs["pred3"], "--predictive"] + RUN)
    cli.main([freq, "-g", "2", "-o", dirs["pred2"], "--predictive", "15"] + RUN)
    return dict(dirs=dirs, counts=counts, contigs=contigs, positions=positions)


def test_desman_predictive_end_to_end(runs):
    plain, pred = runs["dirs"]["plain3"], runs["dirs"]["pred3"]
    new = [predictive.POSITIONS_FILE, predictive.SUMMARY_FILE]
    assert sorted(os.listdir(pred)) == sorted(os.listdir(plain) + new)
    read = lambda d, name: open(os.path.join(d, name), "rb").read()
    for name in os.listdir(plain):                             # the usual files do not change
        if name != "log_file.txt":
            assert read(plain, name) == read(pred, name), name
    pp = pd.read_csv(os.path.join(pred, predictive.POSITIONS_FILE), float_precision="round_trip")
    assert list(pp.columns) == ["Contig", "Position", "kind", "lppd", "p_waic", "elpd_waic"]
    fit, held = pp[pp["kind"] == "fit"], pp[pp["kind"] == "heldout"]
    assert len(fit) == 120 and len(held) == 80 and len(pp) == 200
    tm = pd.read_csv(os.path.join(pred, "Tau_Mean.csv"))
    assert list(fit["Contig"]) == list(tm.iloc[:, 0]) and np.array_equal(fit["Position"], tm["Position"])
    fitted = set(zip(fit["Contig"], fit["Position"]))
    rest = [(c, p) for c, p in zip(runs["contigs"], runs["positions"]) if (c, p) not in fitted]
    assert list(zip(held["Contig"], held["Position"])) == rest          # exactly the unselected positions, in input order
    assert held["p_waic"].isna().all() and np.array_equal(held["elpd_waic"], held["lppd"])
    assert np.isfinite(fit[["lppd", "p_waic", "elpd_waic"]].to_numpy()).all() and (fit["p_waic"] >= 0).all()
    assert np.array_equal(fit["elpd_waic"], fit["lppd"] - fit["p_waic"])
    # the summary recomputed from the positions file
    ps = pd.read_csv(os.path.join(pred, predictive.SUMMARY_FILE), float_precision="round_trip")
    assert list(ps.columns) == ["kind", "n_positions", "n_iterations", "elpd", "se", "p_waic", "n_high_var"] and list(ps["kind"]) == ["fit", "heldout"]
    for kind, part in (("fit", fit), ("heldout", held)):
        pw = dict(lppd=part["lppd"].to_numpy(), p_waic=part["p_waic"].to_numpy(), elpd_waic=part["elpd_waic"].to_numpy(), n_iterations=30)
        if kind == "heldout":
            pw["p_waic"] = np.zeros(len(part))
        want = predictive.summary_row(kind, predictive.summary(pw))
        row = ps[ps["kind"] == kind].iloc[0]
        assert row["n_positions"] == want["n_positions"] and row["n_iterations"] == 30 and row["elpd"] == want["elpd"] and row["se"] == want["se"]
        if kind == "fit":
            assert row["p_waic"] == want["p_waic"] and row["n_high_var"] == want["n_high_var"]
        else:
            assert pd.isna(row["p_waic"]) and pd.isna(row["n_high_var"])
    # `--predictive 15` of 30 stored iterations: every second one
    p2 = pd.read_csv(os.path.join(runs["dirs"]["pred2"], predictive.SUMMARY_FILE))
    assert list(p2["n_iterations"]) == [15, 15] and list(p2["n_positions"]) == [120, 80]


def test_model_comparison_ranks_the_generating_G_first(runs):
    pp = pd.read_csv(os.path.join(runs["dirs"]["pred3"], predictive.POSITIONS_FILE))
    held = pp[pp["kind"] == "heldout"]
    row_of = {(c, p): v for v, (c, p) in enumerate(zip(runs["contigs"], runs["positions"]))}
    heldout = runs["counts"][[row_of[k] for k in zip(held["Contig"], held["Position"])]]
    diff, se = precondition(heldout)
    print("precondition: three haplotypes against the best collapse on the held-out positions: %.1f, %.1f paired standard errors" % (diff, diff / se))
    assert diff >= 5.0 * se
    rows = predictive.compare([runs["dirs"]["pred2"], runs["dirs"]["pred3"]])
    print("chains: %r" % (rows,))
    assert [r["G"] for r in rows] == [3, 2] and all(r["kind"] == "heldout" and r["n_positions"] == 80 for r in rows)
    assert rows[1]["elpd_diff"] < -2.0 * rows[1]["se_diff"] and np.isfinite(rows[1]["se_diff"])
