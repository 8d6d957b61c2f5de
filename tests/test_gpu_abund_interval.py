"""dsm_fit_gamma_interval on the MI355X: profile-likelihood intervals of the projected abundances, against the numpy
restatement of tests/_abund_interval_ref.py (checked on its own in tests/test_abund_interval_cpu.py)."""
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _abund_ref as R  # noqa: E402
import _abund_interval_ref as I  # noqa: E402

from desman_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

Q95 = I.quantile(0.95)
NEAR = 1e-9                    # a trial whose deviance lies within NEAR |L| of q may fall either way: its end is not compared


def _near_threshold(trace, q):
    """the (g, side) searches of a restatement trace with a trial too close to the threshold to call"""
    return {(g, side) for g, side, c, ll, Lhat in trace if np.isfinite(ll) and abs(2.0 * (Lhat - ll) - q) <= NEAR * abs(Lhat)}


def _compare(got, counts, tau, eta, ghat, q, what, **kw):
    """lo and hi within ctol + 1e-12 of the restatement's, flags equal; ends whose search had a trial at the threshold are left out,
    at most 1 % of them.  Returns the restatement's result."""
    S, G = ghat.shape
    ctol = kw.get("ctol", _lib.FIT_CTOL)
    skipped, worst = 0, 0.0
    ref = dict(lo=np.zeros((S, G)), hi=np.zeros((S, G)), flags=np.zeros((S, G), dtype=np.int32))
    for s in range(S):
        trace = []
        ref["lo"][s], ref["hi"][s], ref["flags"][s] = I.interval(counts[:, s], tau, eta, ghat[s], q, trace=trace, **kw)
        near = _near_threshold(trace, q)
        skipped += len(near)
        for g in range(G):
            if not {(g, 0), (g, 1)} & near:
                assert got["flags"][s, g] == ref["flags"][s, g], (what, s, g, got["flags"][s], ref["flags"][s])
            for side, key in ((0, "lo"), (1, "hi")):
                if (g, side) in near:
                    continue
                a, b = got[key][s, g], ref[key][s, g]
                if np.isnan(b):
                    assert np.isnan(a), (what, s, g, key)
                    continue
                worst = max(worst, abs(a - b))
                assert abs(a - b) <= ctol + 1e-12, (what, s, g, key, a, b)
    print("%s: largest |end - restatement| %.3e, %d of %d ends not compared" % (what, worst, skipped, 2 * S * G))
    assert skipped <= 0.01 * 2 * S * G, (what, skipped)
    return ref


# ---- 5. equality with the restatement ------------------------------------------------------------------------------------------
# V: a lane with 0, 1 or 2 rows; one tile, two and three tiles.  G: nothing free, nothing to fit, every register padding, more
# searches than a workgroup has wavefronts (G = 8, 9, 17).  V = 2049 with G = 8: groups along blockIdx.y and the tile barriers together.
# ctol: 1e-4 and 1e-3 keep the trials away from the threshold (no end is left out on these inputs: checked with the restatement) and
# the restatement quick; the default 1e-6 runs in the tests below.
SHAPES = [(1, 3, 3, 1e-4), (63, 5, 3, 1e-4), (65, 2, 3, 1e-4), (65, 1, 3, 1e-4), (65, 8, 1, 1e-4), (65, 9, 1, 1e-3), (65, 17, 1, 1e-3),
          (2048, 3, 1, 1e-3), (2049, 8, 1, 1e-3), (4100, 3, 1, 1e-3)]
PARITY = dict(max_iter=1000, tol=1e-9)


def parity_case(V, G, S, seed_base=300):
    return R.synth(V, S, G, depth=20, seed=seed_base + V + G + S)


@pytest.mark.parametrize("V,G,S,ctol", SHAPES, ids=["V%d-G%d-S%d" % t[:3] for t in SHAPES])
def test_intervals_equal_the_restatement(V, G, S, ctol):
    counts, tau, eta, _ = parity_case(V, G, S)
    ghat = _lib.fit_gamma(counts, tau, eta, **PARITY)["gamma"]
    got = _lib.fit_gamma_interval(counts, tau, eta, ghat, ctol=ctol, **PARITY)
    assert got["lo"].shape == (S, G) and got["hi"].shape == (S, G) and got["flags"].shape == (S, G) and got["flags"].dtype == np.int32
    assert (got["lo"] <= ghat).all() and (ghat <= got["hi"]).all() and (got["lo"] >= 0).all() and (got["hi"] <= 1).all()
    assert np.array_equal(got["flags"] & 1 != 0, got["lo"] == 0.0) and np.array_equal(got["flags"] & 2 != 0, got["hi"] == 1.0)
    _compare(got, counts, tau, eta, ghat, Q95, "V=%d G=%d S=%d" % (V, G, S), ctol=ctol, **PARITY)


# ---- 6. consistency with the presence statistic and with duplicates -----------------------------------------------------------------
def _table(gamma, tau, eta, depth, seed):
    rs = np.random.RandomState(seed)
    p = np.einsum("g,vgb->vb", np.asarray(gamma), eta[tau])
    return np.array([[rs.multinomial(depth, p[v])] for v in range(tau.shape[0])], dtype=np.int64)


def test_lower_end_agrees_with_lr_absent():
    """two absent haplotypes: lo = 0 exactly where lr_absent < q - 1e-6 |L|, lo > 0 where lr_absent > q + 1e-6 |L| (l_g(0) is the
    restricted maximum of the presence fit, reached from another start)"""
    V, G = 257, 5
    _, tau, eta, _ = R.synth(V, 1, G, seed=41)
    counts = _table([0.5, 0.0, 0.3, 0.0, 0.2], tau, eta, 60, 41)
    fit = _lib.fit_gamma(counts, tau, eta, presence=True)
    got = _lib.fit_gamma_interval(counts, tau, eta, fit["gamma"])
    lr, L = fit["lr_absent"][0], abs(fit["loglik"][0])
    print("lr_absent", lr, "lo", got["lo"][0], "hi", got["hi"][0], "flags", got["flags"][0], "gamma", fit["gamma"][0])
    below, above = lr < Q95 - 1e-6 * L, lr > Q95 + 1e-6 * L
    assert below[[1, 3]].all() and above[[0, 2, 4]].all()                 # the table means something
    assert (got["lo"][0][below] == 0.0).all() and (got["flags"][0][below] & 1 == 1).all()
    assert (got["lo"][0][above] > 0.0).all() and (got["flags"][0][above] & 1 == 0).all()


def test_duplicated_haplotypes_share_their_interval():
    """either of a duplicated pair can carry all or none of their joint abundance: lo = 0, hi >= the sum of the two - 2 ctol"""
    V, G = 257, 4
    _, tau, eta, _ = R.synth(V, 1, G, seed=21)
    tau[:, 3] = tau[:, 2]
    counts = _table([0.5, 0.1, 0.25, 0.15], tau, eta, 60, 21)
    fit = _lib.fit_gamma(counts, tau, eta)
    got = _lib.fit_gamma_interval(counts, tau, eta, fit["gamma"])
    pair = fit["gamma"][0][2] + fit["gamma"][0][3]
    print("gamma", fit["gamma"][0], "lo", got["lo"][0], "hi", got["hi"][0])
    for g in (2, 3):
        assert got["lo"][0][g] == 0.0 and got["hi"][0][g] >= pair - 2.0 * _lib.FIT_CTOL
    assert got["lo"][0][0] > 0.3 and got["hi"][0][0] < 0.7


# ---- 7. the held abundance ------------------------------------------------------------------------------------------------------------
def test_two_haplotypes_equal_a_direct_bisection():
    """G = 2: gamma = (c, 1 - c) is the whole model, so the ends are those of a bisection on the one-parameter likelihood written out
    here -- an update that moved the held abundance, or a pass that did not see it, would not reproduce them"""
    V, S, ctol = 130, 3, 1e-6
    counts, tau, eta, _ = R.synth(V, S, 2, depth=20, seed=51)
    ghat = _lib.fit_gamma(counts, tau, eta)["gamma"]
    got = _lib.fit_gamma_interval(counts, tau, eta, ghat, ctol=ctol)
    E = R.emission(tau, eta)
    worst = 0.0
    for s in range(S):
        x = counts[:, s].astype(np.float64)
        pos = x > 0

        def L(c, g):
            p = c * E[:, g] + (1.0 - c) * E[:, 1 - g]
            return float((x[pos] * np.log(p[pos])).sum())
        Lhat = R.loglik(counts[:, s], E, ghat[s])
        for g in range(2):
            for side, key in ((0, "lo"), (1, "hi")):
                b_in, b_out = ghat[s, g], float(side)
                devs = [2.0 * (Lhat - L(b_out, g))]
                if devs[0] <= Q95:
                    want = b_out
                else:
                    while abs(b_out - b_in) > ctol:
                        c = 0.5 * (b_in + b_out)
                        devs.append(2.0 * (Lhat - L(c, g)))
                        if devs[-1] <= Q95:
                            b_in = c
                        else:
                            b_out = c
                    want = b_in
                assert min(abs(d - Q95) for d in devs) > NEAR * abs(Lhat)          # no trial at the threshold on this table
                worst = max(worst, abs(got[key][s, g] - want))
    print("G = 2: largest |end - direct bisection| %.3e" % worst)
    assert worst <= 1e-12
    assert np.abs(got["lo"][:, 0] + got["hi"][:, 1] - 1.0).max() <= 2 * ctol           # the two haplotypes mirror each other


# ---- 8. determinism ------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("lo", "hi", "flags"))


def test_results_are_bit_equal_across_runs_chunks_and_entry_points():
    V, G, S = 2100, 9, 5
    counts, tau, eta, _ = R.synth(V, S, G, depth=20, seed=31)
    kw = dict(max_iter=400, tol=1e-8)
    ghat = _lib.fit_gamma(counts, tau, eta, **kw)["gamma"]
    kw["ctol"] = 1e-4
    base = _lib.fit_gamma_interval(counts, tau, eta, ghat, **kw)
    assert (base["lo"] < ghat).all() and (ghat < base["hi"]).all()
    assert _same(base, _lib.fit_gamma_interval(counts, tau, eta, ghat, **kw))
    try:
        for chunk in (1, 3):
            _lib.abund_debug_set_chunk(chunk)
            assert _same(base, _lib.fit_gamma_interval(counts, tau, eta, ghat, **kw)), chunk
    finally:
        _lib.abund_debug_set_chunk(0)
    ctx = _lib.Context(0)
    try:
        ctx.set_counts(counts)
        assert _same(base, ctx.fit_gamma_interval(eta, ghat, tau=tau, **kw))
        onehot = np.zeros((V, G, 4), dtype=np.int64)
        np.put_along_axis(onehot, tau[..., None], 1, axis=2)
        ctx.set_state(onehot, np.full((S, G), 1.0 / G), eta)
        assert _same(base, ctx.fit_gamma_interval(eta, ghat, **kw))                # the resident tau
        _lib.abund_debug_set_chunk(2)
        assert _same(base, ctx.fit_gamma_interval(eta, ghat, tau=onehot, **kw))    # chunks of the resident tensor
    finally:
        _lib.abund_debug_set_chunk(0)
        ctx.close()


# ---- 9. degenerate operands ------------------------------------------------------------------------------------------------------
def test_a_sample_without_reads_and_max_iter_one():
    counts, tau, eta, _ = R.synth(65, 3, 4, depth=20, seed=61)
    counts[:, 1, :] = 0
    ghat = _lib.fit_gamma(counts, tau, eta)["gamma"]
    got = _lib.fit_gamma_interval(counts, tau, eta, ghat, ctol=1e-4)
    assert np.array_equal(got["lo"][1], np.zeros(4)) and np.array_equal(got["hi"][1], np.ones(4)) and (got["flags"][1] == 3).all()
    assert not got["flags"][[0, 2]].any()
    _compare(got, counts, tau, eta, ghat, Q95, "a sample without reads", ctol=1e-4)
    one = _lib.fit_gamma_interval(counts, tau, eta, ghat, ctol=1e-4, max_iter=1)
    assert (one["flags"][[0, 2]] & 4 == 4).all() and (one["flags"][1] == 3).all()
    _compare(one, counts, tau, eta, ghat, Q95, "max_iter = 1", ctol=1e-4, max_iter=1)
    # one step from a start close to the optimum understates l: the interval is not wider than the converged one
    assert (one["lo"][[0, 2]] >= got["lo"][[0, 2]] - 1e-4).all() and (one["hi"][[0, 2]] <= got["hi"][[0, 2]] + 1e-4).all()


def test_a_dead_sample_next_to_healthy_ones():
    """identity eta: sample 1 has reads no haplotype can emit -- its fitted row is 0, its interval NaN, flags 0; the others are what
    they are without it, and a constrained fit that loses the only haplotype able to emit a read counts as outside"""
    V, G, S = 70, 3, 3
    rs = np.random.RandomState(4)
    tau = rs.randint(0, 4, size=(V, G))
    tau[0] = [0, 1, 2]
    gamma = rs.dirichlet(np.ones(G) * 3, size=S)
    counts = np.zeros((V, S, 4), dtype=np.int64)
    for v in range(V):
        for s in range(S):
            np.add.at(counts[v, s], tau[v], rs.multinomial(30, gamma[s]))
    counts[0, 1, 3] = 2
    eye = np.eye(4)
    kw = dict(max_iter=2000, tol=1e-9, ctol=1e-4)
    ghat = _lib.fit_gamma(counts, tau, eye, max_iter=2000, tol=1e-9)["gamma"]
    assert not ghat[1].any()
    got = _lib.fit_gamma_interval(counts, tau, eye, ghat, **kw)
    assert np.isnan(got["lo"][1]).all() and np.isnan(got["hi"][1]).all() and not got["flags"][1].any()
    keep = [0, 2]
    assert (got["lo"][keep] > 0).all() and (got["hi"][keep] < 1).all()              # position 0: every haplotype is needed
    _compare(got, counts, tau, eye, ghat, Q95, "identity eta", **kw)
    alone = _lib.fit_gamma_interval(counts[:, keep], tau, eye, ghat[keep], **kw)
    assert _same({k: v[keep] for k, v in got.items()}, alone)


def test_bad_arguments_return_err_arg_and_leave_the_library_usable():
    counts, tau, eta, _ = R.synth(65, 2, 3, seed=2)
    ghat = _lib.fit_gamma(counts, tau, eta)["gamma"]
    good = _lib.fit_gamma_interval(counts, tau, eta, ghat, ctol=1e-4)
    lib = _lib.load()
    out = dict(lo=np.zeros((2, 3)), hi=np.zeros((2, 3)), flags=np.zeros((2, 3), dtype=np.int32))
    ptrs = [_lib._ptr(out[k]) for k in ("lo", "hi", "flags")]

    def raw(x=counts, t=tau, e=eta, G=3, gh=ghat, q=Q95, ctol=1e-4, p=ptrs):
        return lib.dsm_fit_gamma_interval(0, np.ascontiguousarray(x), 65, 2, G, np.ascontiguousarray(t), np.ascontiguousarray(e),
                                          np.ascontiguousarray(gh), q, 20000, 1e-9, ctol, *p)
    negative = ghat.copy(); negative[1] = [-0.25, 0.75, 0.5]
    short = ghat.copy(); short[0] *= 0.99
    neg_x = counts.copy(); neg_x[3, 1, 0] = -4
    cases = dict(q0=dict(q=0.0), q_neg=dict(q=-3.0), q_inf=dict(q=np.inf), q_nan=dict(q=np.nan), ctol0=dict(ctol=0.0), ctol1=dict(ctol=1.0),
                 ctol_neg=dict(ctol=-1e-6), negative_row=dict(gh=negative), row_sum=dict(gh=short), counts=dict(x=neg_x),
                 G33=dict(G=33, t=np.zeros((65, 33), dtype=np.int64), gh=np.full((2, 33), 1.0 / 33)), null=dict(p=[None] * 3))
    for name, kw in cases.items():
        assert raw(**kw) == -2, name                                              # DSM_ERR_ARG
        assert lib.dsm_last_error()
        assert raw() == 0, name                                                   # the next valid call succeeds ...
        assert _same(out, good), name                                             # ... with the same bits
    dead = ghat.copy(); dead[1] = 0.0                                             # an all-zero row is the fit's "dead" result, not an error
    assert raw(gh=dead) == 0 and np.isnan(out["lo"][1]).all() and np.array_equal(out["lo"][0], good["lo"][0])


# ---- 10. classes and command line --------------------------------------------------------------------------------------------------
def test_end_to_end_on_a_fitted_run(tmp_path):
    """`desman` on ten samples of the synthetic 240 x 12 table (G = 3) of tests/test_gpu_abund.py, then `desman-abund --interval` for
    all twelve: the file's layout, lo <= Projected_Gamma <= hi, and the other files byte for byte those of a run without the option;
    fitGammaInterval() of a chain on its own counts."""
    from numpy.random import RandomState
    from desman_amd import abund, cli, sampletau
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    from desman_amd.Init_NMFT import Init_NMFT
    from desman_amd.synth import synth_counts
    from test_gpu_abund import _write_freq
    V, S, G = 240, 12, 3
    counts, _, _ = synth_counts(V, S, G, seed=123)
    names = ["S%d" % s for s in range(S)]
    freq = str(tmp_path / "ten.freq")
    _write_freq(freq, counts[:, :10, :], names[:10])
    run = str(tmp_path / "run")
    cli.main([freq, "-g", str(G), "-i", "40", "-o", run, "-s", "7"])
    full = str(tmp_path / "all.freq")
    _write_freq(full, counts, names)
    out, plain = str(tmp_path / "with"), str(tmp_path / "without")
    abund.main([run, full, "-o", out, "--presence", "--interval"])
    abund.main([run, full, "-o", plain, "--presence"])
    assert not os.path.exists(os.path.join(plain, "Projected_interval.csv"))
    for name in ("Projected_Gamma.csv", "Projected_fit.csv", "Projected_presence.csv"):
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(plain, name), "rb").read(), name
    proj = pd.read_csv(os.path.join(out, "Projected_Gamma.csv"), index_col=0, float_precision="round_trip")
    iv = pd.read_csv(os.path.join(out, "Projected_interval.csv"), index_col=0, float_precision="round_trip")
    assert list(iv.index) == names == list(proj.index)
    assert list(iv.columns) == [c + suffix for c in proj.columns for suffix in ("_lo", "_hi", "_flag")]
    for c in proj.columns:
        assert (iv[c + "_lo"] <= proj[c]).all() and (proj[c] <= iv[c + "_hi"]).all()
        assert iv[c + "_flag"].isin(range(8)).all() and (iv[c + "_flag"] & 4 == 0).all()
        assert ((iv[c + "_hi"] - iv[c + "_lo"]) > 0).all()
    width = np.array([(iv[c + "_hi"] - iv[c + "_lo"]).to_numpy() for c in proj.columns])
    print("desman-abund --interval: widths %.4f .. %.4f" % (width.min(), width.max()))
    ninety = str(tmp_path / "ninety")
    abund.main([run, full, "-o", ninety, "--interval", "0.9", "--ctol", "1e-5"])
    iv90 = pd.read_csv(os.path.join(ninety, "Projected_interval.csv"), index_col=0, float_precision="round_trip")
    for c in proj.columns:
        assert (iv90[c + "_lo"] >= iv[c + "_lo"] - 1e-5).all() and (iv90[c + "_hi"] <= iv[c + "_hi"] + 1e-5).all()

    rng = RandomState(7)
    sampletau.initRNG()
    sampletau.setRNG(7)
    try:
        nmft = Init_NMFT(counts, G, rng)
        nmft.factorize()
        chain = HaploSNP_Sampler(counts, G, rng, max_iter=20, ctx=nmft._ctx)
        chain.tau = np.copy(nmft.get_tau(), order='C')
        chain.updateTauIndices()
        chain.gamma = np.copy(nmft.get_gamma(), order='C')
        chain.update()
    finally:
        sampletau.freeRNG()
    res = chain.fitGammaInterval(level=0.9)
    assert res["lo"].shape == (S, chain.G) and (res["lo"] <= res["gamma"]).all() and (res["gamma"] <= res["hi"]).all()
    again = chain.fitGammaInterval(level=0.9, snps=counts)                        # the same samples as a new table
    assert _same(res, again) and np.array_equal(res["gamma"], again["gamma"])
