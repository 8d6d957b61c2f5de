"""Sampled joint haplotype assignment on the device (dsm_assign_tau_sampled / dsm_ctx_assign_tau_sampled, kernels_assign_sampled.hip)
against the numpy restatement of tests/_assign_sampled_ref.py and against the exact call.

Parity tolerances (set by the model, not by what the kernel gives): with delta = 1e-12 max(1, max |L_a|) over the steps of a position --
the project's log-likelihood tolerance applied to every candidate total -- marg and spread are held to 2 delta absolute, map_ll to 1e-12
relative; map_state, draw_state and conf (as a count out of 4 kept) must be equal.  Every parity input is checked on the CPU to have no
decision within 2 delta of a CDF edge (``close`` == 0: a condition of the test, asserted in it)."""
import os

import numpy as np
import pandas as pd
import pytest

from desman_amd import _lib
from _assign_sampled_ref import MISTAKES, assign_sampled_numpy
from _philox import CTR_SEEDS
from test_assign_cpu import loglik_at

pytestmark = pytest.mark.gpu
OUT = ("map_state", "map_ll", "conf", "marg", "spread", "draw_state")


def _case(G, S, N, seed, depth=3.0, conc=0.5):
    """an asymmetric eta (no two candidates tie in the model), Dirichlet abundances, `depth` reads per sample on average"""
    rs = np.random.RandomState(seed)
    gamma = rs.dirichlet(np.full(G, conc), size=S)
    eta = 0.08 * rs.dirichlet(np.ones(4), size=4) + 0.92 * np.eye(4)
    tau = rs.randint(0, 4, size=(N, G))
    p = np.einsum("sg,ngb->nsb", gamma, eta[tau])
    d = rs.poisson(depth, size=(N, S))
    counts = np.array([[rs.multinomial(d[n, s], p[n, s] / p[n, s].sum()) for s in range(S)] for n in range(N)], dtype=np.int64)
    return counts, gamma, eta


def _parity(res, ref, T, what):
    assert ref["close"] == 0, (what, "the input has %d decisions within rounding of an edge: choose another" % ref["close"])
    delta = 1e-12 * ref["lscale"]
    assert np.array_equal(res["map_state"], ref["map_state"]), what
    assert np.array_equal(res["draw_state"], ref["draw_state"]), what
    assert np.array_equal(res["conf"], ref["conf_count"] / (4.0 * T)), what
    e_marg = np.abs(res["marg"] - ref["marg"]).max(axis=(1, 2)) / (2 * delta)
    e_spread = np.abs(res["spread"] - ref["spread"]) / (2 * delta)
    live = np.isfinite(ref["map_ll"])
    assert np.array_equal(np.isfinite(res["map_ll"]), live) and (res["map_ll"][~live] == -np.inf).all(), what
    e_ll = np.abs(res["map_ll"][live] - ref["map_ll"][live]) / (1e-12 * np.abs(ref["map_ll"][live]) + 1e-300)
    worst = [float(e.max()) if e.size else 0.0 for e in (e_marg, e_spread, e_ll)]
    print("%s: error / tolerance: marg %.3g, spread %.3g, map_ll %.3g" % (what, *worst))
    assert max(worst) <= 1.0, (what, worst)
    for k in OUT:
        assert not np.isnan(res[k].astype(np.float64)).any(), (what, k)


# ---- 1. parity with the restatement on every path ------------------------------------------------------------------------------
# (S, G, N, B, T, lanes per chain, slots per lane, gamma in chunks, what the case reaches)
SHAPES = [
    (1, 3, 5, 2, 3, 1, 1, False, "LPV = 1: 16 positions of a workgroup, 5 used"),
    (3, 2, 6, 2, 3, 4, 1, False, "LPV = 4, a padded lane"),
    (16, 4, 9, 2, 3, 16, 1, False, "LPV = 16: 4 positions per workgroup, three workgroups"),
    (17, 5, 6, 2, 3, 32, 1, False, "LPV = 32, 15 padded lanes"),
    (64, 6, 3, 2, 3, 64, 1, False, "LPV = 64: one position per workgroup"),
    (65, 3, 3, 1, 2, 64, 2, False, "NSL = 2"),
    (130, 3, 2, 1, 2, 64, 4, False, "NSL = 4"),
    (300, 4, 2, 1, 2, 64, 8, False, "NSL = 8"),
    (300, 12, 1, 1, 1, 64, 8, True, "gamma staged in two chunks of 8 and 4 haplotypes; N = 1; T = 1"),
    (5, 1, 7, 2, 3, 8, 1, False, "G = 1"),
    (12, 11, 4, 1, 2, 16, 1, False, "G = 11: the first G the exact call refuses"),
    (8, 16, 3, 1, 2, 8, 1, False, "G = 16: half of the state word"),
    (5, 32, 6, 3, 3, 8, 1, False, "G = 32: the whole state word, 4 positions per workgroup by the LDS bound"),
    (6, 3, 70, 1, 2, 8, 1, False, "N = 70 across workgroup edges (8 positions each) and chunk edges (chunks of 32)"),
    (7, 4, 5, 0, 3, 8, 1, False, "B = 0"),
    (7, 4, 5, 2, 1, 8, 1, False, "T = 1"),
]


@pytest.mark.parametrize("S,G,N,B,T,lpv,nsl,chunked,why", SHAPES, ids=["S%d_G%d_N%d_B%d_T%d" % s[:5] for s in SHAPES])
def test_parity_with_the_restatement(S, G, N, B, T, lpv, nsl, chunked, why):
    path = _lib.assign_sampled_debug_path(S, G)
    assert (path["lpv"], path["nsl"], path["gamma_chunk"] < G) == (lpv, nsl, chunked), path
    assert path["inst"] == 2 * (nsl.bit_length() - 1) + int(chunked) and 1 <= path["positions_per_workgroup"] <= 64 // lpv
    counts, gamma, eta = _case(G, S, N, 4000 + 37 * S + G)
    seed = 0x5EEDC0DE00000001
    ref = assign_sampled_numpy(counts, gamma, eta, seed, B, T)
    try:
        if N == 70:
            _lib.assign_sampled_debug_set_chunk(32)
        res = _lib.assign_tau_sampled(counts, gamma, eta, seed=seed, burn=B, kept=T)
    finally:
        _lib.assign_sampled_debug_set_chunk(0)
    _parity(res, ref, T, "S%d G%d N%d" % (S, G, N))
    if G * S >= 12 and N > 2:
        assert (ref["draw_state"] != ref["map_state"]).any() or ref["spread"].max() > 0     # (the chains are not frozen)


# ---- 2. one answer whatever the route ------------------------------------------------------------------------------------------
def _same(a, b):
    return set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_chunks_context_form_and_reruns_agree_bit_for_bit():
    counts, gamma, eta = _case(5, 9, 23, 71)
    base = _lib.assign_tau_sampled(counts, gamma, eta, seed=11, burn=2, kept=5)
    assert _same(base, _lib.assign_tau_sampled(counts, gamma, eta, seed=11, burn=2, kept=5))
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    try:
        assert _same(base, ctx.assign_tau_sampled(gamma, eta, seed=11, burn=2, kept=5))
        for chunk in (1, 7, 23):
            _lib.assign_sampled_debug_set_chunk(chunk)
            assert _same(base, _lib.assign_tau_sampled(counts, gamma, eta, seed=11, burn=2, kept=5)), chunk
            assert _same(base, ctx.assign_tau_sampled(gamma, eta, seed=11, burn=2, kept=5)), chunk
    finally:
        _lib.assign_sampled_debug_set_chunk(0)
        ctx.close()
    other = _lib.assign_tau_sampled(counts, gamma, eta, seed=12, burn=2, kept=5)
    assert not np.array_equal(base["marg"], other["marg"])


@pytest.mark.parametrize("seed", CTR_SEEDS, ids=["%#x" % s for s in CTR_SEEDS])
def test_keying(seed):
    counts, gamma, eta = _case(4, 6, 12, 5)
    B, T = 1, 3
    res = _lib.assign_tau_sampled(counts, gamma, eta, seed=seed, burn=B, kept=T)
    _parity(res, assign_sampled_numpy(counts, gamma, eta, seed, B, T), T, "seed %#x" % seed)
    for mistake in MISTAKES:
        if mistake == "high key word dropped" and seed >> 32 == 0:
            continue
        wrong = assign_sampled_numpy(counts, gamma, eta, seed, B, T, mistake=mistake)
        assert not np.array_equal(wrong["draw_state"], res["draw_state"]) and not np.allclose(wrong["marg"], res["marg"], rtol=0, atol=1e-9), mistake


# ---- 3. degenerate operands ----------------------------------------------------------------------------------------------------
def test_degenerate_operands():
    rs = np.random.RandomState(77)
    G, S, N, B, T = 4, 5, 12, 1, 3
    counts, gamma, eta = _case(G, S, N, 78)
    gamma[2] = [1.0, 0.0, 0.0, 0.0]                                         # exact zeros in gamma
    counts[0] = 0                                                           # a position without reads
    counts[:, 4] = 0                                                        # a sample without reads
    counts[3] = 0; counts[3, 1] = [2 ** 20 - 3, 2, 0, 0]                    # counts near 2^20
    counts[5][counts[5] == 1] = 0                                           # more zero cells
    ref = assign_sampled_numpy(counts, gamma, eta, 9, B, T)
    res = _lib.assign_tau_sampled(counts, gamma, eta, seed=9, burn=B, kept=T)
    _parity(res, ref, T, "edges")
    assert np.array_equal(res["marg"][0], np.full((G, 4), 0.25)) and res["spread"][0] == 0.0 and res["map_ll"][0] == 0.0
    # the identity eta: states inconsistent with an observed base have L = -inf
    g2 = np.array([[0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.2, 0.3, 0.5]])
    c2 = np.zeros((5, 3, 4), dtype=np.int64)
    c2[1, 0] = [3, 0, 0, 1]
    c2[2, 1] = [1, 1, 0, 0]                                                 # A and C in a sample that is haplotype 0 alone: no state has mass
    c2[3, 2] = [4, 0, 2, 9]
    c2[4] = c2[2]; c2[4, 0] = [5, 0, 0, 0]
    ref2 = assign_sampled_numpy(c2, g2, np.eye(4), 3, 2, 4)
    r2 = _lib.assign_tau_sampled(c2, g2, np.eye(4), seed=3, burn=2, kept=4)
    _parity(r2, ref2, 4, "identity eta")
    for n in (2, 4):
        assert r2["map_ll"][n] == -np.inf and r2["conf"][n] == 0 and r2["spread"][n] == 0 and not r2["marg"][n].any()
        assert not r2["map_state"][n].any() and not r2["draw_state"][n].any()
    assert np.isfinite(loglik_at(c2, g2, np.eye(4), r2["map_state"])[[0, 1]]).all()
    # position 3 needs three different bases at once: every state within one site of a corner start has L = -inf, so no chain ever
    # moves and the position comes back as one without mass -- the restatement says the same ("What the chain cannot do")
    assert r2["map_ll"][3] == -np.inf and ref2["map_ll"][3] == -np.inf


def test_every_null_combination_of_the_optional_outputs():
    counts, gamma, eta = _case(3, 4, 9, 12)
    full = _lib.assign_tau_sampled(counts, gamma, eta, seed=4, burn=1, kept=2)
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    try:
        for mask in range(16):
            want = [k for i, k in enumerate(_lib.SAMPLED_OPTIONAL) if mask >> i & 1]
            for got in (_lib.assign_tau_sampled(counts, gamma, eta, seed=4, burn=1, kept=2, want=want),
                        ctx.assign_tau_sampled(gamma, eta, seed=4, burn=1, kept=2, want=want)):
                assert set(got) == set(want) | {"map_state", "marg"}
                assert all(got[k].tobytes() == full[k].tobytes() for k in got), want
    finally:
        ctx.close()


def test_every_error_code():
    counts = np.ones((2, 3, 4), dtype=np.int64)
    eta = 0.96 * np.eye(4) + 0.01
    g2 = np.full((3, 2), 0.5)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*G=33 exceeds DSM_MAX_G=32"):
        _lib.assign_tau_sampled(counts, np.full((3, 33), 1.0 / 33), eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*S=513"):
        _lib.assign_tau_sampled(np.ones((1, 513, 4), dtype=np.int64), np.full((513, 2), 0.5), eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*kept=0"):
        _lib.assign_tau_sampled(counts, g2, eta, kept=0)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*burn=-1"):
        _lib.assign_tau_sampled(counts, g2, eta, burn=-1)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*65537"):
        _lib.assign_tau_sampled(counts, g2, eta, burn=65536, kept=1)
    bad = counts.copy(); bad[1, 2, 3] = -1
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*count -1 at position 1, sample 2"):
        _lib.assign_tau_sampled(bad, g2, eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*gamma"):
        _lib.assign_tau_sampled(counts, np.array([[0.5, 0.5], [np.inf, 1.0], [0.5, 0.5]]), eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*eta"):
        _lib.assign_tau_sampled(counts, g2, -eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2"):
        _lib.assign_tau_sampled(counts, g2, eta, device=99)
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4"):
        ctx.assign_tau_sampled(np.full((3, 33), 1.0 / 33), eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2"):
        ctx.assign_tau_sampled(g2, eta, kept=0)
    assert ctx.assign_tau_sampled(g2, eta, burn=65535, kept=1, want=())["marg"].shape == (2, 2, 4)     # B + T at the limit runs
    ctx.close()


# ---- 4. against the exact kernel -----------------------------------------------------------------------------------------------
def test_marginals_and_conf_follow_the_exact_posterior():
    """G = 6, S = 12, N = 64, R = 32 seeds, B = 20, T = 100: per entry of marg, and for conf, |mean over the seeds - exact| <= 5 sd over
    the seeds / sqrt(R) + 2 delta (5: the z convention of tests/_law.py); a statistic that is constant over the seeds must be within
    2 delta.  The figures are printed before the assertion."""
    G, S, N, R, B, T = 6, 12, 64, 32, 20, 100
    counts, gamma, eta = _case(G, S, N, 606, depth=1.0)
    ex = _lib.assign_tau(counts, gamma, eta)
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    runs = [ctx.assign_tau_sampled(gamma, eta, seed=7000 + k, burn=B, kept=T) for k in range(R)]
    ctx.close()
    delta = 1e-12 * np.maximum(1.0, np.abs(loglik_at(counts, gamma, eta, ex["map_state"])))
    same = np.array([(r["map_state"] == ex["map_state"]).all(axis=1) for r in runs])
    for key, tol in (("marg", delta[:, None, None]), ("conf", delta)):
        x = np.array([r[key] for r in runs])
        err, sd = np.abs(x.mean(axis=0) - ex[key]), x.std(axis=0, ddof=1)
        z = err / np.maximum(sd / np.sqrt(R), 1e-300)
        bad = err > 5 * sd / np.sqrt(R) + 2 * tol
        print("%s: %d of %d entries outside the bound; worst z where sd > 0: %.2f; largest error %.3g; map_state = exact at %.1f %%; "
              "largest spread %.3f" % (key, bad.sum(), bad.size, z[sd > 0].max(), err.max(), 100 * same.mean(),
                                       max(r["spread"].max() for r in runs)))
        assert not bad.any(), key


def test_map_state_of_a_peaked_table_is_the_exact_one():
    """The table is the identified one of tests/test_assign_sampled_cpu.py (every haplotype dominates some sample, 240 reads per
    sample): there a site's own samples decide its base whatever the other sites hold, so the ascent from a corner start has no
    local maximum to end in.  With diffuse Dirichlet(1) abundances it has: measured on the MI355X at the same depth, the polished
    state was the exact one at 18 of 32 positions and spread > 0.1 at 30 ("What the chain cannot do")."""
    from test_assign_sampled_cpu import _case as identified_case
    G, S, N = 8, 12, 32
    counts, gamma, eta = identified_case(G, S, N, 60, 808)
    ex = _lib.assign_tau(counts, gamma, eta)
    assert (ex["conf"] > 0.999).all()
    res = _lib.assign_tau_sampled(counts, gamma, eta, seed=1, burn=20, kept=100)
    agree = (res["map_state"] == ex["map_state"]).all(axis=1)
    print("peaked G = 8: map_state = exact at %d of %d positions; spread > 0.1 at %d" % (agree.sum(), N, (res["spread"] > 0.1).sum()))
    assert agree.all()
    L = loglik_at(counts, gamma, eta, res["map_state"])
    assert (np.abs(res["map_ll"] - L) <= 1e-12 * np.abs(L)).all()


def test_spread_flags_every_wrong_call_on_a_table_that_traps_the_chains():
    """The documented limit as an assertion ("What the chain cannot do"): Dirichlet(1) abundances at S = 12, G = 8,
    240 reads per sample.  The exact posterior is a point mass at every position; corner starts are trapped in swapped-base local
    maxima, the polished best state is the exact one at only 18 of 32 positions -- and every one of the 14 wrong calls comes back with
    spread > 0.1 (all 14 with spread 1.0; 30 of 32 positions are flagged in all).  A wrong call with a small spread fails this test."""
    G, S, N = 8, 12, 32
    counts, gamma, eta = _case(G, S, N, 808, depth=240.0, conc=1.0)
    ex = _lib.assign_tau(counts, gamma, eta)
    assert (ex["conf"] > 0.999).all()
    res = _lib.assign_tau_sampled(counts, gamma, eta, seed=1, burn=20, kept=100)
    wrong = ~(res["map_state"] == ex["map_state"]).all(axis=1)
    flagged = res["spread"] > 0.1
    print("trapping table: %d of %d calls wrong, %d positions flagged, smallest spread of a wrong call %.3f"
          % (wrong.sum(), N, flagged.sum(), res["spread"][wrong].min() if wrong.any() else np.nan))
    assert wrong.any()                                                      # (else the table shows nothing)
    assert not (wrong & ~flagged).any()
    assert (res["conf"][wrong] <= 0.75).all()                               # at least one chain sits elsewhere: never a confident call


def test_class_method_is_the_module_call():
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    G, S, N = 4, 6, 11
    counts, gamma, eta = _case(G, S, N, 21)
    smp = HaploSNP_Sampler(counts, G, np.random.RandomState(3), max_iter=1)
    smp.gamma_star, smp.eta_star = gamma, eta
    want = _lib.assign_tau_sampled(counts, gamma, eta, seed=77, burn=3, kept=6)
    got = smp.assignTauSampled(counts.reshape(N, -1), kept=6, burn=3, seed=77)
    assert got["tau"].shape == (N, G, 4) and got["tau"].dtype == np.int64 and (got["tau"].sum(axis=2) == 1).all()
    assert np.array_equal(np.argmax(got["tau"], axis=2), want["map_state"]) and np.array_equal(np.argmax(got["draw"], axis=2), want["draw_state"])
    for k in ("map_ll", "conf", "marg", "spread"):
        assert got[k].tobytes() == want[k].tobytes(), k
    a, b = smp.assignTauSampled(counts.reshape(N, -1), kept=6, burn=3), smp.assignTauSampled(counts.reshape(N, -1), kept=6, burn=3)
    assert not np.array_equal(a["marg"], b["marg"])                         # seed=None: one randint of the sampler's stream per call


# ---- 5. G = 12 end to end ------------------------------------------------------------------------------------------------------
def test_cli_at_g12(tmp_path, capsys):
    from desman_amd import assign
    G, S, N = 12, 12, 40
    counts, gamma, eta = _case(G, S, N, 1212, depth=30.0)
    names = ["S%d" % s for s in range(S)]
    run = tmp_path / "run"
    run.mkdir()
    pd.DataFrame(gamma, index=names).to_csv(run / "Gamma_star.csv")
    pd.DataFrame(eta).to_csv(run / "Eta_star.csv")
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    table = pd.DataFrame(np.concatenate([np.arange(N)[:, None] * 7 + 3, counts.reshape(N, S * 4)], axis=1),
                         index=["contig%d" % (v // 25) for v in range(N)], columns=cols)
    table.index.name = "Contig"
    freq = str(tmp_path / "new.freq")
    table.to_csv(freq)
    out = str(tmp_path / "out")
    capsys.readouterr()
    got = assign.main([str(run), freq, "-o", out, "--sampled", "40", "--burn", "10", "--seed", "5"])
    assert "desman-assign --sampled: %d of %d positions with spread > 0.1" % ((got["spread"] > 0.1).sum(), N) in capsys.readouterr().err
    _, g_read, e_read = assign.load_model(str(run))
    want = _lib.assign_tau_sampled(counts, g_read, e_read, seed=5, burn=10, kept=40)
    assert _same(got, want)
    star = pd.read_csv(os.path.join(out, "Assigned_Tau_star.csv"), index_col=0)
    assert list(star.columns) == ["Position"] + [str(i) for i in range(4 * G)] and list(star.index) == list(table.index)
    assert np.array_equal(star["Position"].to_numpy(), table["Position"].to_numpy())
    t = star.to_numpy()[:, 1:].reshape(N, G, 4)
    assert (t.sum(axis=2) == 1).all() and np.array_equal(np.argmax(t, axis=2), want["map_state"])
    for fname, key in (("Assigned_Tau_conf.csv", "conf"), ("Assigned_Tau_spread.csv", "spread")):
        fr = pd.read_csv(os.path.join(out, fname), index_col=0, float_precision="round_trip")
        assert list(fr.columns) == ["Position", "0"] and np.array_equal(fr["0"].to_numpy(), want[key])
    mean = pd.read_csv(os.path.join(out, "Assigned_Tau_mean.csv"), index_col=0, float_precision="round_trip")
    assert np.array_equal(mean.to_numpy()[:, 1:].reshape(N, G, 4), want["marg"])
    assert open(os.path.join(out, "assign_fit.txt")).read() == "AssignSampled,%d,%d,10,40,%f\n" % (G, N, want["map_ll"].sum())
    assign.main([str(run), freq, "-o", out, "--sampled", "40", "--burn", "10", "--seed", "5", "--draw"])
    t = pd.read_csv(os.path.join(out, "Assigned_Tau_star.csv"), index_col=0).to_numpy()[:, 1:].reshape(N, G, 4)
    assert np.array_equal(np.argmax(t, axis=2), want["draw_state"])
    with pytest.raises(SystemExit) as e:                                     # without --sampled: the exit of the exact call
        assign.main([str(run), freq, "-o", out])
    assert "12 haplotypes; all 4^G joint states are evaluated, the limit is G = 10" in str(e.value.code)
