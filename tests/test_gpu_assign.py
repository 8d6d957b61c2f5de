"""Exact joint haplotype assignment on the device (dsm_assign_tau / dsm_ctx_assign_tau, kernels_assign.hip) against the
reference's goldens (tests/golden/assign_tau_*.npz) and the numpy restatement of tests/test_assign_cpu.py.

Tolerances (set by the model, not by what the kernel gives): with delta = 1e-12 max_t |L(t)| of a position -- the project's
log-likelihood tolerance (loglik.npz) applied to every L(t) -- logz is held to 1e-12 relative with delta as absolute floor,
conf to 2 delta relative and marg to 2 delta absolute (conf = 1 / sum exp(L - L_max), each L carrying delta)."""
import os

import numpy as np
import pandas as pd
import pytest

from desman_amd import _lib
from _law import chi2_vs_pmf
from test_assign_cpu import FIXTURES, assign_numpy, digits_of, load_fixture, loglik_at

pytestmark = pytest.mark.gpu
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]


def _check(res, ref, what):
    """device results against a reference dict (assign_numpy's keys); returns the measured maxima in units of the tolerances"""
    # max_t |L(t)| where the reference has the whole table (the goldens); else |L_max|, which is smaller: a stricter bound
    scale = ref["labs"] if "labs" in ref else np.where(np.isfinite(ref["lmax"]), np.abs(ref["lmax"]), 0.0)
    delta = 1e-12 * np.maximum(scale, 1.0)
    live = np.isfinite(ref["logz"])
    assert np.array_equal(np.isfinite(res["logz"]), live), what
    e_logz = np.abs(res["logz"][live] - ref["logz"][live]) / np.maximum(1e-12 * np.abs(ref["logz"][live]), delta[live])
    e_conf = np.abs(res["conf"][live] - ref["conf"][live]) / (ref["conf"][live] * 2 * delta[live])
    e_marg = np.abs(res["marg"][live] - ref["marg"][live]).max(axis=(1, 2)) / (2 * delta[live])
    worst = [float(e.max()) if e.size else 0.0 for e in (e_logz, e_conf, e_marg)]
    print("%s: error / tolerance: logz %.3g, conf %.3g, marg %.3g" % (what, *worst))
    assert max(worst) <= 1.0, (what, worst)
    assert not np.isnan(res["conf"]).any() and not np.isnan(res["marg"]).any() and not np.isnan(res["logz"]).any(), what
    assert (np.abs(res["marg"][live].sum(axis=2) - 1.0) <= 1e-12).all(), what
    dead = ~live
    assert (res["conf"][dead] == 0).all() and (res["logz"][dead] == -np.inf).all() and not res["marg"][dead].any() and \
        not res["map_state"][dead].any(), what
    return worst


# ---- 1. the goldens ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_goldens(path):
    """Measured on the MI355X, worst position, as a fraction of the tolerance: logz 6.5e-5 / 7.4e-5 / 6.6e-5, conf 1.4e-5 / 8.8e-6 /
    6.9e-6, marg 9.6e-6 / 4.7e-6 / 4.7e-6 (G = 3 / 4 / 5 fixture): errors of a few ulp.  The tolerances are the issue's, not tightened
    (DESIGN.md sec. 8a)."""
    f = load_fixture(path)
    L, G = f["L"], f["G"]
    res = _lib.assign_tau(f["counts"], f["gamma"], f["eta"])
    assert np.array_equal(res["map_state"], f["state_digits"][np.argmax(L, axis=1)])
    M = L.max(axis=1)
    w = np.exp(L - M[:, None])
    Z = w.sum(axis=1)
    onehot = np.zeros((4 ** G, G * 4))
    onehot[np.arange(4 ** G)[:, None], np.arange(G) * 4 + f["state_digits"]] = 1.0
    ref = dict(logz=M + np.log(Z), conf=f["conf"], marg=((w @ onehot) / Z[:, None]).reshape(-1, G, 4), lmax=M, labs=np.abs(L).max(axis=1))
    _check(res, ref, os.path.basename(path))


# ---- 2. shapes without goldens -------------------------------------------------------------------------------------------------
# (G, S, N, the boundary of kernels_assign.hip the case crosses)
SHAPES = [
    (1, 1, 1, "G < 3: 4 live lanes of 64, one sample, one position"),
    (1, 7, 63, "G = 1, a merge workgroup one position short of full"),
    (2, 64, 64, "G = 2: 16 live lanes; the cell list built in exactly one 64-sample pass; a full merge workgroup"),
    (2, 96, 65, "cell list built in two sample passes; the merge grid's second workgroup holds one position"),
    (3, 1, 5000, "G = 3: all lanes live, no outer haplotype, one block; many positions"),
    (3, 64, 65, "G = 3 at the flagship S"),
    (3, 300, 64, "five sample passes, ~1200 cells"),
    (4, 7, 64, "first outer haplotype: 4 partials of one block each"),
    (4, 96, 63, "G = 4 with a two-pass cell list"),
    (6, 7, 1, "64 partials of one block each, a single position"),
    (6, 64, 65, "64 partials at the flagship S"),
    (6, 512, 2, "DSM_MAX_S: more than 64 KB of LDS asked for by attribute"),
    (8, 1, 3, "partials of 16 blocks: the running maximum moves inside a partial, S = 1"),
    (8, 64, 6, "flagship shape: 16 blocks per partial, five outer haplotypes"),
    (8, 96, 2, "G = 8 with a two-pass cell list"),
]


def _shape_case(G, S, N, seed):
    rs = np.random.RandomState(seed)
    gamma = rs.dirichlet(np.full(G, 0.5), size=S)
    eta = 0.05 * rs.dirichlet(np.ones(4), size=4) + 0.95 * np.eye(4)
    tau = rs.randint(0, 4, size=(N, G))
    # shallow, and the shallower the more samples per haplotype there are (about 3 G reads per position): open posteriors, many zero cells
    depth = rs.poisson(rs.uniform(0.3, 6.0, size=(N, S)) * min(1.0, float(G) / S))
    depth[::5] = rs.randint(40, 500, size=depth[::5].shape)                 # ... and every fifth position deep
    p = np.einsum("sg,ngb->nsb", gamma, eta[tau])
    counts = np.array([[rs.multinomial(depth[n, s], p[n, s] / p[n, s].sum()) for s in range(S)] for n in range(N)], dtype=np.int64)
    return counts, gamma, eta


@pytest.mark.parametrize("G,S,N,why", SHAPES, ids=["G%d_S%d_N%d" % s[:3] for s in SHAPES])
def test_shapes_against_numpy(G, S, N, why):
    counts, gamma, eta = _shape_case(G, S, N, 9000 + 100 * G + S + N)
    res = _lib.assign_tau(counts, gamma, eta)
    ref = assign_numpy(counts, gamma, eta)
    _check(res, ref, "G%d S%d N%d" % (G, S, N))
    assert N < 60 or (ref["conf"] < 0.99).mean() >= 0.15                     # (a table of point-mass posteriors would show nothing)
    # the MAP state: the device's choice is a maximiser of the restatement's L (equal index wherever the race is not a rounding tie)
    L_dev = loglik_at(counts, gamma, eta, res["map_state"])
    tol = 2e-12 * np.maximum(1.0, np.abs(ref["lmax"]))
    assert (L_dev >= ref["lmax"] - tol).all()
    assert (res["map_state"] == ref["map_state"]).all(axis=1).mean() >= 0.95     # (exact model ties, see test_edge_operands)


# ---- 3. edge operands ----------------------------------------------------------------------------------------------------------
def test_edge_operands():
    rs = np.random.RandomState(77)
    G, S, N = 4, 5, 12
    gamma = rs.dirichlet(np.ones(G), size=S)
    gamma[2] = [1.0 - 3e-6, 1e-6, 1e-6, 1e-6]                               # a row at the 1e-6 clamp
    eta = 0.96 * np.eye(4) + 0.01
    counts = rs.poisson(3.0, size=(N, S, 4)).astype(np.int64)
    counts[0] = 0                                                           # a position without reads: every state ties
    counts[:, 4] = 0                                                        # a sample without reads anywhere
    counts[3] = 0; counts[3, 1] = [(2 ** 31 - 1) // S - 3, 2, 0, 0]         # counts near 2^31 / S
    res = _lib.assign_tau(counts, gamma, eta, seed=5)
    ref = assign_numpy(counts, gamma, eta, want_L=True)
    _check(res, ref, "edges")
    assert not res["map_state"][0].any() and res["conf"][0] == 4.0 ** -G and np.array_equal(res["marg"][0], np.full((G, 4), 0.25))
    assert res["logz"][0] == pytest.approx(G * np.log(4.0), rel=1e-15)
    # a position without reads of two of the bases has states that tie exactly in the model (the symmetric eta cannot tell the two
    # unseen bases apart; one such position is in this table): rounding may order them either way, so the index is compared where
    # the best state leads by more than rounding, and everywhere the device's state must be a maximiser
    srt = np.sort(ref["L"], axis=1)
    clear = srt[:, -1] - srt[:, -2] > 1e-9
    assert clear.sum() >= N - 2 and np.array_equal(res["map_state"][clear], ref["map_state"][clear])
    assert (loglik_at(counts, gamma, eta, res["map_state"]) >= ref["lmax"] - 2e-12 * np.maximum(1.0, np.abs(ref["lmax"]))).all()
    for k in ("conf", "logz", "marg"):
        assert np.isfinite(res[k]).all()

    # the identity eta: a state inconsistent with an observed base has L = -inf and gets no mass (the operand class of 0 ln 0)
    g2 = np.array([[0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.2, 0.3, 0.5]])
    c2 = np.zeros((5, 3, 4), dtype=np.int64)
    c2[1, 0] = [3, 0, 0, 1]                                                 # A and T in a sample made of haplotypes 0 and 1
    c2[2, 1] = [1, 1, 0, 0]                                                 # A and C in a sample that is haplotype 0 alone: impossible
    c2[3, 2] = [4, 0, 2, 9]                                                 # three bases over three haplotypes
    c2[4] = c2[2]; c2[4, 0] = [5, 0, 0, 0]
    r2 = _lib.assign_tau(c2, g2, np.eye(4), seed=9)
    ref2 = assign_numpy(c2, g2, np.eye(4))
    _check(r2, ref2, "identity eta")
    assert np.array_equal(r2["map_state"], ref2["map_state"])
    assert r2["conf"][2] == 0.0 and r2["logz"][2] == -np.inf and not r2["marg"][2].any() and not r2["draw_state"][2].any()
    assert r2["conf"][4] == 0.0 and r2["logz"][4] == -np.inf
    assert r2["conf"][1] == pytest.approx(1.0 / 8, rel=1e-14)                # (A,T,*) and (T,A,*): 8 states of equal mass
    assert np.array_equal(r2["marg"][1, 0], [0.5, 0.0, 0.0, 0.5]) and np.allclose(r2["marg"][1, 2], 0.25, rtol=1e-15)
    # a draw never lands on a state without mass
    L_draw = loglik_at(c2, g2, np.eye(4), r2["draw_state"])
    assert np.isfinite(L_draw[[0, 1, 3]]).all()


# ---- 4. the draw, in law -------------------------------------------------------------------------------------------------------
def test_draw_follows_the_exact_posterior():
    f = load_fixture([p for p in FIXTURES if "_G3" in p][0])
    G, N = f["G"], f["counts"].shape[0]
    ctx = _lib.Context(0)
    ctx.set_counts(f["counts"])
    n_seeds = 2400
    draws = np.empty((n_seeds, N), dtype=np.int64)
    w = 4 ** (G - 1 - np.arange(G))
    for k in range(n_seeds):
        draws[k] = (ctx.assign_tau(f["gamma"], f["eta"], seed=1000 + k)["draw_state"].astype(np.int64) * w).sum(axis=1)
    again = ctx.assign_tau(f["gamma"], f["eta"], seed=1000)
    assert np.array_equal((again["draw_state"].astype(np.int64) * w).sum(axis=1), draws[0])          # same seed, same draw
    ctx.close()
    post = np.exp(f["L"] - f["L"].max(axis=1, keepdims=True))
    post /= post.sum(axis=1, keepdims=True)
    flat = np.argsort(f["conf"])[:10]                                       # the flattest posteriors
    ps = np.array([chi2_vs_pmf(draws[:, n], post[n]) for n in flat])
    print("draw law: p-values of the %d flattest positions %s; off the MAP state in %.1f %% of all draws"
          % (len(flat), np.round(ps, 3), 100 * (draws != np.argmax(f["L"], axis=1)[None, :]).mean()))
    assert ps.min() * len(flat) > 1e-3, ps
    assert (draws != np.argmax(f["L"], axis=1)[None, :]).mean() > 0.05      # the draw is not the MAP call in disguise
    # where the posterior is a point mass the draw is the MAP state
    d = load_fixture([p for p in FIXTURES if "_G5" in p][0])
    res = _lib.assign_tau(d["counts"], d["gamma"], d["eta"], seed=3)
    sure = res["conf"] > 1.0 - 1e-9
    assert sure.sum() >= d["n_deep"] - 1 and np.array_equal(res["draw_state"][sure], res["map_state"][sure])


# ---- 5. one answer whatever the route ------------------------------------------------------------------------------------------
def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) and a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("G,S,N", [(5, 12, 16), (6, 9, 70), (2, 4, 300)])
def test_context_form_chunking_and_reruns_agree_bit_for_bit(G, S, N):
    if (G, S, N) == (5, 12, 16):
        f = load_fixture([p for p in FIXTURES if "_G5" in p][0])
        counts, gamma, eta = f["counts"], f["gamma"], f["eta"]
    else:
        counts, gamma, eta = _shape_case(G, S, N, 31 + G)
    base = _lib.assign_tau(counts, gamma, eta, seed=11)
    assert _same(base, _lib.assign_tau(counts, gamma, eta, seed=11))         # run to run
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    assert _same(base, ctx.assign_tau(gamma, eta, seed=11))                  # the resident tensor
    try:
        for chunk in (1, 7, 64):
            _lib.assign_debug_set_chunk(chunk)
            assert _same(base, _lib.assign_tau(counts, gamma, eta, seed=11)), chunk
            assert _same(base, ctx.assign_tau(gamma, eta, seed=11)), chunk
    finally:
        _lib.assign_debug_set_chunk(0)
        ctx.close()
    other = _lib.assign_tau(counts, gamma, eta, seed=12)
    assert all(np.array_equal(base[k], other[k]) for k in ("map_state", "conf", "logz", "marg"))     # the seed moves the draw only


# ---- 6. classes and command line -----------------------------------------------------------------------------------------------
def _write_freq(path, counts, names):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.arange(V)[:, None] * 7 + 3, counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=["contig%d" % (v // 50) for v in range(V)], columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)
    return df


def test_cli_on_a_fitted_run(tmp_path):
    """Fit a synthetic table with `desman`, then assign the same positions from the run's Gamma_star / Eta_star files.
    Measured on the MI355X: the exact MAP call agrees with the chain's Filtered_Tau_star.csv at 100.0 % of the 240 positions
    (not gated: printed)."""
    from desman_amd import assign, cli
    from desman_amd.synth import synth_counts
    V, S, G = 240, 12, 3
    counts, _, _ = synth_counts(V, S, G, seed=123)
    names = ["S%d" % s for s in range(S)]
    freq = str(tmp_path / "syn.freq")
    _write_freq(freq, counts, names)
    run = str(tmp_path / "run")
    cli.main([freq, "-g", str(G), "-i", "40", "-o", run, "-s", "7"])
    out = str(tmp_path / "assigned")
    # the new table lists the samples in another order, with one the run never saw
    order = [5, 0, 11, 3, 1, 2, 4, 6, 7, 8, 9, 10]
    extra = np.concatenate([counts[:, order, :], counts[:, :1, :]], axis=1)
    freq2 = str(tmp_path / "new.freq")
    table = _write_freq(freq2, extra, [names[k] for k in order] + ["other"])
    assign.main([run, freq2, "-o", out])

    run_names, gamma, eta = assign.load_model(run)
    kept = [names.index(n) for n in run_names]
    ref = assign_numpy(counts[:, kept, :], gamma, eta)
    Gk = gamma.shape[1]
    star = pd.read_csv(os.path.join(out, "Assigned_Tau_star.csv"), index_col=0)
    assert list(star.columns) == ["Position"] + [str(i) for i in range(4 * Gk)]
    assert list(star.index) == list(table.index) and np.array_equal(star["Position"].to_numpy(), table["Position"].to_numpy())
    t = star.to_numpy()[:, 1:].reshape(V, Gk, 4)
    assert (t.sum(axis=2) == 1).all() and np.array_equal(np.argmax(t, axis=2), ref["map_state"])
    conf = pd.read_csv(os.path.join(out, "Assigned_Tau_conf.csv"), index_col=0)
    assert list(conf.columns) == ["Position", "0"]
    mean = pd.read_csv(os.path.join(out, "Assigned_Tau_mean.csv"), index_col=0)
    res = dict(map_state=np.argmax(t, axis=2), conf=conf["0"].to_numpy(), marg=mean.to_numpy()[:, 1:].reshape(V, Gk, 4))
    fit = open(os.path.join(out, "assign_fit.txt")).read().strip().split(",")
    assert fit[0] == "Assign" and int(fit[1]) == Gk and int(fit[2]) == V
    assert float(fit[3]) == pytest.approx(ref["logz"].sum(), rel=1e-9)       # (written with %f)
    res["logz"] = ref["logz"]                                               # per-position logz is not a file; checked through the class below
    _check(res, ref, "cli")

    # the same positions at 0.4 % of their depth (posteriors that are not point masses), as draws
    thin = np.random.RandomState(8).binomial(extra, 0.004)
    freq4 = str(tmp_path / "thin.freq")
    _write_freq(freq4, thin, [names[k] for k in order] + ["other"])
    out4 = str(tmp_path / "thin")
    got4 = assign.main([run, freq4, "-o", out4, "--draw", "--seed", "5"])
    back = {n: j for j, n in enumerate([names[k] for k in order])}
    ref4 = assign_numpy(thin[:, [back[n] for n in run_names], :], gamma, eta)
    assert (ref4["conf"] < 0.99).mean() > 0.2
    _check(got4, ref4, "cli, thinned")
    star4 = pd.read_csv(os.path.join(out4, "Assigned_Tau_star.csv"), index_col=0).to_numpy()[:, 1:].reshape(V, Gk, 4)
    assert np.array_equal(np.argmax(star4, axis=2), got4["draw_state"]) and not np.array_equal(got4["draw_state"], got4["map_state"])
    conf4 = pd.read_csv(os.path.join(out4, "Assigned_Tau_conf.csv"), index_col=0, float_precision="round_trip")["0"].to_numpy()
    assert np.array_equal(conf4, got4["conf"])

    fitted = pd.read_csv(os.path.join(run, "Filtered_Tau_star.csv"), index_col=0)
    key = lambda fr: list(zip(fr.index, fr["Position"]))
    pos = {k: i for i, k in enumerate(key(star))}
    rows = [pos[k] for k in key(fitted)]
    same = (fitted.to_numpy()[:, 1:] == star.to_numpy()[rows, 1:]).all(axis=1)
    print("cli: exact MAP call = chain's tau_star at %.1f %% of %d fitted positions" % (100 * same.mean(), len(rows)))

    # the same through the class: assignTauExact is deterministic, assignTau a seeded draw of the same posterior
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    smp = HaploSNP_Sampler(counts[:, kept, :], Gk, np.random.RandomState(3), max_iter=1)
    smp.gamma_star, smp.eta_star = gamma, eta
    ex = smp.assignTauExact(counts[:, kept, :].reshape(V, -1))
    assert np.array_equal(np.argmax(ex["tau"], axis=2), ref["map_state"]) and ex["tau"].shape == (V, Gk, 4) and ex["tau"].dtype == np.int64
    _check(dict(map_state=ref["map_state"], conf=ex["conf"], logz=ex["logz"], marg=ex["marg"]), ref, "class")
    a1, c1 = smp.assignTau(counts[:, kept, :].reshape(V, -1))
    assert a1.shape == (V, Gk, 4) and (a1.sum(axis=2) == 1).all() and np.array_equal(c1, ex["conf"])

    # a table that lacks one of the run's samples
    freq3 = str(tmp_path / "short.freq")
    _write_freq(freq3, counts[:, 1:, :], names[1:])
    with pytest.raises(SystemExit) as e:
        assign.main([run, freq3, "-o", out])
    assert e.value.code not in (0, None) and "'S0'" in str(e.value.code)


def test_repeated_class_draws_differ_on_open_posteriors():
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    f = load_fixture([p for p in FIXTURES if "_G3" in p][0])
    N = f["counts"].shape[0]
    smp = HaploSNP_Sampler(f["counts"], f["G"], np.random.RandomState(3), max_iter=1)
    smp.gamma_star, smp.eta_star = f["gamma"], f["eta"]
    a1, c1 = smp.assignTau(f["counts"].reshape(N, -1))
    a2, c2 = smp.assignTau(f["counts"].reshape(N, -1))
    assert np.array_equal(c1, c2) and not np.array_equal(a1, a2)             # one randint of the sampler's stream per call, as upstream
    np.testing.assert_allclose(c1, f["conf"], rtol=1e-9)


# ---- 7. the limit ----------------------------------------------------------------------------------------------------------------
def test_g_above_the_limit_is_unsupported():
    counts = np.ones((2, 3, 4), dtype=np.int64)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*DSM_ASSIGN_MAX_G=10"):
        _lib.assign_tau(counts, np.full((3, 11), 1.0 / 11), 0.96 * np.eye(4) + 0.01)
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4"):
        ctx.assign_tau(np.full((3, 11), 1.0 / 11), 0.96 * np.eye(4) + 0.01)
    ctx.close()


def test_g_at_the_limit_runs():
    """G = 10: a million states per position; S = 300 takes the kernel's LDS above the default limit.  Checked against the
    restatement through a symmetry instead of a million-state numpy pass: with equal abundances in every sample the likelihood
    depends on the multiset of bases only, so each haplotype has the same marginal and logz follows from G = 10's multinomial sum."""
    rs = np.random.RandomState(4)
    G, S, N = 10, 300, 2
    gamma = np.full((S, G), 1.0 / G)
    eta = 0.9 * np.eye(4) + 0.025
    counts = rs.poisson(0.05, size=(N, S, 4)).astype(np.int64)
    counts[:, :, 0] += rs.poisson(0.3, size=(N, S))
    res = _lib.assign_tau(counts, gamma, eta, seed=1)
    X = counts.sum(axis=1).astype(np.float64)                                # [N][4]: with equal gamma rows only the totals matter
    from math import factorial, log
    for n in range(N):
        terms, m0 = [], np.zeros(4)
        for k0 in range(G + 1):
            for k1 in range(G + 1 - k0):
                for k2 in range(G + 1 - k0 - k1):
                    k = np.array([k0, k1, k2, G - k0 - k1 - k2])
                    mult = factorial(G) // np.prod([factorial(int(i)) for i in k])
                    Lk = float(X[n] @ np.log((k @ eta) / G))
                    terms.append((Lk + log(mult), k / G))
        Ls = np.array([t[0] for t in terms])
        logz = Ls.max() + np.log(np.exp(Ls - Ls.max()).sum())
        marg = sum(np.exp(t[0] - logz) * t[1] for t in terms)
        assert res["logz"][n] == pytest.approx(logz, rel=1e-12)
        assert np.abs(res["marg"][n] - marg[None, :]).max() <= 2e-12 * max(1.0, abs(Ls).max())
        # the MAP state: a best multiset of bases, and of its arrangements the one with the lowest index (digits ascending)
        plain = {tuple(np.round(t[1] * G).astype(int)): float(X[n] @ np.log(t[1] @ eta)) for t in terms}
        assert plain[tuple(np.bincount(res["map_state"][n], minlength=4))] >= max(plain.values()) - 1e-9
        # (its arrangements tie in the model only: their mixtures are summed in different orders, rounding picks among them)
