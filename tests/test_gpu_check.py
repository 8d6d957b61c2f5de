"""Posterior predictive fit sums from the resident traces (dsm_ctx_trace_fit_stats; kernels_fit.hip) on the GPU, against the numpy
restatement desman_amd/check.py summed on the host.  Tolerance, everywhere: 1e-12 times the sum of the absolute values of the terms
that enter an output element (for D those of n_b ln(n_b / (N p_b)), which cancel) -- the project's likelihood convention; E, a sum of
small integers, is compared exactly.  Worst fraction of that tolerance seen on an MI355X over this file: 0.0052.
The host side alone is tests/test_check_cpu.py.
Run on an MI355X with:  python -m pytest tests/test_gpu_check.py -m gpu
"""
import itertools
import os

import numpy as np
import pandas as pd
import pytest
from numpy.random import RandomState

from desman_amd import _lib, check
from desman_amd.synth import synth_counts, random_state

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = r"error -2: ", r"error -3: "
TOL = 1e-12
WORST = [0.0]


@pytest.fixture()
def ctx():
    c = _lib.Context(0)
    yield c
    _lib.fit_debug_set_parts(0)
    c.close()


def _digits(onehot):
    return np.argmax(onehot, axis=2)


def _per_iter(counts, digits, gamma, eta):
    """cell_terms of every iteration, stacked: dict of [n, V, S] arrays (digits [n, V, G] or [V, G])"""
    n = len(gamma)
    cs = [check.cell_terms(counts, digits if digits.ndim == 2 else digits[t], gamma[t], eta[t]) for t in range(n)]
    return {k: np.stack([c[k] for c in cs]) for k in cs[0]}


def _want(terms, it0=0, n_it=None):
    """the three outputs and the tolerance of each element from _per_iter terms over iterations it0 .. it0 + n_it - 1"""
    sl = slice(it0, None if n_it is None else it0 + n_it)
    keys = (("X", "absX"), ("D", "absD"), ("E", "E"), ("W", "W"))
    with np.errstate(invalid="ignore"):
        sample = np.stack([terms[k][sl].sum(axis=(0, 1)) for k, _ in keys], axis=1)
        position = np.stack([terms[k][sl].sum(axis=(0, 2)) for k, _ in keys], axis=1)
        tol_s = TOL * np.stack([np.abs(terms[m][sl]).sum(axis=(0, 1)) for _, m in keys], axis=1)
        tol_p = TOL * np.stack([np.abs(terms[m][sl]).sum(axis=(0, 2)) for _, m in keys], axis=1)
    tol_s[:, 2] = 0.0
    tol_p[:, 2] = 0.0
    return dict(sample=sample, position=position, cell=terms["X"][sl].sum(axis=0)), \
        dict(sample=tol_s, position=tol_p, cell=TOL * terms["absX"][sl].sum(axis=0))


def _close(got, want, tol, what):
    """every element within its tolerance; +inf exactly where the restatement has it, NaN nowhere"""
    for k in ("sample", "position", "cell"):
        if k not in got:
            continue
        g, w, t = got[k], want[k], tol[k]
        assert g.shape == w.shape and g.dtype == np.float64, (what, k)
        assert not np.isnan(g).any() and not np.isnan(w).any(), (what, k)
        assert np.array_equal(np.isinf(g), np.isinf(w)) and (g[np.isinf(g)] > 0).all(), (what, k)
        fin = np.isfinite(w)
        err = np.abs(g[fin] - w[fin])
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(err > 0, err / t[fin], 0.0)
        if frac.size:
            WORST[0] = max(WORST[0], float(frac.max()))
        assert (err <= t[fin]).all(), (what, k, float(frac.max()) if frac.size else 0.0)
    print("worst fraction of the tolerance so far: %.3g" % WORST[0])


def _plant(c, V, S, G, n, seed=0, depth=60):
    rs = RandomState(7000 + 31 * V + 7 * S + G + seed)
    counts = rs.randint(0, depth, size=(V, S, 4)).astype(np.int64)
    counts[rs.random_sample((V, S)) < 0.05] = 0
    c.set_counts(counts)
    tau, gamma0, eta0 = random_state(V, S, G, seed=5 + seed)
    c.set_state(tau, gamma0, eta0)
    digits = rs.randint(0, 4, size=(n, V, G))
    gamma = rs.dirichlet(np.ones(G), size=(n, S))
    eta = 0.9 * np.eye(4) + 0.1 * rs.dirichlet(np.ones(4), size=(n, 4))
    c.debug_set_trace(digits)
    c.debug_set_param_trace(gamma, eta)
    return counts, digits, gamma, eta


# ---- 1. planted traces: every instantiation, tile boundary, chunked gamma, every split into parts, sub-ranges ---------------------------
#          V    S    G   n  nsl lpv
SHAPES = [(1, 1, 1, 1, 1, 1), (63, 3, 2, 2, 1, 4), (64, 8, 3, 7, 1, 8), (65, 9, 5, 7, 1, 16), (257, 16, 8, 7, 1, 16),
          (1000, 17, 12, 7, 1, 32), (65, 33, 16, 7, 1, 64), (63, 64, 32, 2, 1, 64), (65, 65, 5, 7, 2, 64), (64, 130, 3, 7, 4, 64),
          (5, 512, 12, 2, 8, 64), (257, 9, 3, 40, 1, 16)]


@pytest.mark.parametrize("V,S,G,n,nsl,lpv", SHAPES)
def test_planted_trace_in_every_split(ctx, V, S, G, n, nsl, lpv):
    counts, digits, gamma, eta = _plant(ctx, V, S, G, n)
    path = ctx.fit_debug_path()
    assert (path["nsl"], path["lpv"]) == (nsl, lpv) and path["tiles"] == -(-V // (256 // lpv)) and 1 <= path["parts"] <= n
    assert path["gc"] == min(G, 4096 // (nsl * lpv))
    terms = _per_iter(counts, digits, gamma, eta)
    want, tol = _want(terms)
    for parts in sorted({0, 1, 2, 3, n, n + 5}):
        _lib.fit_debug_set_parts(parts)
        if parts:
            assert ctx.fit_debug_path()["parts"] == min(parts, n)
        got = ctx.trace_fit_stats()
        assert got["n_it"] == n
        _close(got, want, tol, (parts,))
        again = ctx.trace_fit_stats()
        assert all(again[k].tobytes() == got[k].tobytes() for k in ("sample", "position", "cell")), parts
        assert np.array_equal(got["sample"][:, 2], want["sample"][:, 2]) and np.array_equal(got["position"][:, 2], want["position"][:, 2])
    _lib.fit_debug_set_parts(0)
    for it0, n_it in {(n // 2, n - n // 2), (1 if n > 1 else 0, max(n - 2, 0)), (n - 1, 1)}:
        if n_it < 1:
            continue
        w, t = _want(terms, it0, n_it)
        for parts in (0, 2):
            _lib.fit_debug_set_parts(parts)
            _close(ctx.trace_fit_stats(it0=it0, n_it=n_it), w, t, (it0, n_it, parts))


# ---- 2. degenerate operands -------------------------------------------------------------------------------------------------------------
def test_degenerate_operands(ctx):
    """an empty sample (3) and an empty position (4), counts near 2^20, exact zeros in eta (base 3 is never produced, base 2 only by true
    base 2) and in gamma (sample 1 has no haplotype 2, sample 2 nothing but haplotype 1): cell (0, 1) has reads of base 2 where
    p_2 = 0, so X and D are +inf there, in sample 1's row and in position 0's row, and nowhere else; nothing is NaN"""
    rs = RandomState(5)
    V, S, G, n = 5, 4, 3, 3
    counts = rs.randint((1 << 20) - 1000, (1 << 20) + 1000, size=(V, S, 4)).astype(np.int64)
    counts[:, :, 3] = 0
    counts[:, 3, :] = 0
    counts[4, :, :] = 0
    digits1 = np.array([[0, 1, 2], [0, 0, 1], [1, 1, 1], [2, 0, 1], [0, 1, 2]])
    counts[1, :, 2] = 0
    counts[2, :, 2] = 0
    counts[3, 1, 2] = 0                                      # (3, 1): true base 2 only through haplotype 0 ... which sample 1 has: finite
    counts[3, 2, 2] = 0                                      # sample 2 = haplotype 1 only: base 0 at position 3, p_2 = 0 = n_2
    counts[0, 2, 0] = 0
    counts[0, 2, 2] = 0                                      # sample 2 at position 0: true base 1 only: p = (0.1, 0.9, 0, 0)
    counts[4, :, :] = 0
    gamma1 = np.array([[0.5, 0.3, 0.2], [0.6, 0.4, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    eta1 = np.array([[0.9, 0.1, 0.0, 0.0], [0.1, 0.9, 0.0, 0.0], [0.05, 0.05, 0.9, 0.0], [0.25, 0.25, 0.5, 0.0]])
    ctx.set_counts(counts)
    tau, g0, e0 = random_state(V, S, G, seed=1)
    ctx.set_state(tau, g0, e0)
    digits, gamma, eta = np.broadcast_to(digits1, (n, V, G)), np.broadcast_to(gamma1, (n, S, G)), np.broadcast_to(eta1, (n, 4, 4))
    ctx.debug_set_trace(digits)
    ctx.debug_set_param_trace(gamma, eta)
    terms = _per_iter(counts, digits, gamma, eta)
    want, tol = _want(terms)
    inf = np.zeros((V, S), dtype=bool)
    inf[0, 1] = True
    assert np.array_equal(np.isinf(want["cell"]), inf)       # the restatement itself
    for parts in (0, 1, 3):
        _lib.fit_debug_set_parts(parts)
        got = ctx.trace_fit_stats()
        _close(got, want, tol, parts)
        assert np.array_equal(np.isinf(got["cell"]), inf)
        assert np.array_equal(np.isinf(got["sample"]), [[False] * 4, [True, True, False, False], [False] * 4, [False] * 4])
        assert np.array_equal(np.isinf(got["position"]), [[True, True, False, False]] + [[False] * 4] * 4)
        assert not got["sample"][3].any() and not got["position"][4].any() and not got["cell"][:, 3].any() and not got["cell"][4].any()
    sc = check.fit_scores(got, n, counts)
    assert sc["sample"]["z"][1] == np.inf and not np.isnan(sc["sample"]["z"]).any() and not np.isnan(sc["position"]["z"]).any()


# ---- 3. NULL outputs, n_it = 0, error codes --------------------------------------------------------------------------------------------
def test_null_outputs_edge_calls_and_error_codes(ctx):
    V, S, G, n = 70, 5, 3, 6
    rs = RandomState(9)
    counts = rs.randint(0, 30, size=(V, S, 4)).astype(np.int64)
    ctx.set_counts(counts)
    tau, g0, e0 = random_state(V, S, G, seed=3)
    ctx.set_state(tau, g0, e0)
    for call in (lambda: ctx.trace_fit_stats(0, 0), lambda: ctx.trace_fit_stats(0, 2)):
        with pytest.raises(_lib.DesmanHipError, match=ERR_STATE + ".*no update has run"):
            call()
    gam, et = rs.dirichlet(np.ones(G), size=(n, S)), np.broadcast_to(e0, (n, 4, 4))
    with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
        ctx.debug_set_param_trace(gam[:1], et[:1])            # no trace yet: its length is 0
    counts, digits, gamma, eta = _plant(ctx, V, S, G, n)
    full = ctx.trace_fit_stats()
    keys = ("sample", "position", "cell")
    for r in range(4):
        for want in itertools.combinations(keys, r):          # all eight combinations of NULL outputs
            part = ctx.trace_fit_stats(want=want)
            assert set(part) == set(want) | {"n_it"} and all(part[k].tobytes() == full[k].tobytes() for k in want), want
    assert ctx.lib.dsm_ctx_trace_fit_stats(ctx._h, 0, n, None, None, None) == 0
    for it0 in (0, 3, n):
        z = ctx.trace_fit_stats(it0=it0, n_it=0)
        assert z["n_it"] == 0 and not any(z[k].any() for k in keys)
    cases = [lambda: ctx.trace_fit_stats(it0=-1, n_it=2), lambda: ctx.trace_fit_stats(it0=5, n_it=2), lambda: ctx.trace_fit_stats(it0=7, n_it=0),
             lambda: ctx.trace_fit_stats(it0=0, n_it=-1), lambda: ctx.trace_fit_stats(it0=0, n_it=n + 1),
             lambda: ctx.debug_set_param_trace(np.concatenate([gamma, gamma[:1]]), np.concatenate([eta, eta[:1]])),
             lambda: _lib.fit_debug_set_parts(-1), lambda: ctx.fit_debug_path(0)]
    for k, call in enumerate(cases):
        with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
            call()
        assert ctx.trace_fit_stats()["sample"].tobytes() == full["sample"].tobytes(), k
    with pytest.raises(ValueError):
        ctx.trace_fit_stats(want=("sample", "cells"))
    with pytest.raises(ValueError):
        ctx.debug_set_param_trace(gamma[:, :, :2], eta)
    ctx.debug_set_param_trace(gamma[:0], eta[:0])             # n = 0: a no-op
    ctx.debug_set_param_trace(gamma[3:5], eta[3:5])           # the first two rows only
    terms = _per_iter(counts, digits, np.concatenate([gamma[3:5], gamma[2:]]), np.concatenate([eta[3:5], eta[2:]]))
    _close(ctx.trace_fit_stats(), *_want(terms), "partly overwritten")


# ---- 4. a fixed-tau trace -----------------------------------------------------------------------------------------------------------------
def test_fixed_tau_trace(ctx):
    V, S, G, n = 150, 8, 4, 9
    counts, _, _ = synth_counts(V, S, G, seed=41)
    tau, gamma, eta = random_state(V, S, G, seed=42)
    ctx.set_counts(counts); ctx.set_state(tau, gamma, eta); ctx.seed(5, ctr_seed=99)
    ctx.gibbs_update_fixed_tau(n, pool=0)
    tr = ctx.get_trace()
    terms = _per_iter(counts, _digits(tau), tr["gamma"], tr["eta"])
    for parts, it0, n_it in ((0, 0, n), (2, 0, n), (4, 0, n), (3, 2, 5), (0, 8, 1)):
        _lib.fit_debug_set_parts(parts)
        _close(ctx.trace_fit_stats(it0=it0, n_it=n_it), *_want(terms, it0, n_it), (parts, it0, n_it))


# ---- 5. a real chain: against get_trace / get_tau_at, the deviance against the chain's own log-likelihood, bitwise continuation ------------
def _chain(c, counts, tau, gamma, eta, n):
    c.set_counts(counts); c.set_state(tau, gamma, eta); c.seed(4321, ctr_seed=0xABCDEF12345)
    c.set_tau_rng(_lib.RNG_MT19937)
    c.gibbs_update(n)


def test_real_chain_deviance_identity_and_bitwise_continuation(ctx):
    V, S, G, n = 130, 6, 3, 20
    counts, _, _ = synth_counts(V, S, G, seed=31)
    tau, gamma, eta = random_state(V, S, G, seed=32)
    twin = _lib.Context(0)
    try:
        _chain(ctx, counts, tau, gamma, eta, n)
        _chain(twin, counts, tau, gamma, eta, n)
        tr = ctx.get_trace()
        digits = np.stack([_digits(ctx.get_tau_at(t)) for t in range(n)])
        terms = _per_iter(counts, digits, tr["gamma"], tr["eta"])
        for parts, it0, n_it in ((0, 0, n), (1, 0, n), (3, 0, n), (2, 5, 11), (n, 0, n)):
            _lib.fit_debug_set_parts(parts)
            got = ctx.trace_fit_stats(it0=it0, n_it=n_it)
            _close(got, *_want(terms, it0, n_it), (parts, it0, n_it))
            again = ctx.trace_fit_stats(it0=it0, n_it=n_it)
            assert all(again[k].tobytes() == got[k].tobytes() for k in ("sample", "position", "cell"))
        _lib.fit_debug_set_parts(0)
        # ll_trace[t] is the log-likelihood of the stored triple (tau_t, gamma_t, eta_t) (api.hip: the sweep's epilogue runs on the new
        # tau and gamma with the new eta), and D = 2 (saturated - ll) cell by cell, so between two iterations the saturated part cancels
        dev = [ctx.trace_fit_stats(it0=t, n_it=1, want=("sample",))["sample"][:, 1].sum() for t in range(n)]
        mag = 2.0 * terms["absD"].sum(axis=(1, 2))
        for t1, t2 in ((0, n - 1), (3, 12), (7, 8)):
            lhs, rhs = dev[t1] - dev[t2], -2.0 * (tr["ll"][t1] - tr["ll"][t2])
            tol = TOL * (mag[t1] + mag[t2]) + 2.0 * TOL * (abs(tr["ll"][t1]) + abs(tr["ll"][t2]))
            print("deviance identity (%d, %d): %.17g vs %.17g, %.3g of the tolerance" % (t1, t2, lhs, rhs, abs(lhs - rhs) / tol))
            assert abs(lhs - rhs) <= tol, (t1, t2, lhs, rhs, tol)
        # nothing of the chain moved: five more iterations equal the twin's, on which none of this was called
        assert np.array_equal(ctx.get_mt_state(), twin.get_mt_state()) and ctx.counters() == twin.counters()
        a, b = ctx.get_trace(), twin.get_trace()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        ctx.gibbs_update(5); twin.gibbs_update(5)
        a, b = ctx.get_trace(), twin.get_trace()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        for t in range(-1, 5):
            assert ctx.get_tau_at(t).tobytes() == twin.get_tau_at(t).tobytes(), t
        for x, y in zip(ctx.get_state(), twin.get_state()):
            assert x.tobytes() == y.tobytes()
        sa, sb = ctx.get_star(), twin.get_star()
        assert sa["lp"] == sb["lp"] and sa["it"] == sb["it"] and np.array_equal(sa["tau"], sb["tau"])
    finally:
        twin.close()


# ---- 6. command line ---------------------------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_desman_check(tmp_path, caplog, monkeypatch):
    import logging
    from desman_amd import cli
    caplog.set_level(logging.INFO)
    V, S, G, n = 120, 8, 3, 20
    counts, _, _ = synth_counts(V, S, G, seed=123)
    freq = str(tmp_path / "fit.freq")
    names = ["S%d" % s for s in range(S)]
    contigs, positions = ["contig%d" % (v // 50) for v in range(V)], np.arange(V) * 7 + 3
    _write_freq(freq, counts, names, contigs, positions)
    seen = []
    report_check = cli._report_check

    def keep(report, chain, cells):
        seen.append((chain, cells))
        report_check(report, chain, cells)
    monkeypatch.setattr(cli, "_report_check", keep)
    plain, chk, both = (str(tmp_path / d) for d in ("plain", "check", "both"))
    args = [freq, "-g", str(G), "-i", str(n), "-s", "7"]
    cli.main(args + ["-o", plain])
    assert not seen
    caplog.clear()
    cli.main(args + ["-o", chk, "--check", "--check-cells"])
    log_check = caplog.text
    cli.main(args + ["-o", both, "--relabel", "--diagnose", "--check"])
    assert [c for _, c in seen] == [True, False]
    new = ["Fit_samples.csv", "Fit_positions.csv", "Fit_cells.csv"]
    assert sorted(os.listdir(chk)) == sorted(os.listdir(plain) + new)
    assert set(new[:2]) <= set(os.listdir(both)) and "Fit_cells.csv" not in os.listdir(both) and "Tau_MCSE.csv" in os.listdir(both)
    read = lambda d, name: open(os.path.join(d, name), "rb").read()
    for name in os.listdir(plain):                             # the usual files do not change
        if name != "log_file.txt":
            assert read(plain, name) == read(chk, name) == read(both, name), name
    for name in new[:2]:                                       # the same chain, the same bits, whatever else was asked for
        assert read(chk, name) == read(both, name), name
    chain = seen[0][0]
    samples, pos, cell = chain.fitCheck(cells=True)
    fs = pd.read_csv(os.path.join(chk, "Fit_samples.csv"), float_precision="round_trip")
    assert list(fs.columns) == ["sample", "cells", "X2", "expected", "z", "deviance"] and list(fs["sample"]) == names
    for col in ("cells", "X2", "expected", "z", "deviance"):
        assert np.array_equal(fs[col].to_numpy(), samples[col]), col
    fp = pd.read_csv(os.path.join(chk, "Fit_positions.csv"), float_precision="round_trip")
    tm = pd.read_csv(os.path.join(chk, "Tau_Mean.csv"))
    assert list(fp.columns) == ["Contig", "Position", "cells", "X2", "expected", "z", "deviance"] and len(fp) == V
    assert list(fp["Contig"]) == list(tm.iloc[:, 0]) == contigs and np.array_equal(fp["Position"], tm["Position"])
    for col in ("cells", "X2", "expected", "z", "deviance"):
        assert np.array_equal(fp[col].to_numpy(), pos[col]), col
    fc = pd.read_csv(os.path.join(chk, "Fit_cells.csv"), float_precision="round_trip")
    assert list(fc.columns) == ["Contig", "Position"] + names and np.array_equal(fc[names].to_numpy(), cell)
    # the table against the restatement fed from the chain's own stores
    ctx = chain._ctx
    digits = np.stack([_digits(ctx.get_tau_at(t)) for t in range(n)])
    terms = _per_iter(chain.variants, digits, chain.gamma_store[:n], chain.eta_store[:n])
    want, tol = _want(terms)
    assert (np.abs(samples["X2"] * n - want["sample"][:, 0]) <= tol["sample"][:, 0]).all()
    assert np.array_equal(samples["expected"] * n, want["sample"][:, 2]) and np.isfinite(samples["z"]).all()
    line = "Fit_samples.csv / Fit_positions.csv written: %d of %d samples and %d of %d positions have z > 3" % (
        int((samples["z"] > 3).sum()), S, int((pos["z"] > 3).sum()), V)
    assert log_check.count(line) == 1 and log_check.count("Fit_cells.csv written") == 1
