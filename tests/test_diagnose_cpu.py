"""Convergence diagnostics, host side (desman_amd/diagnose.py and the HaploSNP_Sampler methods on it), without a GPU: the estimators
against a brute-force restatement from raw series, their behaviour on two-state Markov series of known autocorrelation, R-hat on
agreeing and disagreeing halves and chains (planted traces served by a numpy stand-in context), the library's surface and the command
line's refusals.  The device side is tests/test_gpu_diagnose.py.
"""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
from numpy.random import RandomState

from desman_amd import _lib, diagnose, relabel
from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler


# ---- restatements ------------------------------------------------------------------------------------------------------------------
def batch_stats(x, L):
    """what dsm_ctx_trace_batch_stats returns for 0/1 series x [n, ...]: integers, from the series reshaped into batches"""
    x = np.asarray(x, dtype=np.int64)
    n = x.shape[0]
    B = 2 * (n // (2 * L))
    N = B * L
    x = x[n - N:]
    per = x.reshape((B, L) + x.shape[1:]).sum(axis=1)
    return dict(sum=per.sum(axis=0), first=per[:B // 2].sum(axis=0), bsq=(per * per).sum(axis=0), B=B, N=N, L=L)


def brute(series, L):
    """mean, population sd, mcse, ess and split R-hat of ONE series by the textbook formulas, in Python loops"""
    x = [float(v) for v in series]
    n = len(x)
    B = 2 * (n // (2 * L))
    N = B * L
    x = x[n - N:]
    if B < 2:
        return dict(mean=math.nan, sd=math.nan, mcse=math.nan, ess=math.nan, split_rhat=math.nan)
    m = sum(x) / N
    var0 = sum((v - m) ** 2 for v in x) / N
    bm = [sum(x[b * L:(b + 1) * L]) / L for b in range(B)]
    var_of_mean = sum((v - m) ** 2 for v in bm) / (B - 1) / B           # batch means: the variance of the mean of B batch means
    ess = var0 / var_of_mean if var_of_mean > 0 else float(N)
    h = N // 2
    if h < 2:
        r = math.nan
    else:
        halves = [x[:h], x[h:]]
        mj = [sum(a) / h for a in halves]
        sj = [sum((v - mu) ** 2 for v in a) / (h - 1) for a, mu in zip(halves, mj)]
        W = 0.5 * (sj[0] + sj[1])
        plus = (h - 1.0) / h * W + (mj[0] - mj[1]) ** 2 / 2.0
        r = math.sqrt(plus / W) if W > 0 else (1.0 if mj[0] == mj[1] else math.inf)
    return dict(mean=m, sd=math.sqrt(var0), mcse=math.sqrt(var_of_mean), ess=ess, split_rhat=r)


def _close(got, want, tol=1e-9):
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return abs(got - want) <= tol * max(1.0, abs(want))


def markov(rs, n, V, stay):
    x = np.zeros((n, V), dtype=np.int64)
    x[0] = rs.randint(0, 2, V)
    u = rs.rand(n, V)
    for t in range(1, n):
        x[t] = np.where(u[t] < stay, x[t - 1], 1 - x[t - 1])
    return x


# ---- 1. the estimators against brute force -------------------------------------------------------------------------------------------
def _binary_cases():
    rs = RandomState(7)
    x = markov(rs, 41, 6, 0.8)
    x[:, 1] = 1                                               # constant
    x[:, 2] = 0
    x[:, 3] = np.arange(41) % 2                               # alternating: every even batch holds the same count (sigma2 = 0, p = 1/2)
    return x


@pytest.mark.parametrize("L", [1, 2, 3, 5, 6, 10, 20, 21])
def test_indicator_estimators_against_brute_force(L):
    x = _binary_cases()
    st = batch_stats(x, L)
    assert (st["B"], st["N"]) == diagnose.batch_range(41, L)[:2] and diagnose.batch_range(41, L)[2] == 41 - st["N"]
    if L == 1:
        assert np.array_equal(st["bsq"], st["sum"])
    d = diagnose.tau_diagnostics(st)
    assert d["num"].dtype == np.int64
    for k in range(x.shape[1]):
        want = brute(x[:, k], L)
        assert _close(d["p"][k], want["mean"]) and _close(d["mcse"][k], want["mcse"]), (L, k)
        assert _close(d["ess"][k], want["ess"]) and _close(d["split_rhat"][k], want["split_rhat"]), (L, k, d["ess"][k], want)
    if st["B"] >= 2:
        assert d["num"][1] == 0 and d["ess"][1] == st["N"] and d["mcse"][1] == 0.0 and d["split_rhat"][1] == 1.0      # constant series
        assert d["num"][2] == 0 and d["ess"][2] == st["N"]
    if L in (2, 6, 10, 20):                                   # even batches of the alternating series: sigma2 = 0 exactly, ess = N
        assert d["num"][3] == 0 and d["ess"][3] == st["N"] and d["p"][3] == 0.5
    if L == 3:                                                # ... and odd batches hold 1 or 2 of 3: the batch means vary by 1/6 where
        assert d["ess"][3] > 2 * st["N"]                      # independent draws would give sqrt(1/12): antithetic, ess near 3 N, not capped


def test_skip_rule_and_too_few_batches():
    assert diagnose.batch_range(41, 5) == (8, 40, 1) and diagnose.batch_range(40, 7) == (4, 28, 12) and diagnose.batch_range(7, 3) == (2, 6, 1)
    assert diagnose.batch_range(5, 3) == (0, 0, 5) and diagnose.batch_range(0, 1) == (0, 0, 0)
    with pytest.raises(ValueError):
        diagnose.batch_range(10, 0)
    assert [diagnose.default_batch_len(n) for n in (0, 1, 3, 4, 250, 500, 4000)] == [1, 1, 1, 2, 15, 22, 63]
    x = _binary_cases()
    # the head is skipped: changing it changes nothing
    y = x.copy(); y[:1] = 1 - y[:1]
    a, b = diagnose.tau_diagnostics(batch_stats(x, 5)), diagnose.tau_diagnostics(batch_stats(y, 5))
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("p", "mcse", "ess", "split_rhat"))
    # B < 2: NaN, and no exception
    d = diagnose.tau_diagnostics(dict(sum=np.zeros((3, 2, 4), dtype=np.int64), first=np.zeros((3, 2, 4), dtype=np.int64),
                                      bsq=np.zeros((3, 2, 4), dtype=np.int64), B=0, N=0, L=30))
    assert np.isnan(d["mcse"]).all() and np.isnan(d["ess"]).all() and np.isnan(d["split_rhat"]).all()
    s = diagnose.scalar_diagnostics(np.arange(5.0), 3)
    assert s["B"] == 0 and math.isnan(s["mcse"]) and math.isnan(s["ess"])
    # N = 2: two batches of one iteration; a half of one iteration has no variance
    d = diagnose.tau_diagnostics(batch_stats(np.array([[0, 1], [1, 1]]), 1))
    assert d["B"] == 2 and np.isnan(d["split_rhat"]).all() and d["ess"][1] == 2


def test_cell_summary():
    rs = RandomState(3)
    n, V, G, L = 60, 5, 2, 5
    digits = rs.randint(0, 2, size=(n, V, G))                 # bases 0 and 1 only: bases 2, 3 have p = 0
    digits[:, 0, 0] = 3                                       # a cell that never moves
    x = (digits[..., None] == np.arange(4)).astype(np.int64)
    st = batch_stats(x, L)
    flips = (digits[1:] != digits[:-1]).sum(axis=0)
    d = diagnose.tau_diagnostics(st)
    c = diagnose.cell_summary(d, flips)
    assert c["ess_min"][0, 0] == st["N"] and c["base"][0, 0] == 3 and c["p"][0, 0] == 1.0 and c["rhat_max"][0, 0] == 1.0
    for v in range(V):
        for g in range(G):
            if (v, g) != (0, 0):
                assert c["ess_min"][v, g] == min(d["ess"][v, g, 0], d["ess"][v, g, 1])
                assert c["rhat_max"][v, g] == d["split_rhat"][v, g].max() and c["p"][v, g] == d["p"][v, g].max()
    assert np.array_equal(c["flips"], flips)
    share = diagnose.flagged_share(c)
    assert share == ((c["ess_min"] < 100) | (c["rhat_max"] > 1.1)).mean() and 0.0 <= share <= 1.0


# ---- 2. two-state Markov series: conditions on the estimator ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def markov_series():
    return {stay: markov(RandomState(0), 4000, 400, stay) for stay in (0.5, 0.9)}


@pytest.mark.parametrize("stay,lo,hi", [(0.5, 0.90, 1.15), (0.9, 0.10, 0.14)])
def test_ess_of_two_state_markov_series(markov_series, stay, lo, hi):
    """theory: ess / N = (1 - lam) / (1 + lam), lam = 2 stay - 1: 1 and 0.111; batch means at L = 63 sit slightly above"""
    d = diagnose.tau_diagnostics(batch_stats(markov_series[stay], 63))
    assert (d["B"], d["N"]) == (62, 3906)
    med = float(np.median(d["ess"] / d["N"]))
    print("stay %.1f: median ess / N = %.4f" % (stay, med))
    assert lo <= med <= hi, med


def test_split_rhat_tells_stationary_from_drifting(markov_series):
    for stay in (0.5, 0.9):
        d = diagnose.tau_diagnostics(batch_stats(markov_series[stay], 63))
        med = float(np.median(d["split_rhat"]))
        print("stay %.1f: median split R-hat = %.4f" % (stay, med))
        assert med < 1.05
    rs = RandomState(1)
    x = np.concatenate([rs.rand(2000, 50) < 0.2, rs.rand(2000, 50) < 0.8]).astype(np.int64)
    d = diagnose.tau_diagnostics(batch_stats(x, 50))
    assert d["N"] == 4000 and (d["split_rhat"] > 1.2).all()
    s = diagnose.scalar_diagnostics(x.astype(np.float64), 50)
    assert np.allclose(s["split_rhat"], d["split_rhat"], rtol=1e-9) and np.allclose(s["ess"], d["ess"], rtol=1e-9)
    # halves that are constant: 1 where they agree, inf where they do not
    x = np.zeros((8, 2), dtype=np.int64); x[4:, 1] = 1
    assert diagnose.tau_diagnostics(batch_stats(x, 2))["split_rhat"].tolist() == [1.0, math.inf]


# ---- 3. float series ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [None, 1, 7, 30])
def test_scalar_diagnostics_on_a_planted_ar1_series(L):
    rs = RandomState(5)
    n, K = 203, 4
    x = np.zeros((n, K))
    e = rs.normal(size=(n, K))
    for t in range(1, n):
        x[t] = 0.7 * x[t - 1] + e[t]
    x[:, 3] = 2.5                                             # a constant series
    x += 100.0
    d = diagnose.scalar_diagnostics(x, L)
    Lq = 14 if L is None else L
    assert d["L"] == Lq and (d["B"], d["N"]) == diagnose.batch_range(n, Lq)[:2]
    for k in range(K):
        want = brute(x[:, k], Lq)
        for key in ("mean", "sd", "mcse", "ess", "split_rhat"):
            assert _close(float(d[key][k]), want[key], 1e-7), (L, k, key, d[key][k], want[key])
    assert d["ess"][3] == d["N"] and d["split_rhat"][3] == 1.0
    if Lq == 7:                                               # theory (1 - 0.7) / (1 + 0.7) = 0.18 of N; 28 batches: the estimate of
        assert (d["ess"][:3] < 0.6 * d["N"]).all()           # sigma2 would have to come out at 0.3 of its value to miss this
    one = diagnose.scalar_diagnostics(x[:, 0], L)             # a single series: plain numbers
    assert _close(float(one["mcse"]), float(d["mcse"][0]))


# ---- 4. the sampler's methods and rhat_chains on planted traces, the device calls served by numpy ----------------------------------------
class FakeCtx:
    """what the diagnostics use of _lib.Context, restated in numpy on digits: trace [n, V, G], star [V, G]"""

    def __init__(self, trace, star):
        self.trace, self.star = np.asarray(trace), np.asarray(star)
        self.n_trace, self.V, self.G = self.trace.shape
        self.calls = []

    def set_counts(self, v):
        pass

    def set_priors(self, *a):
        pass

    def trace_snd(self, mode=_lib.SND_STAR, ref=None, it0=0, n_it=None):
        self.calls.append(("snd", mode))
        r = self.star if mode == _lib.SND_STAR else np.asarray(ref)
        return (self.trace[:, :, :, None] != r[None, :, None, :]).sum(axis=1).astype(np.int32)

    def relabelled(self, perm):
        """digits [n, V, G] with label l's digit in column l"""
        t = self.trace
        if perm is None:
            return t
        return np.take_along_axis(t, relabel.inverse(perm)[:, None, :], axis=2)

    def trace_batch_stats(self, batch_len, perm=None, it0=0, n_it=None, want=("sum", "first", "bsq", "flips")):
        self.calls.append(("stats", batch_len, perm is not None))
        d = self.relabelled(perm)
        st = batch_stats((d[..., None] == np.arange(4)).astype(np.int64), batch_len)
        used = d[d.shape[0] - st["N"]:]
        st["flips"] = (used[1:] != used[:-1]).sum(axis=0).astype(np.int32)
        return {k: v for k, v in st.items() if k in want or k in ("B", "N", "L")}


V, S, G, N_IT = 40, 3, 3, 200


def _chain(seed, base, sigma, shift=0.0, flip=0.03):
    """a sampler on a planted trace: base [V, G] under the constant relabelling sigma, ``flip`` of the cells moved per iteration"""
    rs = RandomState(seed)
    trace = np.broadcast_to(base[:, sigma], (N_IT, V, G)).copy()
    moved = rs.random_sample(trace.shape) < flip
    trace = np.where(moved, (trace + rs.randint(1, 4, size=trace.shape)) % 4, trace)
    ctx = FakeCtx(trace, base[:, sigma])
    smp = HaploSNP_Sampler(np.ones((V, S, 4), dtype=np.int64), G, RandomState(1), max_iter=N_IT, ctx=ctx)
    gam = rs.dirichlet(np.array([8.0, 4.0, 2.0]) + shift * np.array([0.0, 6.0, 0.0]), size=(N_IT, S))      # per BASE haplotype
    smp.gamma_store = gam[:, :, sigma]
    smp.lp_store = -1000.0 + rs.normal(size=N_IT) + 20.0 * shift
    smp.ll_store = smp.lp_store + 5.0
    smp.tau_star = HaploSNP_Sampler._onehot(base[:, sigma])
    smp._have_trace = True
    return smp, ctx, trace


def test_sampler_methods_use_the_relabelling_in_force_and_are_kept():
    base = RandomState(2).randint(0, 4, size=(V, G))
    smp, ctx, trace = _chain(11, base, np.array([0, 1, 2]))
    L = 14
    assert diagnose.default_batch_len(N_IT) == L
    mc = smp.tauMCSE()
    assert ctx.calls == [("stats", L, False)]                 # no relabelling was made: identity, one device call
    cells = smp.tauDiagnostics()
    sc = smp.scalarDiagnostics()
    assert ctx.calls == [("stats", L, False)] and smp.tauMCSE() is mc and smp.scalarDiagnostics() is sc
    x = (trace[..., None] == np.arange(4)).astype(np.int64)
    want = diagnose.tau_diagnostics(batch_stats(x, L))
    assert np.array_equal(mc, want["mcse"]) and mc.shape == (V, G, 4)
    assert set(cells) == {"ess_min", "rhat_max", "flips", "base", "p"} and cells["ess_min"].shape == (V, G)
    used = trace[N_IT - want["N"]:]
    assert np.array_equal(cells["flips"], (used[1:] != used[:-1]).sum(axis=0))
    assert np.array_equal(cells["base"], base) and (cells["p"] > 0.9).all()
    assert sc["names"][:2] == ["lp", "ll"] and sc["names"][2:] == ["gamma_%d_%d" % (s, g) for s in range(S) for g in range(G)]
    assert _close(float(sc["mean"][0]), float(smp.lp_store[N_IT - want["N"]:].mean()))
    assert np.allclose(sc["mcse"][2:].reshape(S, G), diagnose.scalar_diagnostics(smp.gamma_store, L)["mcse"])
    assert smp.tauMCSE(5) is not mc and ctx.calls[-1] == ("stats", 5, False)
    # a relabelling in force: the diagnostics are those of the relabelled trace, gamma included
    other = np.ascontiguousarray(base[:, [2, 0, 1]])
    smp.relabel_ref = other
    mc2 = smp.tauMCSE()
    assert ctx.calls[-1] == ("stats", L, True)
    perm = smp.relabelling()["perm"]
    assert (perm == np.array([1, 2, 0])).all()
    assert np.array_equal(mc2, mc[:, [2, 0, 1], :])
    assert np.array_equal(smp.scalarDiagnostics()["mcse"][2:].reshape(S, G), sc["mcse"][2:].reshape(S, G)[:, [2, 0, 1]])
    assert np.array_equal(smp.tauDiagnostics()["base"], other)
    # the next update drops what was kept
    smp._relabel = smp._diag = None
    smp.relabel_ref = None
    assert smp.tauMCSE() is not mc and np.array_equal(smp.tauMCSE(), mc)


def test_rhat_chains_tells_agreeing_from_disagreeing_chains():
    base = RandomState(2).randint(0, 4, size=(V, G))
    sigmas = [np.array([0, 1, 2]), np.array([1, 0, 2]), np.array([2, 0, 1])]
    chains = [_chain(20 + k, base, sigmas[k])[0] for k in range(3)]
    r = diagnose.rhat_chains(chains)
    assert r["m"] == 3 and (r["L"], r["N"]) == (14, 196) and r["tau"].shape == (V, G, 4) and r["gamma"].shape == (S, G)
    assert np.isfinite(r["tau"]).all() and np.median(r["tau"]) < 1.05 and r["tau"].max() < 1.2
    assert r["gamma"].max() < 1.05 and r["lp"] < 1.05
    for c in chains:                                          # every chain went through the given reference: the first chain's MAP haplotypes
        assert [k for k in c._ctx.calls if k[0] == "snd"] == [("snd", _lib.SND_GIVEN)]
        assert c._ctx.calls[-1] == ("stats", 14, True)
    # relabelled to another reference: the same numbers under that reference's labels
    r2 = diagnose.rhat_chains(chains[::-1], ref=base[:, [1, 2, 0]], batch_len=14)
    assert np.allclose(r2["tau"], r["tau"][:, [1, 2, 0], :], rtol=1e-12) and np.allclose(r2["gamma"], r["gamma"][:, [1, 2, 0]], rtol=1e-9)
    # a chain that sits elsewhere: another base at five positions of haplotype 0, other abundances, another lp level
    off = base.copy()
    off[:5, 0] = (off[:5, 0] + 1) % 4
    bad = _chain(31, off, np.array([0, 1, 2]), shift=1.0)[0]
    r3 = diagnose.rhat_chains(chains[:2] + [bad], ref=base)
    hit = np.zeros((V, G, 4), dtype=bool)
    hit[np.arange(5), 0, base[:5, 0]] = True
    hit[np.arange(5), 0, off[:5, 0]] = True
    assert (r3["tau"][hit] > 1.2).all() and np.median(r3["tau"][~hit]) < 1.05
    assert (r3["gamma"][:, 1] > 1.2).all() and r3["lp"] > 1.2
    short = _chain(40, base, sigmas[0])[0]
    short.max_iter = N_IT - 1
    with pytest.raises(ValueError, match="differ in shape"):
        diagnose.rhat_chains([chains[0], short])
    with pytest.raises(ValueError):
        diagnose.rhat_chains(chains[:1])
    with pytest.raises(ValueError, match="fewer than two batches"):
        diagnose.rhat_chains(chains, batch_len=101)


# ---- 5. the library's surface and the command line ---------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_ctx_trace_batch_stats", "dsm_diag_debug_set_parts"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(_lib.Context.trace_batch_stats) and callable(_lib.diag_debug_set_parts)
    assert lib.dsm_ctx_trace_batch_stats(None, None, 0, 0, 1, None, None, None, None) == -2
    assert lib.dsm_diag_debug_set_parts(-1) == -2 and lib.dsm_diag_debug_set_parts(3) == 0 and lib.dsm_diag_debug_set_parts(0) == 0
    assert all(callable(getattr(HaploSNP_Sampler, m)) for m in ("tauMCSE", "tauDiagnostics", "scalarDiagnostics"))


def test_diagnose_is_refused_before_any_chain(tmp_path):
    from desman_amd import cli
    Vn, Sn = 30, 3
    counts = RandomState(3).randint(20, 60, size=(Vn, Sn, 4))
    cols = ["Position"] + ["S%d-%s" % (s, b) for s in range(Sn) for b in "ACGT"]
    df = pd.DataFrame(np.concatenate([(np.arange(Vn) * 5 + 2)[:, None], counts.reshape(Vn, Sn * 4)], axis=1),
                      index=["c%d" % (v // 10) for v in range(Vn)], columns=cols)
    df.index.name = "Contig"
    freq = str(tmp_path / "t.freq")
    df.to_csv(freq)
    out = str(tmp_path / "out")
    base = [freq, "-g", "3", "-m", "0", "-o", out]
    for extra, what in ((["-i", "40", "--diagnose", "0"], "at least 1"), (["-i", "40", "--diagnose", "-2"], "at least 1"),
                        (["-i", "40", "--diagnose", "21"], "40 stored iterations (-i) are fewer than two batches of 21"),
                        (["-i", "1", "--diagnose"], "1 stored iterations (-i) are fewer than two batches of 1"),
                        (["--diagnose", "126"], "250 stored iterations (-i) are fewer than two batches of 126")):
        for run in (cli.main, lambda argv: cli.main_replicates([argv])):
            with pytest.raises(SystemExit) as e:
                run(base + extra)
            assert "--diagnose" in str(e.value) and what in str(e.value), (extra, e.value)
    assert not os.path.exists(out)
    parse = cli.build_parser().parse_args
    assert parse(base).diagnose is None and parse(base + ["--diagnose"]).diagnose is True and parse(base + ["--diagnose", "9"]).diagnose == 9
    assert cli._diagnose_batch_len(parse(base)) is None and cli._diagnose_batch_len(parse(base + ["--diagnose"])) == 15
    assert cli._diagnose_batch_len(parse(base + ["-i", "500", "--diagnose"])) == 22 and cli._diagnose_batch_len(parse(base + ["-i", "40", "--diagnose", "20"])) == 20
