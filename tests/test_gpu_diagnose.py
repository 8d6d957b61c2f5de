"""Batch sums of the resident tau trace (dsm_ctx_trace_batch_stats; kernels_diag.hip) and the convergence diagnostics on them, on the
GPU.  Every comparison of the device's integers is exact equality against a numpy restatement built from the planted digits or from
get_tau_at.  The host side alone is tests/test_diagnose_cpu.py.
Run on an MI355X with:  python -m pytest tests/test_gpu_diagnose.py -m gpu
"""
import itertools
import os

import numpy as np
import pandas as pd
import pytest
from numpy.random import RandomState

from desman_amd import _lib, diagnose
from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
from desman_amd.synth import synth_counts, random_state

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = r"error -2: ", r"error -3: "
KEYS = ("sum", "first", "bsq", "flips")


@pytest.fixture()
def ctx():
    c = _lib.Context(0)
    yield c
    _lib.diag_debug_set_parts(0)
    c.close()


def _digits(onehot):
    return np.argmax(onehot, axis=2)


def _want(trace, perm, L):
    """the four outputs from digits trace [n, V, G] (the iterations handed to the call) and perm [n, G] or None"""
    n, V, G = trace.shape
    B = 2 * (n // (2 * L))
    N = B * L
    d = trace
    if perm is not None:
        inv = np.argsort(np.asarray(perm, dtype=np.int64), axis=1)               # inv[t, label] = the haplotype carrying it
        d = np.take_along_axis(trace, inv[:, None, :], axis=2)
    d = d[n - N:]
    per = np.stack([(d == a).reshape(B, L, V, G).sum(axis=1) for a in range(4)], axis=-1).astype(np.int64)     # [B, V, G, 4]
    flips = (d[1:] != d[:-1]).sum(axis=0).astype(np.int32) if N else np.zeros((V, G), dtype=np.int32)
    return dict(sum=per.sum(axis=0), first=per[:B // 2].sum(axis=0), bsq=(per * per).sum(axis=0), flips=flips, B=B, N=N)


def _same(got, want, what):
    assert got["B"] == want["B"] and got["N"] == want["N"], what
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def _load(c, V, G, S=2, seed=0):
    rs = RandomState(1000 + 7 * V + G + seed)
    c.set_counts(rs.randint(0, 30, size=(V, S, 4)).astype(np.int64))
    tau, gamma, eta = random_state(V, S, G, seed=5 + seed)
    c.set_state(tau, gamma, eta)
    return _digits(tau)


# ---- 1. planted traces: every workgroup boundary, every G up to the packing limit, every batch length, every split into parts -----------
@pytest.mark.parametrize("G", [1, 2, 3, 5, 8, 12, 16, 32])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257, 1000])
def test_planted_trace_in_every_split(ctx, V, G):
    """uniform random digits: three of four iterations flip a cell, so a flip missed or counted twice at a part boundary shows"""
    state = _load(ctx, V, G)
    rs = RandomState(V * 100 + G)
    for n in (2, 7, 40):
        trace = rs.randint(0, 4, size=(n, V, G))
        ctx.debug_set_trace(trace)
        perm = np.array([rs.permutation(G) for _ in range(n)])
        for L in sorted({L for L in (1, 2, 3, n // 2) if 2 * L <= n}):
            for p in (None, perm):
                want = _want(trace, p, L)
                for parts in sorted({0, 1, 2, 3, want["B"]}):     # (3 never divides the even B; B = one batch per part)
                    _lib.diag_debug_set_parts(parts)
                    _same(ctx.trace_batch_stats(L, perm=p), want, (n, L, p is not None, parts))
        _lib.diag_debug_set_parts(0)
    assert np.array_equal(_digits(ctx.get_state()[0]), state)


def test_more_parts_than_batches_and_long_batches(ctx):
    V, G, n = 300, 3, 40
    _load(ctx, V, G)
    trace = RandomState(5).randint(0, 4, size=(n, V, G))
    ctx.debug_set_trace(trace)
    for L, parts in ((20, 7), (5, 5), (5, 100000), (6, 4), (13, 2)):
        _lib.diag_debug_set_parts(parts)
        _same(ctx.trace_batch_stats(L), _want(trace, None, L), (L, parts))


# ---- 2. against the existing reductions, sub-ranges, NULL outputs ---------------------------------------------------------------------
def test_against_tau_sum_perm_halves_subranges_and_null_outputs(ctx):
    V, G, n = 257, 5, 40
    _load(ctx, V, G)
    rs = RandomState(77)
    trace = rs.randint(0, 4, size=(n, V, G))
    ctx.debug_set_trace(trace)
    perm = np.array([rs.permutation(G) for _ in range(n)]).astype(np.uint8)
    for it0, n_it, L in ((0, 40, 3), (0, 40, 5), (0, 40, 7), (3, 30, 4), (11, 29, 2), (38, 2, 1), (1, 39, 19)):
        got = ctx.trace_batch_stats(L, perm=perm[it0:it0 + n_it], it0=it0, n_it=n_it)
        _same(got, _want(trace[it0:it0 + n_it], perm[it0:it0 + n_it], L), (it0, n_it, L))
        N, lo = got["N"], it0 + n_it - got["N"]
        assert np.array_equal(got["sum"], ctx.get_tau_sum_perm(perm[lo:lo + N], it0=lo))
        # the second half as a range of its own: its sum is what `first` leaves of `sum`
        h = N // 2
        if h % (2 * L) == 0:                                   # (a half that is itself an even number of batches: nothing of it is skipped)
            second = ctx.trace_batch_stats(L, perm=perm[lo + h:lo + N], it0=lo + h, n_it=h)
            assert second["N"] == h and np.array_equal(got["first"] + second["sum"], got["sum"])
        assert np.array_equal(got["first"], ctx.get_tau_sum_perm(perm[lo:lo + h], it0=lo))
    full = ctx.trace_batch_stats(3, perm=perm)
    for r in range(len(KEYS) + 1):
        for want in itertools.combinations(KEYS, r):
            part = ctx.trace_batch_stats(3, perm=perm, want=want)
            assert set(part) == set(want) | {"B", "N", "L"} and all(np.array_equal(part[k], full[k]) for k in want), want
    ident = np.tile(np.arange(G, dtype=np.uint8), (n, 1))
    _same(ctx.trace_batch_stats(3, perm=ident), ctx.trace_batch_stats(3), "identity rows")
    # n_it = 0: success, zeros
    z = ctx.trace_batch_stats(5, it0=17, n_it=0)
    assert (z["B"], z["N"]) == (0, 0) and not any(z[k].any() for k in KEYS)


# ---- 3. a fixed-tau trace ---------------------------------------------------------------------------------------------------------------
def test_fixed_tau_trace(ctx):
    V, S, G, n = 150, 8, 4, 9
    counts, _, _ = synth_counts(V, S, G, seed=41)
    tau, gamma, eta = random_state(V, S, G, seed=42)
    ctx.set_counts(counts); ctx.set_state(tau, gamma, eta); ctx.seed(5, ctr_seed=99)
    ctx.gibbs_update_fixed_tau(n, pool=0)
    for L, parts in ((1, 0), (2, 0), (2, 2), (4, 2), (3, 3)):
        _lib.diag_debug_set_parts(parts)
        got = ctx.trace_batch_stats(L)
        B, N = got["B"], got["N"]
        assert (B, N) == diagnose.batch_range(n, L)[:2]
        assert not got["flips"].any()
        assert np.array_equal(got["sum"], N * tau) and np.array_equal(got["first"], N // 2 * tau) and np.array_equal(got["bsq"], B * L * L * tau)
    _lib.diag_debug_set_parts(0)
    rev = np.tile(np.arange(G, dtype=np.uint8)[::-1], (n, 1))
    got = ctx.trace_batch_stats(2, perm=rev[:6], it0=3, n_it=6)
    assert np.array_equal(got["sum"], 4 * tau[:, ::-1]) and not got["flips"].any()
    swap = rev.copy(); swap[1::2] = np.arange(G)              # the labels alternate between two relabellings: the flips are those of the labels
    held = _digits(tau)
    want = _want(np.broadcast_to(held, (n, V, G)), swap, 2)
    _same(ctx.trace_batch_stats(2, perm=swap), want, "alternating relabelling")
    assert np.array_equal(want["flips"], 7 * (held != held[:, ::-1]))


# ---- 4. a real chain: against get_tau_at, repeatable, and the chain goes on bit for bit ---------------------------------------------------
def _chain(c, counts, tau, gamma, eta, n):
    c.set_counts(counts); c.set_state(tau, gamma, eta); c.seed(4321, ctr_seed=0xABCDEF12345)
    c.set_tau_rng(_lib.RNG_MT19937)
    c.gibbs_update(n)


def test_real_chain_and_bitwise_continuation(ctx):
    V, S, G, n = 130, 6, 3, 12
    counts, _, _ = synth_counts(V, S, G, seed=31)
    tau, gamma, eta = random_state(V, S, G, seed=32)
    twin = _lib.Context(0)
    try:
        _chain(ctx, counts, tau, gamma, eta, n)
        _chain(twin, counts, tau, gamma, eta, n)
        trace = np.stack([_digits(ctx.get_tau_at(t)) for t in range(n)])
        perm = np.array([RandomState(t).permutation(G) for t in range(n)])
        for L, p, parts in ((1, None, 0), (2, None, 3), (3, perm, 0), (3, perm, 4), (5, perm, 2), (6, None, 2)):
            _lib.diag_debug_set_parts(parts)
            got = ctx.trace_batch_stats(L, perm=p)
            _same(got, _want(trace, p, L), (L, parts))
            again = ctx.trace_batch_stats(L, perm=p)
            assert all(again[k].tobytes() == got[k].tobytes() for k in KEYS)
        _lib.diag_debug_set_parts(0)
        assert np.array_equal(ctx.trace_batch_stats(1)["sum"], ctx.get_tau_sum())
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
        assert np.array_equal(ctx.get_mt_state(), twin.get_mt_state()) and ctx.counters() == twin.counters()
    finally:
        twin.close()


# ---- 5. error codes -------------------------------------------------------------------------------------------------------------------
def test_error_codes_leave_the_context_usable(ctx):
    V, G, n = 70, 3, 6
    _load(ctx, V, G)
    for call in (lambda: ctx.trace_batch_stats(1, it0=0, n_it=0), lambda: ctx.trace_batch_stats(1, it0=0, n_it=2)):
        with pytest.raises(_lib.DesmanHipError, match=ERR_STATE + ".*no update has run"):
            call()
    trace = RandomState(8).randint(0, 4, size=(n, V, G))
    ctx.debug_set_trace(trace)
    want = _want(trace, None, 2)
    ident = np.tile(np.arange(G, dtype=np.uint8), (n, 1))
    dup = ident.copy(); dup[5] = (0, 0, 1)
    big = ident.copy(); big[0] = (0, 1, 3)                    # row 0 is a skipped iteration at L = 2 (B = 2, N = 4): validated all the same
    cases = [lambda: ctx.trace_batch_stats(1, it0=-1, n_it=2), lambda: ctx.trace_batch_stats(1, it0=5, n_it=2),
             lambda: ctx.trace_batch_stats(1, it0=7, n_it=0), lambda: ctx.trace_batch_stats(1, it0=0, n_it=-1),
             lambda: ctx.trace_batch_stats(0), lambda: ctx.trace_batch_stats(-3), lambda: ctx.trace_batch_stats(0, n_it=0),
             lambda: ctx.trace_batch_stats(4), lambda: ctx.trace_batch_stats(2, it0=3, n_it=3), lambda: ctx.trace_batch_stats(2 ** 30),
             lambda: ctx.trace_batch_stats(1, it0=2, n_it=1),
             lambda: ctx.trace_batch_stats(2, perm=dup), lambda: ctx.trace_batch_stats(2, perm=big)]
    for k, call in enumerate(cases):
        with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
            call()
        _same(ctx.trace_batch_stats(2), want, k)
    with pytest.raises(ValueError):
        ctx.trace_batch_stats(2, perm=ident[:5])
    assert ctx.lib.dsm_ctx_trace_batch_stats(ctx._h, None, 0, n, 3, None, None, None, None) == 0       # every output NULL
    z = ctx.trace_batch_stats(2 ** 30, it0=n, n_it=0)         # n_it = 0: a successful no-op anywhere in 0 .. n, whatever L >= 1
    assert z["N"] == 0 and not any(z[k].any() for k in KEYS)
    with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
        _lib.diag_debug_set_parts(-1)
    _same(ctx.trace_batch_stats(2), want, "after all")


# ---- 6. replicate chains -----------------------------------------------------------------------------------------------------------------
def test_rhat_chains_on_batched_replicates():
    """shapes, no NaN and invariance to the order of the chains under one reference: no statistical threshold on a real chain.  (A tau
    cell that no chain ever moves but on which the chains differ has W = 0 and R-hat = inf by definition: inf is allowed, NaN is not.)"""
    V, S, G, n = 90, 6, 3, 40
    counts, _, _ = synth_counts(V, S, G, seed=61)
    chains = []
    for k in range(3):
        s = HaploSNP_Sampler(counts, G, RandomState(300 + k), max_iter=n)
        s.mt_state = _lib.mt_seed_state(900 + k)
        chains.append(s)
    HaploSNP_Sampler.update_batch(chains)
    r = diagnose.rhat_chains(chains)
    assert (r["m"], r["L"], r["N"]) == (3, 6, 36) and r["tau"].shape == (V, G, 4) and r["gamma"].shape == (S, G)
    assert not np.isnan(r["tau"]).any() and (r["tau"] > 0).all() and np.isfinite(r["gamma"]).all() and np.isfinite(r["lp"])
    ref = chains[0].tau_star
    for order in ((2, 1, 0), (1, 2, 0)):
        q = diagnose.rhat_chains([chains[k] for k in order], ref=ref)
        assert np.allclose(q["tau"], r["tau"], rtol=1e-12, atol=0) and np.allclose(q["gamma"], r["gamma"], rtol=1e-9, atol=0)
        assert abs(q["lp"] - r["lp"]) <= 1e-9 * r["lp"]
    d = chains[1].tauDiagnostics(5)
    assert d["ess_min"].shape == (V, G) and d["flips"].dtype == np.int32 and (d["flips"] <= 39).all()
    with pytest.raises(ValueError, match="differ in shape"):
        other = HaploSNP_Sampler(counts[:50], G, RandomState(1), max_iter=n)
        diagnose.rhat_chains([chains[0], other])


# ---- 7. command line -------------------------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_desman_diagnose(tmp_path, caplog, monkeypatch):
    import logging
    from desman_amd import cli
    caplog.set_level(logging.INFO)
    V, S, G, n = 240, 12, 3, 40
    counts, _, _ = synth_counts(V, S, G, seed=123)
    freq = str(tmp_path / "fit.freq")
    names = ["S%d" % s for s in range(S)]
    _write_freq(freq, counts, names, ["contig%d" % (v // 50) for v in range(V)], np.arange(V) * 7 + 3)
    seen = []
    report_diagnose = cli._report_diagnose

    def keep(report, chain, L):
        seen.append((chain, L, chain.relabel_ref is not None or chain._relabel is not None))
        report_diagnose(report, chain, L)
    monkeypatch.setattr(cli, "_report_diagnose", keep)
    plain, diag, rel, both = (str(tmp_path / d) for d in ("plain", "diag", "rel", "both"))
    args = [freq, "-g", str(G), "-i", str(n), "-s", "7"]
    cli.main(args + ["-o", plain])
    cli.main(args + ["-o", rel, "--relabel"])
    assert not seen
    caplog.clear()
    cli.main(args + ["-o", diag, "--diagnose"])
    log_diag = caplog.text
    cli.main(args + ["-o", both, "--relabel", "--diagnose", "4"])
    assert [(L, r) for _, L, r in seen] == [(6, False), (4, True)]
    new = ["Tau_MCSE.csv", "Tau_diag.csv", "Diag_scalars.csv"]
    assert sorted(os.listdir(diag)) == sorted(os.listdir(plain) + new) and sorted(os.listdir(both)) == sorted(os.listdir(rel) + new)
    read = lambda d, name: open(os.path.join(d, name), "rb").read()
    for a, b in ((plain, diag), (rel, both)):                  # the usual files do not change
        for name in os.listdir(a):
            if name != "log_file.txt":
                assert read(a, name) == read(b, name), name
    for d, (chain, L, relabelled) in zip((diag, both), seen):
        Gk = chain.G
        mc = pd.read_csv(os.path.join(d, "Tau_MCSE.csv"), index_col=0, float_precision="round_trip")
        mean_name = "Tau_Mean_relabelled.csv" if relabelled else "Tau_Mean.csv"
        assert list(mc.columns) == list(pd.read_csv(os.path.join(d, mean_name), index_col=0).columns) and mc.shape == (V, 1 + 4 * Gk)
        assert list(mc.index) == ["contig%d" % (v // 50) for v in range(V)] and np.array_equal(mc["Position"], np.arange(V) * 7 + 3)
        want = chain.tauMCSE(L)
        assert want.shape == (V, Gk, 4) and np.array_equal(mc.to_numpy()[:, 1:].reshape(V, Gk, 4), want)
        # the error belongs to the mean next to it: zero exactly where that mean is 0 or 1 in every batch
        mean = pd.read_csv(os.path.join(d, mean_name), index_col=0).to_numpy()[:, 1:].reshape(V, Gk, 4)
        if 2 * (n // (2 * L)) * L == n:
            assert (want[(mean == 0) | (mean == 1)] == 0).all()
        td = pd.read_csv(os.path.join(d, "Tau_diag.csv"), float_precision="round_trip")
        assert list(td.columns) == ["Contig", "Position"] + [c % g for g in range(Gk) for c in ("ess_min_%d", "rhat_max_%d", "flips_%d")]
        assert len(td) == V and np.array_equal(td["Position"], np.arange(V) * 7 + 3)
        cells = chain.tauDiagnostics(L)
        for g in range(Gk):
            assert np.array_equal(td["ess_min_%d" % g], cells["ess_min"][:, g]) and np.array_equal(td["flips_%d" % g], cells["flips"][:, g])
            assert np.array_equal(td["rhat_max_%d" % g], cells["rhat_max"][:, g])
        ds = pd.read_csv(os.path.join(d, "Diag_scalars.csv"), index_col=0, float_precision="round_trip")
        assert list(ds.columns) == ["mean", "sd", "mcse", "ess", "split_rhat"]
        assert list(ds.index) == ["lp", "ll"] + ["gamma_%s_%d" % (s, g) for s in names for g in range(Gk)]
        sc = chain.scalarDiagnostics(L)
        assert all(np.array_equal(ds[k].to_numpy(), sc[k]) for k in ds.columns)
        gm_name = "Gamma_Mean_relabelled.csv" if relabelled else "Gamma_mean.csv"
        if 2 * (n // (2 * L)) * L == n:                        # nothing skipped: the means are those of the file next to it
            gm = pd.read_csv(os.path.join(d, gm_name), index_col=0).to_numpy()
            assert np.allclose(ds["mean"].to_numpy()[2:].reshape(S, Gk), gm, rtol=0, atol=1e-12)
    share = diagnose.flagged_share(seen[0][0].tauDiagnostics(6))
    line = "Tau_diag.csv written: %.2f %% of %d (position, haplotype) cells have ess_min < 100 or rhat_max > 1.1" % (100.0 * share, V * seen[0][0].G)
    assert log_diag.count(line) == 1 and log_diag.count("Tau_MCSE.csv written") == 1 and log_diag.count("Diag_scalars.csv written") == 1
