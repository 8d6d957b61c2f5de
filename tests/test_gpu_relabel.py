"""Reductions of the resident tau trace (dsm_ctx_trace_snd, dsm_ctx_get_tau_sum_perm; kernels_relabel.hip) and the label-switch-aware
summaries on them, on the GPU.  Every comparison is exact integer equality against a numpy restatement built from the planted digits
or from get_tau_at / get_star.  The host side alone is tests/test_relabel_cpu.py.
Run on an MI355X with:  python -m pytest tests/test_gpu_relabel.py -m gpu
"""
import itertools
import os

import numpy as np
import pandas as pd
import pytest
from numpy.random import RandomState

from desman_amd import _lib
from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
from desman_amd.synth import synth_counts, random_state

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = r"error -2: ", r"error -3: "


@pytest.fixture()
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _digits(onehot):
    return np.argmax(onehot, axis=2)


def _snd(a, b):
    """[n, G, Gr] from digits a [n, V, G] and b [V, Gr] or [n, V, Gr]"""
    b = np.broadcast_to(b, (a.shape[0],) + b.shape[-2:])
    return (a[:, :, :, None] != b[:, :, None, :]).sum(axis=1).astype(np.int32)


def _tau_sum(trace, perm):
    n, V, G = trace.shape
    out = np.zeros((V, G, 4), dtype=np.int64)
    for t in range(n):
        for g in range(G):
            out[np.arange(V), perm[t, g], trace[t, :, g]] += 1         # (one cell per position: no index repeats within the statement)
    return out


def _load(c, V, G, S=2, seed=0):
    rs = RandomState(1000 + 7 * V + G + seed)
    c.set_counts(rs.randint(0, 30, size=(V, S, 4)).astype(np.int64))
    tau, gamma, eta = random_state(V, S, G, seed=5 + seed)
    c.set_state(tau, gamma, eta)
    return _digits(tau)


# ---- 1. planted traces: every wavefront / workgroup boundary, every G up to the packing limit, the reference tiling ---------------------
@pytest.mark.parametrize("G", [1, 2, 3, 5, 8, 12, 16, 32])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257, 1000])
def test_planted_trace_distances_in_all_modes(ctx, V, G):
    state = _load(ctx, V, G)
    rs = RandomState(V * 100 + G)
    for n in (1, 7, 40):
        trace = rs.randint(0, 4, size=(n, V, G))
        if n == 7:
            trace[3] = state                                   # an iteration equal to the reference: a row of zeros on the diagonal
        ctx.debug_set_trace(trace)
        assert ctx.n_trace == n and np.array_equal(_digits(ctx.get_tau_at(n - 1)), trace[n - 1]) and np.array_equal(_digits(ctx.get_tau_at(-1)), state)
        star = ctx.trace_snd(_lib.SND_STAR)                    # no update has run on this context: the MAP record is the resident state
        assert star.dtype == np.int32 and star.shape == (n, G, G) and np.array_equal(star, _snd(trace, state))
        own = ctx.trace_snd(_lib.SND_SELF)
        assert np.array_equal(own, _snd(trace, trace))
        assert (own[:, np.arange(G), np.arange(G)] == 0).all() and np.array_equal(own, own.transpose(0, 2, 1))
        for Gr in sorted({1, 3, G, 32}):
            ref = rs.randint(0, 4, size=(V, Gr))
            got = ctx.trace_snd(_lib.SND_GIVEN, ref=ref)
            assert got.shape == (n, G, Gr) and np.array_equal(got, _snd(trace, ref)), (n, Gr)
        lo = n // 3
        assert np.array_equal(ctx.trace_snd(_lib.SND_SELF, it0=lo, n_it=n - lo), own[lo:])
        perm = np.array([rs.permutation(G) for _ in range(n)])
        assert np.array_equal(ctx.get_tau_sum_perm(perm), _tau_sum(trace, perm))
    assert np.array_equal(_digits(ctx.get_state()[0]), state)


def test_star_mode_reads_the_slot_the_map_record_names(ctx):
    """after a real update the record names one of the chain's slots; a planted trace then serves that slot's planted row"""
    V, S, G = 130, 6, 3
    counts, _, _ = synth_counts(V, S, G, seed=9)
    tau, gamma, eta = random_state(V, S, G, seed=10)
    ctx.set_counts(counts); ctx.set_state(tau, gamma, eta); ctx.seed(77)
    ctx.gibbs_update(3)
    state = _digits(ctx.get_state()[0])
    trace = RandomState(4).randint(0, 4, size=(9, V, G))
    ctx.debug_set_trace(trace)
    ref = _digits(ctx.get_star()["tau"])
    assert any(np.array_equal(ref, r) for r in [state] + list(trace[:3]))
    assert np.array_equal(ctx.trace_snd(_lib.SND_STAR), _snd(trace, ref))


# ---- 2. planted switches end to end ----------------------------------------------------------------------------------------------------
def test_planted_switches_are_found_and_undone(ctx):
    V, S, G, n = 300, 4, 4, 40
    rs = RandomState(2024)
    base = rs.randint(0, 4, size=(V, G))
    for g, h in itertools.combinations(range(G), 2):
        assert (base[:, g] != base[:, h]).mean() >= 0.5
    sigma = np.tile(np.arange(G), (n, 1))                      # iteration t's haplotype g carries base haplotype sigma[t, g]
    sigma[10:20] = (1, 0, 2, 3)
    sigma[30:40] = (1, 2, 0, 3)
    trace = np.stack([base[:, sigma[t]] for t in range(n)])
    # 5 % of the cells flipped in every iteration: iteration t takes the next V G / 20 cells of one random order of all cells, so over
    # the 40 iterations every cell is flipped exactly twice and carries its base digit in 38 of 40 iterations (0.95 >= 0.9)
    order, per = rs.permutation(V * G), V * G // 20
    for t in range(n):
        cells = order[(np.arange(per) + t * per) % (V * G)]
        v, b = cells // G, cells % G                           # the cell of BASE haplotype b, wherever the iteration holds it
        g = np.argsort(sigma[t])[b]
        trace[t, v, g] = (trace[t, v, g] + rs.randint(1, 4, size=per)) % 4
    d = _snd(trace, base)
    for t in range(n):                                         # the optimum of every iteration is unique (checked here, on the host)
        costs = sorted(int(d[t, np.arange(G), list(p)].sum()) for p in itertools.permutations(range(G)))
        assert costs[0] < costs[1], t
    counts = rs.randint(0, 30, size=(V, S, 4)).astype(np.int64)
    smp = HaploSNP_Sampler(counts, G, RandomState(1), max_iter=n, ctx=ctx)
    _, gamma, eta = random_state(V, S, G, seed=3)
    ctx.set_state(HaploSNP_Sampler._onehot(base), gamma, eta)  # the MAP record of a context without an update: this state
    ctx.debug_set_trace(trace)
    smp.tau_star, smp._have_trace = HaploSNP_Sampler._onehot(base), True
    rel = smp.relabelling()
    assert np.array_equal(rel["perm"], sigma)
    assert np.array_equal(rel["cost_identity"], np.trace(d, axis1=1, axis2=2)) and (rel["cost_best"] == per).all()
    assert np.array_equal(ctx.get_tau_sum_perm(rel["perm"]), _tau_sum(trace, sigma))
    at_base = lambda mean: np.take_along_axis(mean, base[:, :, None], axis=2)[:, :, 0]
    assert at_base(smp.tauMeanRelabelled()).min() >= 0.9
    assert at_base(smp.tauMean()).min() < 0.9 and at_base(smp.tauMean())[:, 3].min() >= 0.9      # label 3 never moved
    st = smp.haplotypeStability()
    assert st["moved"].tolist() == [20, 20, 10, 0] and st["max"].max() <= per / float(V)
    post = smp.sndPosterior()
    assert post["map"].tolist() == [int((base[:, g] != base[:, h]).sum()) for g, h in itertools.combinations(range(G), 2)]
    assert (np.abs(post["mean"] - post["map"]) <= 2 * per).all()


# ---- 3. a real chain: against get_tau_at / get_star, identity and sub-ranges, and the chain goes on bit for bit ---------------------------
def _chain(c, counts, tau, gamma, eta, n):
    c.set_counts(counts); c.set_state(tau, gamma, eta); c.seed(4321, ctr_seed=0xABCDEF12345)
    c.set_tau_rng(_lib.RNG_MT19937)
    c.gibbs_update(n)


def test_real_chain_and_bitwise_continuation(ctx):
    V, S, G, n = 200, 12, 3, 30
    counts, _, _ = synth_counts(V, S, G, seed=31)
    tau, gamma, eta = random_state(V, S, G, seed=32)
    twin = _lib.Context(0)
    try:
        _chain(ctx, counts, tau, gamma, eta, n)
        _chain(twin, counts, tau, gamma, eta, n)
        trace = np.stack([_digits(ctx.get_tau_at(t)) for t in range(n)])
        star = _digits(ctx.get_star()["tau"])
        assert np.array_equal(ctx.trace_snd(_lib.SND_STAR), _snd(trace, star))
        own = ctx.trace_snd(_lib.SND_SELF)
        smp = HaploSNP_Sampler.__new__(HaploSNP_Sampler)
        for t in range(n):
            assert np.array_equal(own[t], smp.calculateSND(ctx.get_tau_at(t)))
        ident = np.tile(np.arange(G), (n, 1))
        full = ctx.get_tau_sum_perm(ident)
        assert np.array_equal(full, ctx.get_tau_sum()) and np.array_equal(full, _tau_sum(trace, ident))
        again = ctx.get_tau_sum_perm(ident)
        assert again.tobytes() == full.tobytes() and ctx.trace_snd(_lib.SND_SELF).tobytes() == own.tobytes()
        parts = [ctx.get_tau_sum_perm(ident[a:b], it0=a) for a, b in ((0, 1), (1, 17), (17, 30))]
        assert np.array_equal(parts[0], _tau_sum(trace[:1], ident[:1])) and np.array_equal(parts[1], _tau_sum(trace[1:17], ident[1:17]))
        assert np.array_equal(parts[0] + parts[1] + parts[2], full)
        perm = np.array([RandomState(t).permutation(G) for t in range(n)])
        assert np.array_equal(ctx.get_tau_sum_perm(perm), _tau_sum(trace, perm))
        assert np.array_equal(ctx.trace_snd(_lib.SND_GIVEN, ref=star[:, :2], it0=5, n_it=10), _snd(trace[5:15], star[:, :2]))
        # nothing of the chain moved: five more iterations equal the twin's, on which none of this was called
        assert np.array_equal(ctx.get_mt_state(), twin.get_mt_state()) and ctx.counters() == twin.counters()
        ctx.gibbs_update(5); twin.gibbs_update(5)
        a, b = ctx.get_trace(), twin.get_trace()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        for x, y in zip(ctx.get_state(), twin.get_state()):
            assert x.tobytes() == y.tobytes()
        sa, sb = ctx.get_star(), twin.get_star()
        assert sa["lp"] == sb["lp"] and sa["it"] == sb["it"] and np.array_equal(sa["tau"], sb["tau"])
        assert np.array_equal(ctx.get_mt_state(), twin.get_mt_state())
    finally:
        twin.close()


def test_fixed_tau_trace(ctx):
    V, S, G, n = 150, 8, 4, 5
    counts, _, _ = synth_counts(V, S, G, seed=41)
    tau, gamma, eta = random_state(V, S, G, seed=42)
    ctx.set_counts(counts); ctx.set_state(tau, gamma, eta); ctx.seed(5, ctr_seed=99)
    ctx.gibbs_update_fixed_tau(n, pool=0)
    held = _digits(tau)
    one = _snd(held[None], held)
    for mode in (_lib.SND_STAR, _lib.SND_SELF):
        got = ctx.trace_snd(mode)
        assert got.shape == (n, G, G) and all(np.array_equal(got[t], one[0]) for t in range(n))
    ref = RandomState(6).randint(0, 4, size=(V, 7))
    assert np.array_equal(ctx.trace_snd(_lib.SND_GIVEN, ref=ref, it0=2, n_it=3), np.repeat(_snd(held[None], ref), 3, axis=0))
    ident = np.tile(np.arange(G), (n, 1))
    assert np.array_equal(ctx.get_tau_sum_perm(ident), n * tau) and np.array_equal(ctx.get_tau_sum_perm(ident), ctx.get_tau_sum())
    rev = ident[:, ::-1]
    assert np.array_equal(ctx.get_tau_sum_perm(rev[:2], it0=3), 2 * tau[:, ::-1])


# ---- 4. error codes -------------------------------------------------------------------------------------------------------------------
def test_error_codes_leave_the_context_usable(ctx):
    V, G = 70, 3
    with pytest.raises(_lib.DesmanHipError, match=ERR_STATE):          # neither counts nor state
        ctx.debug_set_trace(np.zeros((1, 0, 0), dtype=np.int64))
    state = _load(ctx, V, G)
    for call in (lambda: ctx.trace_snd(_lib.SND_SELF, it0=0, n_it=0), lambda: ctx.get_tau_sum_perm(np.zeros((0, G), dtype=np.uint8))):
        with pytest.raises(_lib.DesmanHipError, match=ERR_STATE + ".*no update has run"):
            call()
    trace = RandomState(8).randint(0, 4, size=(6, V, G))
    bad = trace.copy(); bad[4, 69, 2] = 4
    with pytest.raises(_lib.DesmanHipError, match=ERR_ARG + ".*digit 4"):
        ctx.debug_set_trace(bad)
    ctx.debug_set_trace(trace)
    want = _snd(trace, state)
    ident = np.tile(np.arange(G), (6, 1))
    bad_ref = state.copy(); bad_ref[0, 0] = -1
    dup = ident.copy(); dup[5] = (0, 0, 1)
    big = ident.copy(); big[0] = (0, 1, 3)
    cases = [lambda: ctx.trace_snd(_lib.SND_STAR, it0=-1, n_it=2), lambda: ctx.trace_snd(_lib.SND_STAR, it0=5, n_it=2),
             lambda: ctx.trace_snd(_lib.SND_SELF, it0=7, n_it=0), lambda: ctx.trace_snd(_lib.SND_SELF, it0=0, n_it=-1),
             lambda: ctx.trace_snd(3), lambda: ctx.trace_snd(-1),
             lambda: ctx.trace_snd(_lib.SND_GIVEN, ref=np.zeros((V, 0), dtype=np.int64)),
             lambda: ctx.trace_snd(_lib.SND_GIVEN, ref=np.zeros((V, 33), dtype=np.int64)),
             lambda: ctx.trace_snd(_lib.SND_GIVEN, ref=bad_ref),
             lambda: ctx.get_tau_sum_perm(dup), lambda: ctx.get_tau_sum_perm(big), lambda: ctx.get_tau_sum_perm(ident, it0=1),
             lambda: ctx.get_tau_sum_perm(ident[:1], it0=-1)]
    for k, call in enumerate(cases):
        with pytest.raises(_lib.DesmanHipError, match=ERR_ARG):
            call()
        assert np.array_equal(ctx.trace_snd(_lib.SND_STAR), want), k
    assert ctx.lib.dsm_ctx_trace_snd(ctx._h, _lib.SND_STAR, None, 2, 0, 6, None) == -2     # Gr of the chain's own modes: 0 or G
    # n_it = 0: a successful no-op, anywhere in 0 .. n
    assert ctx.trace_snd(_lib.SND_STAR, it0=6, n_it=0).shape == (0, G, G) and ctx.trace_snd(_lib.SND_GIVEN, ref=state, it0=0, n_it=0).shape == (0, G, G)
    assert not ctx.get_tau_sum_perm(np.zeros((0, G), dtype=np.uint8), it0=3).any()
    ctx.debug_set_trace(np.zeros((0, V, G), dtype=np.int64))
    assert ctx.n_trace == 0 and ctx.trace_snd(_lib.SND_SELF).shape == (0, G, G)
    ctx.debug_set_trace(trace)
    assert np.array_equal(ctx.get_tau_sum_perm(ident), _tau_sum(trace, ident)) and np.array_equal(_digits(ctx.get_state()[0]), state)


# ---- 5. command line -------------------------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_desman_relabel(tmp_path, caplog):
    import logging
    from desman_amd import cli
    caplog.set_level(logging.INFO)
    V, S, G, n = 240, 12, 3, 40
    counts, _, _ = synth_counts(V, S, G, seed=123)
    freq = str(tmp_path / "fit.freq")
    _write_freq(freq, counts, ["S%d" % s for s in range(S)], ["contig%d" % (v // 50) for v in range(V)], np.arange(V) * 7 + 3)
    plain, rel, ref = (str(tmp_path / d) for d in ("plain", "rel", "ref"))
    args = [freq, "-g", str(G), "-i", str(n), "-s", "7"]
    cli.main(args + ["-o", plain])
    log_plain = caplog.text
    caplog.clear()
    cli.main(args + ["-o", rel, "--relabel"])
    log_rel = caplog.text
    cli.main(args + ["-o", ref, "--relabel-ref", os.path.join(plain, "Filtered_Tau_star.csv")])
    new = ["Relabel.csv", "Tau_Mean_relabelled.csv", "Gamma_Mean_relabelled.csv", "SND_posterior.csv", "Haplotype_stability.csv"]
    assert sorted(os.listdir(rel)) == sorted(os.listdir(plain) + new) == sorted(os.listdir(ref))
    read = lambda d, name: open(os.path.join(d, name), "rb").read()
    for name in os.listdir(plain):
        if name != "log_file.txt":                             # (time stamps; its lines are compared below)
            assert read(plain, name) == read(rel, name) == read(ref, name), name
    for name in new:                                           # the same chain against its own MAP haplotypes, read back from the file
        assert read(rel, name) == read(ref, name), name
    t = pd.read_csv(os.path.join(rel, "Relabel.csv"))
    Gk = (pd.read_csv(os.path.join(rel, "Filtered_Tau_star.csv"), index_col=0).shape[1] - 1) // 4
    assert list(t.columns) == ["iter", "cost_identity", "cost_best", "switched", "perm"] and t["iter"].tolist() == list(range(n))
    assert (t["cost_best"] <= t["cost_identity"]).all()
    perms = np.array([[int(x) for x in p.split()] for p in t["perm"]])
    assert perms.shape == (n, Gk) and (np.sort(perms, axis=1) == np.arange(Gk)).all()
    assert np.array_equal(t["switched"].to_numpy() != 0, (perms != np.arange(Gk)).any(axis=1))
    tm = pd.read_csv(os.path.join(rel, "Tau_Mean_relabelled.csv"), index_col=0)
    assert list(tm.columns) == list(pd.read_csv(os.path.join(rel, "Tau_Mean.csv"), index_col=0).columns) and tm.shape == (V, 1 + 4 * Gk)
    assert np.allclose(tm.to_numpy()[:, 1:].reshape(V, Gk, 4).sum(axis=2), 1.0, atol=1e-12)
    if not t["switched"].any():
        assert read(rel, "Tau_Mean_relabelled.csv") == read(rel, "Tau_Mean.csv")
    gm = pd.read_csv(os.path.join(rel, "Gamma_Mean_relabelled.csv"), index_col=0)
    assert gm.shape == (S, Gk) and np.allclose(gm.to_numpy().sum(axis=1), 1.0, atol=1e-9)
    sp = pd.read_csv(os.path.join(rel, "SND_posterior.csv"))
    assert list(sp.columns) == ["g", "h", "mean", "sd", "lo", "med", "hi", "map"] and len(sp) == Gk * (Gk - 1) // 2
    assert ((sp["lo"] <= sp["med"]) & (sp["med"] <= sp["hi"])).all()
    hs = pd.read_csv(os.path.join(rel, "Haplotype_stability.csv"))
    assert list(hs.columns) == ["haplotype", "mean_diff", "max_diff", "moved"] and len(hs) == Gk and (hs["mean_diff"] <= hs["max_diff"]).all()
    assert log_rel.count("Relabel.csv written: %d of %d stored iterations had switched labels" % (int(t["switched"].sum()), n)) == 1
    strip = lambda text: [ln for ln in text.splitlines() if "Results created in" not in ln]
    assert "Gibbs sampling" in log_plain and "elabel" not in "\n".join(strip(log_plain))
    assert strip(log_rel)[:len(strip(log_plain))] == strip(log_plain)          # the run's own log lines are what they were
    # a reference that holds the same haplotypes under OTHER labels: every relabelled file follows the reference's labels, and in
    # SND_posterior.csv the MAP distance of a row belongs to the same two strains as the row's posterior columns
    order = np.roll(np.arange(Gk), 1)                          # reference label j = this run's MAP haplotype order[j]
    star = pd.read_csv(os.path.join(plain, "Filtered_Tau_star.csv"), index_col=0)
    blocks = star.to_numpy()[:, 1:].reshape(V, Gk, 4)[:, order, :].reshape(V, 4 * Gk)
    moved = pd.DataFrame(blocks, index=star.index)
    moved.insert(0, "Position", star["Position"].to_numpy())
    moved.to_csv(str(tmp_path / "moved_star.csv"))
    other = str(tmp_path / "other")
    cli.main(args + ["-o", other, "--relabel-ref", str(tmp_path / "moved_star.csv")])
    for name in os.listdir(plain):
        if name != "log_file.txt":
            assert read(plain, name) == read(other, name), name
    tmo = pd.read_csv(os.path.join(other, "Tau_Mean_relabelled.csv"), index_col=0).to_numpy()[:, 1:].reshape(V, Gk, 4)
    assert np.array_equal(tmo, tm.to_numpy()[:, 1:].reshape(V, Gk, 4)[:, order, :])
    gmo = pd.read_csv(os.path.join(other, "Gamma_Mean_relabelled.csv"), index_col=0).to_numpy()
    assert np.array_equal(gmo, gm.to_numpy()[:, order])
    digits = np.argmax(star.to_numpy()[:, 1:].reshape(V, Gk, 4), axis=2)
    spo = pd.read_csv(os.path.join(other, "SND_posterior.csv"))
    own = {(int(r.g), int(r.h)): r for r in sp.itertuples()}
    for r in spo.itertuples():
        a, b = sorted((int(order[int(r.g)]), int(order[int(r.h)])))
        assert r.map == (digits[:, a] != digits[:, b]).sum() == own[(a, b)].map
        assert (r.mean, r.sd, r.lo, r.med, r.hi) == (own[(a, b)].mean, own[(a, b)].sd, own[(a, b)].lo, own[(a, b)].med, own[(a, b)].hi)
