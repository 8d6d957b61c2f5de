"""Pair moves of the sampled joint assignment on the device (dsm_assign_tau_sampled_pairs / dsm_ctx_assign_tau_sampled_pairs,
kernels_assign_sampled.hip) against the numpy restatement of tests/_assign_pairs_ref.py and against the exact call.  The parity
tolerances are those stated at the top of tests/test_gpu_assign_sampled.py; every parity input has ``close`` == 0, asserted."""
import os

import numpy as np
import pandas as pd
import pytest

from desman_amd import _lib
from _assign_pairs_ref import MISTAKES, assign_pairs_numpy
from _philox import CTR_SEEDS
from test_gpu_assign_sampled import _case, _parity, _same

pytestmark = pytest.mark.gpu

# (S, G, N, B, T, E, lanes per chain, slots per lane, gamma in chunks, what the case reaches)
SHAPES = [
    (1, 3, 5, 2, 3, 1, 1, 1, False, "LPV = 1, the smallest: 16 positions of a workgroup, 5 used"),
    (3, 2, 6, 2, 3, 3, 4, 1, False, "G = 2: one pair; a padded lane"),
    (5, 1, 7, 2, 3, 1, 8, 1, False, "G = 1: no pairs"),
    (16, 4, 9, 2, 3, 1, 16, 1, False, "4 positions per workgroup, three workgroups, the last with one"),
    (64, 5, 3, 2, 3, 3, 64, 1, False, "LPV = 64, the largest; NSL = 1"),
    (65, 3, 3, 1, 2, 1, 64, 2, False, "NSL = 2"),
    (130, 3, 2, 1, 2, 1, 64, 4, False, "NSL = 4"),
    (300, 4, 2, 1, 2, 1, 64, 8, False, "NSL = 8"),
    (33, 12, 3, 2, 4, 3, 64, 1, False, "a mid case: G = 12, 31 padded lanes"),
    (130, 32, 2, 1, 2, 1, 64, 4, True, "NSL = 4 with gamma staged in chunks; G = 32: 496 pairs, the whole state word"),
    (300, 12, 1, 1, 2, 3, 64, 8, True, "NSL = 8 with gamma staged in chunks; N = 1"),
    (6, 3, 37, 1, 2, 1, 8, 1, False, "N = 37 across workgroup edges (8 positions each) and a launch split into chunks of 16"),
]


@pytest.mark.parametrize("S,G,N,B,T,E,lpv,nsl,chunked,why", SHAPES, ids=["S%d_G%d_N%d_E%d" % (s[0], s[1], s[2], s[5]) for s in SHAPES])
def test_parity_with_the_restatement(S, G, N, B, T, E, lpv, nsl, chunked, why):
    path = _lib.assign_sampled_debug_path(S, G)
    assert (path["lpv"], path["nsl"], path["gamma_chunk"] < G) == (lpv, nsl, chunked), path
    counts, gamma, eta = _case(G, S, N, 5000 + 37 * S + G)
    seed = 0x5EEDC0DE00000002
    ref = assign_pairs_numpy(counts, gamma, eta, seed, B, T, pair_every=E)
    try:
        if N == 37:
            _lib.assign_sampled_debug_set_chunk(16)
        res = _lib.assign_tau_sampled(counts, gamma, eta, seed=seed, burn=B, kept=T, pair_every=E)
    finally:
        _lib.assign_sampled_debug_set_chunk(0)
    _parity(res, ref, T, "S%d G%d N%d E%d" % (S, G, N, E))


def test_without_pairs_the_new_entry_points_are_the_old_ones_bit_for_bit():
    counts, gamma, eta = _case(5, 9, 23, 71)
    lib = _lib.load()
    N, S, G = 23, 9, 5
    g, e = np.ascontiguousarray(gamma), np.ascontiguousarray(eta)

    def outs():
        return dict(map_state=np.zeros((N, G), dtype=np.uint8), map_ll=np.zeros(N), conf=np.zeros(N), marg=np.zeros((N, G, 4)),
                    spread=np.zeros(N), draw_state=np.zeros((N, G), dtype=np.uint8))

    def ptrs(o):
        return [_lib._ptr(o[k]) for k in ("map_state", "map_ll", "conf", "marg", "spread", "draw_state")]
    old, new = outs(), outs()
    _lib.check(lib.dsm_assign_tau_sampled(0, counts, N, S, G, g, e, 11, 2, 5, *ptrs(old)))
    _lib.check(lib.dsm_assign_tau_sampled_pairs(0, counts, N, S, G, g, e, 11, 2, 5, 0, *ptrs(new)))
    assert _same(old, new) and old["marg"].any()
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    try:
        c_old, c_new = outs(), outs()
        _lib.check(lib.dsm_ctx_assign_tau_sampled(ctx._h, g, e, G, 11, 2, 5, *ptrs(c_old)))
        _lib.check(lib.dsm_ctx_assign_tau_sampled_pairs(ctx._h, g, e, G, 11, 2, 5, 0, *ptrs(c_new)))
        assert _same(old, c_old) and _same(old, c_new)
    finally:
        ctx.close()
    assert _same(old, _lib.assign_tau_sampled(counts, gamma, eta, seed=11, burn=2, kept=5))


def test_chunks_context_form_and_reruns_agree_bit_for_bit():
    counts, gamma, eta = _case(5, 9, 23, 71)
    kw = dict(seed=11, burn=2, kept=6, pair_every=2)
    base = _lib.assign_tau_sampled(counts, gamma, eta, **kw)
    assert _same(base, _lib.assign_tau_sampled(counts, gamma, eta, **kw))
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    try:
        assert _same(base, ctx.assign_tau_sampled(gamma, eta, **kw))
        for chunk in (1, 7, 23):
            _lib.assign_sampled_debug_set_chunk(chunk)
            assert _same(base, _lib.assign_tau_sampled(counts, gamma, eta, **kw)), chunk
            assert _same(base, ctx.assign_tau_sampled(gamma, eta, **kw)), chunk
    finally:
        _lib.assign_sampled_debug_set_chunk(0)
        ctx.close()
    assert not np.array_equal(base["draw_state"], _lib.assign_tau_sampled(counts, gamma, eta, seed=11, burn=2, kept=6)["draw_state"])
    assert not np.array_equal(base["draw_state"], _lib.assign_tau_sampled(counts, gamma, eta, seed=11, burn=2, kept=6, pair_every=3)["draw_state"])


@pytest.mark.parametrize("seed", CTR_SEEDS, ids=["%#x" % s for s in CTR_SEEDS])
def test_keying(seed):
    counts, gamma, eta = _case(4, 6, 12, 5)
    B, T, E = 1, 3, 1
    res = _lib.assign_tau_sampled(counts, gamma, eta, seed=seed, burn=B, kept=T, pair_every=E)
    _parity(res, assign_pairs_numpy(counts, gamma, eta, seed, B, T, pair_every=E), T, "seed %#x" % seed)
    for mistake in MISTAKES:
        if mistake == "high key word dropped" and seed >> 32 == 0:
            continue
        wrong = assign_pairs_numpy(counts, gamma, eta, seed, B, T, pair_every=E, mistake=mistake)
        assert not np.array_equal(wrong["draw_state"], res["draw_state"]), mistake


def test_degenerate_operands():
    G, S, N, B, T, E = 4, 5, 12, 1, 3, 1
    counts, gamma, eta = _case(G, S, N, 78)
    gamma[2] = [1.0, 0.0, 0.0, 0.0]                                         # exact zeros in gamma
    counts[0] = 0                                                           # a position without reads
    counts[:, 4] = 0                                                        # a sample without reads
    counts[3] = 0; counts[3, 1] = [2 ** 20 - 3, 2, 0, 0]                    # counts near 2^20
    counts[5][counts[5] == 1] = 0
    ref = assign_pairs_numpy(counts, gamma, eta, 9, B, T, pair_every=E)
    res = _lib.assign_tau_sampled(counts, gamma, eta, seed=9, burn=B, kept=T, pair_every=E)
    _parity(res, ref, T, "edges")
    assert np.array_equal(res["marg"][0], np.full((G, 4), 0.25)) and res["spread"][0] == 0.0 and res["map_ll"][0] == 0.0
    # the identity eta: states inconsistent with an observed base have L = -inf (exact zeros in eta)
    g2 = np.array([[0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.2, 0.3, 0.5]])
    c2 = np.zeros((5, 3, 4), dtype=np.int64)
    c2[1, 0] = [3, 0, 0, 1]
    c2[2, 1] = [1, 1, 0, 0]                                                 # A and C in a sample that is haplotype 0 alone: no state has mass,
    c2[3, 2] = [4, 0, 2, 9]                                                 # all sixteen candidates of every pair step are -inf
    c2[4] = c2[2]; c2[4, 0] = [5, 0, 0, 0]
    ref2 = assign_pairs_numpy(c2, g2, np.eye(4), 3, 2, 4, pair_every=1)
    r2 = _lib.assign_tau_sampled(c2, g2, np.eye(4), seed=3, burn=2, kept=4, pair_every=1)
    _parity(r2, ref2, 4, "identity eta")
    for n in (2, 4):
        assert r2["map_ll"][n] == -np.inf and r2["conf"][n] == 0 and r2["spread"][n] == 0 and not r2["marg"][n].any()
        assert not r2["map_state"][n].any() and not r2["draw_state"][n].any()


def dead_chains_case():
    """S = 300, G = 12 (eight slots per lane, gamma staged in chunks), an eta with exact zeros: base a is read as a (0.9) or as the next
    base (0.1).  Samples 0, 1, 2 are haplotypes 0, 1, 2 alone and read A, which only A and T emit: the chains that start at all A and
    all T are live at every pair step, the chains that start at all C and all G are three sites from any state with mass, so all
    sixteen totals of every pair step of theirs are -inf.  The chains of one workgroup so decide differently at every pair.  (With
    the identity eta the best total is exactly 0, where a relative tolerance on map_ll says nothing.)"""
    _, gamma, _ = _case(12, 300, 1, 321)
    gamma[:3] = np.eye(12)[:3]
    counts = np.zeros((3, 300, 4), dtype=np.int64)
    counts[:, 0] = [5, 0, 0, 0]; counts[:, 1] = [4, 0, 0, 0]; counts[:, 2] = [3, 0, 0, 0]
    counts[1, 7] = [2, 3, 0, 0]
    counts[2, 250] = [6, 0, 0, 0]
    return counts, gamma, 0.9 * np.eye(4) + 0.1 * np.roll(np.eye(4), 1, axis=1)


def test_chains_without_mass_beside_live_ones_where_gamma_is_staged_in_chunks():
    """a pair step whose sixteen totals are all -inf is decided per chain; at eight slots per lane the totals are formed three times
    with gamma staged between barriers, which every chain of the workgroup must reach alike"""
    counts, gamma, eta = dead_chains_case()
    path = _lib.assign_sampled_debug_path(300, 12)
    assert path["nsl"] == 8 and path["gamma_chunk"] < 12
    B, T, E = 1, 2, 1
    ref = assign_pairs_numpy(counts, gamma, eta, 5, B, T, pair_every=E)
    res = _lib.assign_tau_sampled(counts, gamma, eta, seed=5, burn=B, kept=T, pair_every=E)
    _parity(res, ref, T, "dead chains beside live ones")
    assert np.isfinite(res["map_ll"]).all() and (res["map_state"][:, :3] == [0, 0, 0]).all()
    assert (ref["ends"][:, :, 1:3] == np.arange(1, 3)[None, None, :, None]).all()     # (chains 1 and 2 never moved: dead at every step)
    assert (ref["ends"][:, :, 0] != 0).any() and (ref["ends"][:, :, 3] != 3).any()    # (chains 0 and 3 did)
    assert _same(res, _lib.assign_tau_sampled(counts, gamma, eta, seed=5, burn=B, kept=T, pair_every=E))


def test_every_null_combination_of_the_optional_outputs():
    counts, gamma, eta = _case(3, 4, 9, 12)
    kw = dict(seed=4, burn=1, kept=2, pair_every=1)
    full = _lib.assign_tau_sampled(counts, gamma, eta, **kw)
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    try:
        for mask in range(16):
            want = [k for i, k in enumerate(_lib.SAMPLED_OPTIONAL) if mask >> i & 1]
            for got in (_lib.assign_tau_sampled(counts, gamma, eta, want=want, **kw), ctx.assign_tau_sampled(gamma, eta, want=want, **kw)):
                assert set(got) == set(want) | {"map_state", "marg"}
                assert all(got[k].tobytes() == full[k].tobytes() for k in got), want
    finally:
        ctx.close()


def test_every_error_code():
    counts = np.ones((2, 3, 4), dtype=np.int64)
    eta = 0.96 * np.eye(4) + 0.01
    g2 = np.full((3, 2), 0.5)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*pair_every=-1"):
        _lib.assign_tau_sampled(counts, g2, eta, pair_every=-1)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*pair_every = 65537"):
        _lib.assign_tau_sampled(counts, g2, eta, pair_every=65537)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*G=33 exceeds DSM_MAX_G=32"):
        _lib.assign_tau_sampled(counts, np.full((3, 33), 1.0 / 33), eta, pair_every=2)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*S=513"):
        _lib.assign_tau_sampled(np.ones((1, 513, 4), dtype=np.int64), np.full((513, 2), 0.5), eta, pair_every=2)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*kept=0"):
        _lib.assign_tau_sampled(counts, g2, eta, kept=0, pair_every=2)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*burn=-1"):
        _lib.assign_tau_sampled(counts, g2, eta, burn=-1, pair_every=2)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*65537"):
        _lib.assign_tau_sampled(counts, g2, eta, burn=65536, kept=1, pair_every=2)
    bad = counts.copy(); bad[1, 2, 3] = -1
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*count -1 at position 1, sample 2"):
        _lib.assign_tau_sampled(bad, g2, eta, pair_every=2)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*gamma"):
        _lib.assign_tau_sampled(counts, np.array([[0.5, 0.5], [np.inf, 1.0], [0.5, 0.5]]), eta, pair_every=2)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*eta"):
        _lib.assign_tau_sampled(counts, g2, -eta, pair_every=2)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2"):
        _lib.assign_tau_sampled(counts, g2, eta, device=99, pair_every=2)
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*pair_every=-3"):
        ctx.assign_tau_sampled(g2, eta, pair_every=-3)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4"):
        ctx.assign_tau_sampled(np.full((3, 33), 1.0 / 33), eta, pair_every=2)
    assert ctx.assign_tau_sampled(g2, eta, burn=1, kept=1, pair_every=65536, want=())["marg"].shape == (2, 2, 4)   # E at the limit runs
    ctx.close()


def test_pair_passes_do_not_disturb_the_stationary_law():
    """The shape and the bound of test_gpu_assign_sampled.test_marginals_and_conf_follow_the_exact_posterior (G = 6, S = 12, N = 64,
    32 seeds, B = 20, T = 100) with E = 5: per entry of marg, and for conf, |mean over the seeds - exact| <= 5 sd / sqrt(R) + 2 delta."""
    from test_assign_cpu import loglik_at
    G, S, N, R, B, T, E = 6, 12, 64, 32, 20, 100, 5
    counts, gamma, eta = _case(G, S, N, 606, depth=1.0)
    ex = _lib.assign_tau(counts, gamma, eta)
    ctx = _lib.Context(0)
    ctx.set_counts(counts)
    runs = [ctx.assign_tau_sampled(gamma, eta, seed=7000 + k, burn=B, kept=T, pair_every=E) for k in range(R)]
    ctx.close()
    delta = 1e-12 * np.maximum(1.0, np.abs(loglik_at(counts, gamma, eta, ex["map_state"])))
    for key, tol in (("marg", delta[:, None, None]), ("conf", delta)):
        x = np.array([r[key] for r in runs])
        err, sd = np.abs(x.mean(axis=0) - ex[key]), x.std(axis=0, ddof=1)
        z = err / np.maximum(sd / np.sqrt(R), 1e-300)
        bad = err > 5 * sd / np.sqrt(R) + 2 * tol
        print("%s with E = 5: %d of %d entries outside the bound; worst z where sd > 0: %.2f; largest error %.3g"
              % (key, bad.sum(), bad.size, z[sd > 0].max(), err.max()))
        assert not bad.any(), key


def test_pairs_mend_calls_on_the_table_that_traps_single_site_chains():
    """The point of the feature, on the Dirichlet(1) table of test_gpu_assign_sampled (S = 12, G = 8, 240 reads per sample; B = 20,
    T = 100, seed 1), against dsm_assign_tau: the device's wrong calls with E = 5 are the restatement's (parity, close == 0) and
    strictly fewer than those of the same run with E = 0; no wrong call is both unflagged (spread <= 0.1) and confident (conf > 0.75).
    On the identified table all 32 calls stay exact."""
    from test_assign_sampled_cpu import _case as identified_case
    G, S, N, B, T = 8, 12, 32, 20, 100
    counts, gamma, eta = _case(G, S, N, 808, depth=240.0, conc=1.0)
    ex = _lib.assign_tau(counts, gamma, eta)
    ref = assign_pairs_numpy(counts, gamma, eta, 1, B, T, pair_every=5)
    r0 = _lib.assign_tau_sampled(counts, gamma, eta, seed=1, burn=B, kept=T)
    r5 = _lib.assign_tau_sampled(counts, gamma, eta, seed=1, burn=B, kept=T, pair_every=5)
    _parity(r5, ref, T, "trapping table, E = 5")
    w0, w5 = ~(r0["map_state"] == ex["map_state"]).all(axis=1), ~(r5["map_state"] == ex["map_state"]).all(axis=1)
    wref = ~(ref["map_state"] == ex["map_state"]).all(axis=1)
    print("trapping table: wrong calls %d of %d at E = 0, %d at E = 5 (restatement %d); spread > 0.1 at %d (E = 0) and %d (E = 5) positions"
          % (w0.sum(), N, w5.sum(), wref.sum(), (r0["spread"] > 0.1).sum(), (r5["spread"] > 0.1).sum()))
    assert w5.sum() == wref.sum() and w5.sum() < w0.sum()
    assert not (w5 & (r5["spread"] <= 0.1) & (r5["conf"] > 0.75)).any()
    ci, gi, ei = identified_case(G, S, N, 60, 808)
    exi = _lib.assign_tau(ci, gi, ei)
    ri = _lib.assign_tau_sampled(ci, gi, ei, seed=1, burn=B, kept=T, pair_every=5)
    agree = (ri["map_state"] == exi["map_state"]).all(axis=1)
    print("identified table with E = 5: map_state = exact at %d of %d positions" % (agree.sum(), N))
    assert agree.all()


def test_the_polish_ends_on_a_table_whose_pair_ascent_cycles():
    """identical gamma columns: rounding orders the tied permutations differently under each pair, and pair ascent without a bound on
    its rounds cycles (tests/test_assign_pairs_cpu.py has the table).  No parity here -- the input is all ties -- but the call
    returns, twice the same, with the L of the state it reports; so does a table of equal columns at G = 8."""
    from test_assign_cpu import loglik_at
    from test_assign_pairs_cpu import tied_columns_case, trapping_case
    counts, gamma, eta = tied_columns_case()
    a = _lib.assign_tau_sampled(counts, gamma, eta, seed=1, burn=2, kept=4, pair_every=1)
    assert _same(a, _lib.assign_tau_sampled(counts, gamma, eta, seed=1, burn=2, kept=4, pair_every=1))
    L = loglik_at(counts, gamma, eta, a["map_state"])
    assert np.isfinite(a["map_ll"]).all() and (np.abs(a["map_ll"] - L) <= 1e-12 * np.abs(L)).all()
    c8, _, e8 = _case(8, 3, 6, 99, depth=6.0)
    b = _lib.assign_tau_sampled(c8, np.full((3, 8), 0.125), e8, seed=2, burn=1, kept=3, pair_every=1)
    L = loglik_at(c8, np.full((3, 8), 0.125), e8, b["map_state"])
    assert np.isfinite(b["map_ll"]).all() and (np.abs(b["map_ll"] - L) <= 1e-12 * np.abs(L)).all()
    for x, y in zip(trapping_case(), _case(8, 12, 32, 808, depth=240.0, conc=1.0)):     # (the CPU file's copy of the trapping table)
        assert np.array_equal(x, y)


def test_class_method_passes_pair_every():
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    G, S, N = 4, 6, 11
    counts, gamma, eta = _case(G, S, N, 21)
    smp = HaploSNP_Sampler(counts, G, np.random.RandomState(3), max_iter=1)
    smp.gamma_star, smp.eta_star = gamma, eta
    want = _lib.assign_tau_sampled(counts, gamma, eta, seed=77, burn=3, kept=6, pair_every=2)
    got = smp.assignTauSampled(counts.reshape(N, -1), kept=6, burn=3, seed=77, pair_every=2)
    assert np.array_equal(np.argmax(got["tau"], axis=2), want["map_state"]) and np.array_equal(np.argmax(got["draw"], axis=2), want["draw_state"])
    for k in ("map_ll", "conf", "marg", "spread"):
        assert got[k].tobytes() == want[k].tobytes(), k


def test_cli_at_g12(tmp_path):
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
    outs = [str(tmp_path / d) for d in ("plain", "pairs", "again")]
    assign.main([str(run), freq, "-o", outs[0], "--sampled", "100", "--burn", "20", "--seed", "5"])
    got = assign.main([str(run), freq, "-o", outs[1], "--sampled", "100", "--burn", "20", "--seed", "5", "--pairs"])
    assign.main([str(run), freq, "-o", outs[2], "--sampled", "100", "--burn", "20", "--seed", "5", "--pairs"])
    _, g_read, e_read = assign.load_model(str(run))
    assert _same(got, _lib.assign_tau_sampled(counts, g_read, e_read, seed=5, burn=20, kept=100, pair_every=5))
    assert sorted(os.listdir(outs[0])) == sorted(os.listdir(outs[1])) == sorted(os.listdir(outs[2]))
    assert "Assigned_Tau_spread.csv" in os.listdir(outs[1])
    for f in os.listdir(outs[1]):
        assert open(os.path.join(outs[1], f), "rb").read() == open(os.path.join(outs[2], f), "rb").read(), f
    assert open(os.path.join(outs[1], "assign_fit.txt")).read() == "AssignSampled,%d,%d,20,100,%f\n" % (G, N, got["map_ll"].sum())
    star = pd.read_csv(os.path.join(outs[1], "Assigned_Tau_star.csv"), index_col=0)
    assert list(star.columns) == ["Position"] + [str(i) for i in range(4 * G)]
    assert np.array_equal(np.argmax(star.to_numpy()[:, 1:].reshape(N, G, 4), axis=2), got["map_state"])
