"""The Rao-Blackwellised joint posterior of two haplotypes' bases (dsm_ctx_trace_rb_pairs, desman --marginal-pairs):
what can be checked without a GPU -- the numpy restatement (tests/_tau_rb_pairs_ref.py) against the single-site conditionals and
against enumerated posteriors, the relabelling with its transposition, the tables of desman_amd/marginals.py (the phase / base
distinction above all), the symbols, and the refusals made before any device work."""
import os
import re

import numpy as np
import pytest

from desman_amd import _lib, marginals
import _tau_rb_ref as R
import _tau_rb_pairs_ref as RP
from test_assign_pairs_cpu import trapping_case


def _smooth(seed, n, V, S, G):
    rng = np.random.RandomState(seed)
    x = R.sparse_counts(rng, V, S, hi=12)
    taus, gammas, etas = R.smooth_trace(rng, n, V, S, G)
    return x, taus, gammas, etas


def test_the_restatement_is_a_distribution_and_the_tolerance_is_what_the_design_derives():
    x, taus, gammas, etas = _smooth(3, 1, 9, 5, 4)
    res = RP.pair_conditionals(x, taus[0], gammas[0], etas[0])
    assert res["q"].shape == (9, 6, 16) and np.all(np.isfinite(res["q"])) and np.all(res["q"] >= 0) and not res["dead"].any()
    assert np.abs(res["q"].sum(axis=2) - 1.0).max() <= 16 * R.EPS
    assert RP.pair_list(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert [RP.pair_index(4, h, g) for g, h in RP.pair_list(4)] == list(range(6))
    assert RP.k_bound(64, 8) == pytest.approx(2 * (17 / R.LN_FLOOR + 1 / R.LN_FLOOR + 2 + 256) + 24)
    # the dead rule: no base of eta's rows supplies what position 0 shows
    eta = np.eye(4)
    x[0] = 0
    x[0, :, 0], x[0, :, 1], x[0, :, 2] = 3, 2, 1                      # three bases seen in every sample: two haplotypes supply two at most
    dead = RP.pair_conditionals(x[:1], np.array([[2, 1]]), gammas[0][:, :2] / gammas[0][:, :2].sum(axis=1, keepdims=True), eta)
    assert dead["dead"].all() and dead["q"][0, 0].tolist() == np.eye(16)[9].tolist() and dead["A"][0, 0] == 0


def test_at_two_haplotypes_the_rows_and_columns_are_the_single_site_conditionals_in_law():
    """G = 2: q is the posterior of (tau_0, tau_1), so by total probability its row sums are the single-site conditional of tau_0 given
    tau_1 = a' (tests/_tau_rb_ref.py: conditionals) weighted by q's own column sums, and the columns likewise.  Every conditional is
    live (a smooth eta: asserted).  Tolerance: the two restatements' own, every term of the identity counted."""
    V, S = 11, 4
    x, taus, gammas, etas = _smooth(8, 1, V, S, 2)
    gamma, eta = gammas[0], etas[0]
    res = RP.pair_conditionals(x, taus[0], gamma, eta)
    assert not res["dead"].any()
    J = res["q"][:, 0].reshape(V, 4, 4)
    tolJ = RP.q_tolerance(res["q"], res["A"], S, 2)[:, 0].reshape(V, 4, 4)
    rows, cols = np.zeros((V, 4)), np.zeros((V, 4))
    tol_r, tol_c = np.zeros((V, 4)), np.zeros((V, 4))
    for other in range(4):
        tau = np.full((V, 2), other, dtype=np.int64)
        single = R.conditionals(x, tau, gamma, eta)
        assert not single["dead"].any()
        ts = R.q_tolerance(single["q"], single["A"], S, 2)
        rows += J.sum(axis=1)[:, other, None] * single["q"][:, 0, :]          # tau_1 = other, weighted by its marginal
        cols += J.sum(axis=2)[:, other, None] * single["q"][:, 1, :]
        tol_r += ts[:, 0, :] + tolJ.sum(axis=1)[:, other, None] + 8 * R.EPS
        tol_c += ts[:, 1, :] + tolJ.sum(axis=2)[:, other, None] + 8 * R.EPS
    assert np.all(np.abs(J.sum(axis=2) - rows) <= tol_r + tolJ.sum(axis=2))
    assert np.all(np.abs(J.sum(axis=1) - cols) <= tol_c + tolJ.sum(axis=1))


def test_at_two_haplotypes_and_constant_parameters_the_mean_is_the_enumerated_posterior():
    """G = 2: the pair conditional does not look at tau at all, so under a constant (gamma, eta) joint / n is the posterior of the
    position, enumerated over its 16 states without anything of pair_candidates (exact_posterior)"""
    V, S, n = 7, 3, 6
    x, taus, gammas, etas = _smooth(21, n, V, S, 2)
    gammas[:], etas[:] = gammas[0], etas[0]
    r = RP.pairs(x, taus, gammas, etas, L=1)
    assert (r["B"], r["N"], r["dead"]) == (6, 6, 0)
    post, digits = RP.exact_posterior(x, gammas[0], etas[0])
    exact = RP.exact_pair_joint(post, digits, 0, 1)
    assert np.all(np.abs(r["joint"][:, 0] / n - exact) <= 2 * r["tol_joint"][:, 0] / n)
    assert np.abs(r["same_batch"].sum(axis=0)[0] / n - np.trace(exact, axis1=1, axis2=2).sum()) <= 2 * r["tol_same"].sum()


def test_a_swap_of_two_labels_is_undone_by_perm_and_the_transposition():
    """every second iteration stores haplotypes 0 and 2 in each other's columns (tau and gamma alike); with the perm that says so, the
    call returns the joint of the unswapped trace -- pair (0, 1) arrives as (2, 1) and is transposed, (0, 2) as (2, 0) likewise"""
    V, S, G, n = 6, 4, 3, 8
    x, taus, gammas, etas = _smooth(34, n, V, S, G)
    want = RP.pairs(x, taus, gammas, etas, L=2)
    sw = np.array([2, 1, 0])
    t2, g2 = taus.copy(), gammas.copy()
    t2[1::2], g2[1::2] = taus[1::2][:, :, sw], gammas[1::2][:, :, sw]
    perm = np.tile(np.arange(G, dtype=np.uint8), (n, 1))
    perm[1::2] = sw
    got = RP.pairs(x, t2, g2, etas, perm=perm, L=2)
    assert np.all(np.abs(got["joint"] - want["joint"]) <= 2 * want["tol_joint"])
    assert np.all(np.abs(got["same_batch"] - want["same_batch"]) <= 2 * want["tol_same"])
    plain = RP.pairs(x, t2, g2, etas, L=2)                            # without the perm the swapped iterations land in the wrong cells
    assert not np.all(np.abs(plain["joint"] - want["joint"]) <= 2 * want["tol_joint"])
    # stride and the batch rule: every third of 8 iterations are 0, 3, 6; with L = 1 the last two of them
    used, B, n_used = RP.used_iterations(8, 3, 1)
    assert used.tolist() == [3, 6] and (B, n_used) == (2, 3)
    third = RP.pairs(x, taus, gammas, etas, L=1, stride=3, res=want["res"])
    assert np.array_equal(third["joint"], RP.pairs(x, taus[[3, 6]], gammas[[3, 6]], etas[[3, 6]], L=1)["joint"])


# ---- phase or base -------------------------------------------------------------------------------------------------------------------
def _exact_draws(post, digits, n, seed):
    rs = np.random.RandomState(seed)
    return np.stack([digits[[rs.choice(post.shape[1], p=post[v]) for v in range(post.shape[0])]] for _ in range(n)])


def _rb_tables(x, gamma, eta, taus):
    n = len(taus)
    r = RP.pairs(x, taus, np.stack([gamma] * n), np.stack([eta] * n), L=1)
    return marginals.pair_tables(marginals.rb_pairs(dict(joint=r["joint"], pairs=RP.pair_list(gamma.shape[1]), B=r["B"], N=r["N"], L=1))["J"])


def _exact_phase(EJ):
    """[V] bool, from an exact pair posterior [V, 4, 4] alone: some unordered {a, a'} has >= 0.9, neither of its orders has"""
    iu = np.triu_indices(4, 1)
    U = (EJ + EJ.transpose(0, 2, 1))[:, iu[0], iu[1]]
    O = np.maximum(EJ, EJ.transpose(0, 2, 1))[:, iu[0], iu[1]]
    return ((U >= 0.9) & (O < 0.9)).any(axis=1)


def phase_case():
    """S = 6, G = 3, V = 24, 120 reads per sample: haplotypes 0 and 1 have abundances within one per cent of each other in every sample,
    so where they carry different bases the data fix the two bases and say next to nothing about their owners"""
    rs = np.random.RandomState(2024)
    S, G, V = 6, 3, 24
    col = rs.dirichlet(np.ones(2), size=S)
    gamma = np.stack([col[:, 0] * 0.5 * (1 + 0.01 * rs.uniform(-1, 1, S)), col[:, 0] * 0.5, col[:, 1]], axis=1)
    gamma /= gamma.sum(axis=1, keepdims=True)
    eta = 0.08 * rs.dirichlet(np.ones(4), size=4) + 0.92 * np.eye(4)
    tau = rs.randint(0, 4, size=(V, G))
    p = np.einsum("sg,ngb->nsb", gamma, eta[tau])
    counts = np.array([[rs.multinomial(rs.poisson(120.0), p[v, s]) for s in range(S)] for v in range(V)], dtype=np.int64)
    return counts, gamma, eta


def one_read_case():
    """S = 2, G = 2, V = 12, one read per sample, each sample nine tenths one haplotype, a noisy eta: both bases are open and nearly
    independent of each other"""
    rs = np.random.RandomState(100)
    gamma = np.array([[0.9, 0.1], [0.1, 0.9]])
    eta = 0.45 * np.eye(4) + 0.55 * rs.dirichlet(np.full(4, 50.0), size=4)
    tau = rs.randint(0, 4, size=(12, 2))
    p = np.einsum("sg,ngb->nsb", gamma, eta[tau])
    counts = np.array([[rs.multinomial(1, p[v, s]) for s in range(2)] for v in range(12)], dtype=np.int64)
    return counts, gamma, eta


def test_phase_and_base_are_told_apart():
    """kind = phase exactly where the exact posterior (enumerated, nothing of the pair restatement) puts >= 0.9 on an unordered swap of
    two haplotypes' bases and on neither order; kind = base where both digits are open and independent.  The trace is 24 independent
    draws from the exact posterior, so the Rao-Blackwellised joint estimates the exact pair posterior.  A reduction that returned the
    product of the single marginals would read 0.5 x 0.5 at a phase cell and call it base (asserted on the table's own joint).

    trapping_case() at its generating (gamma, eta), G = 8: the criterion selects NO position -- with 240 reads per sample the exact
    4^8 posterior of every position has at least 1 - 3e-16 on one state, and the largest unordered mass whose two orders are both
    below 0.9 is 1.2e-16 (both asserted) -- so on that table the check is that every (position, pair) is `base`, and the phase side
    of the distinction is carried by phase_case(), where the same criterion selects 17 of 24 positions for the pair (0, 1)."""
    counts, gamma, eta = trapping_case()
    post, digits = RP.exact_posterior(counts, gamma, eta)
    assert post.shape == (32, 4 ** 8) and post.max(axis=1).min() >= 1 - 1e-12
    tables = _rb_tables(counts, gamma, eta, _exact_draws(post, digits, 4, 1))
    for pi, (g, h) in enumerate(RP.pair_list(8)):
        want = _exact_phase(RP.exact_pair_joint(post, digits, g, h))
        assert not want.any()
        assert np.array_equal(tables["kind"][:, pi] == "phase", want), (g, h)

    counts, gamma, eta = phase_case()
    post, digits = RP.exact_posterior(counts, gamma, eta)
    tables = _rb_tables(counts, gamma, eta, _exact_draws(post, digits, 24, 7))
    n_phase = 0
    for pi, (g, h) in enumerate(RP.pair_list(3)):
        want = _exact_phase(RP.exact_pair_joint(post, digits, g, h))
        n_phase += int(want.sum())
        assert np.array_equal(tables["kind"][:, pi] == "phase", want), (g, h)
        if (g, h) == (0, 1):
            assert want.sum() == 17
            assert np.all(tables["swap"][want, pi] >= 0.9) and np.all(tables["mi"][want, pi] >= 0.6) and np.all(tables["p_same"][want, pi] <= 0.1)
            EJ = RP.exact_pair_joint(post, digits, 0, 1)
            product = EJ.sum(axis=2)[:, :, None] * EJ.sum(axis=1)[:, None, :]
            assert np.all(marginals.pair_tables(product)["kind"][want] == "base")
    assert n_phase == 17

    counts, gamma, eta = one_read_case()
    post, digits = RP.exact_posterior(counts, gamma, eta)
    EJ = RP.exact_pair_joint(post, digits, 0, 1)
    exact = marginals.pair_tables(EJ)
    assert EJ.sum(axis=2).max() < 0.9 and EJ.sum(axis=1).max() < 0.9          # neither digit reaches 0.9 ...
    assert exact["mi"].max() < 0.05                                           # ... and they are next to independent
    tables = _rb_tables(counts, gamma, eta, _exact_draws(post, digits, 4, 3))
    assert np.all(tables["kind"] == "base") and np.all(tables["mi"] < 0.05)


def test_the_tables_of_the_marginals_module():
    J = np.zeros((3, 4, 4))
    J[0, 0, 1], J[0, 1, 0] = 0.55, 0.45                                       # phase: {A, C} certain, the order open
    J[1, 2, 2], J[1, 2, 3] = 0.95, 0.05                                       # a settled pair
    J[2] = np.outer([0.5, 0.5, 0, 0], [0, 0, 0.5, 0.5])                       # two open, independent digits
    t = marginals.pair_tables(J)
    assert t["kind"].tolist() == ["phase", "base", "base"] and t["best"].tolist() == [1, 10, 2]
    assert t["best_prob"].tolist() == [0.55, 0.95, 0.25] and t["p_same"].tolist() == [0.0, 0.95, 0.0]
    assert t["swap"].tolist() == [0.9, 0.0, 0.0] and t["mi"][2] == 0.0
    assert t["mi"][0] == pytest.approx(-(0.55 * np.log(0.55) + 0.45 * np.log(0.45)))
    assert marginals.PHASE_MASS == 0.9 and marginals.PAIR_FLAG_LOW == 0.9
    pairs = np.array(RP.pair_list(3))
    flags = marginals.pair_flags(np.array([[0.95, 0.5, 0.99], [0.91, 0.92, 0.9]]), pairs)
    assert flags.tolist() == [[True, False, True], [False, False, False]]
    assert marginals.star_distance(np.array([[0, 0, 1], [2, 3, 3]]), pairs).tolist() == [1, 2, 1]
    stats = dict(joint=np.stack([J * 4.0, J[::-1] * 4.0], axis=1)[:, :, None].repeat(1, axis=2).reshape(3, 2, 4, 4),
                 same_batch=np.array([[2.0, 1.0], [4.0, 1.0]]), pairs=pairs[:2], dead=2, B=2, N=4, L=2)
    m = marginals.rb_pairs(stats)
    assert np.array_equal(m["J"][:, 0], J) and m["p_same"][:, 0].tolist() == [0.0, 0.95, 0.0] and m["differ"].tolist() == [2 / 3, 2 / 3]
    assert m["dist"].tolist() == [3 - 1.5, 3 - 0.5] and m["dist_mcse"].tolist() == [pytest.approx(np.sqrt(0.5) / np.sqrt(2)), 0.0]
    few = marginals.rb_pairs(dict(stats, B=0, N=0))
    assert np.isnan(few["J"]).all() and np.isnan(few["dist"]).all()
    # the bare flag's stride: about 50 iterations, never fewer than two batches
    assert [marginals.pairs_stride(n, L) for n, L in ((250, 15), (40, 6), (1000, 31), (1000, 5), (10, 1))] == [5, 1, 16, 20, 1]
    assert all(-(-n // marginals.pairs_stride(n, L)) >= min(n, max(50, 2 * L)) for n in range(1, 400) for L in (1, 7, 40))


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    from desman_amd.Output_Results import Output_Results
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_ctx_trace_rb_pairs", "dsm_rbpair_debug_path", "dsm_rbpair_debug_set_chunk"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(_lib.Context.trace_rb_pairs) and callable(_lib.rbpair_debug_path) and callable(_lib.rbpair_debug_set_chunk)
    assert callable(HaploSNP_Sampler.tauPairs) and callable(Output_Results.output_Tau_pairs)
    assert lib.dsm_ctx_trace_rb_pairs(None, None, 0, 0, 1, 1, None, None, None) == -2 and lib.dsm_last_error().decode() == "null context"
    assert _lib.rbpair_debug_path(12, 8) == (16, 1) and _lib.rbpair_debug_path(64, 8) == (32, 2) and _lib.rbpair_debug_path(512, 32) == (64, 8)
    assert all(_lib.rbpair_debug_path(S, 2) == _lib.pairtau_debug_path(S, 2) for S in range(1, 513))    # the pair pass's own tiling
    with pytest.raises(_lib.DesmanHipError):
        _lib.rbpair_debug_path(513, 8)
    with pytest.raises(_lib.DesmanHipError):
        _lib.rbpair_debug_path(16, 33)
    try:
        assert lib.dsm_rbpair_debug_set_chunk(-1) == -2 and lib.dsm_last_error().decode() == "rbpair: chunk -1"
        _lib.rbpair_debug_set_chunk(7)
    finally:
        _lib.rbpair_debug_set_chunk(0)


def test_the_command_line_refuses_what_it_cannot_serve_before_any_chain(tmp_path, monkeypatch):
    from desman_amd import cli

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", boom)
    out = str(tmp_path / "out")
    freq = str(tmp_path / "never_read.freq")                   # the file does not exist: a run that got as far as loading would say so
    for run in (cli.main, lambda argv: cli.main_replicates([argv])):
        with pytest.raises(SystemExit, match=r"--marginal-pairs: a pair needs two haplotypes; got -g 1"):
            run([freq, "-g", "1", "-o", out, "-i", "40", "--marginal-pairs"])
        with pytest.raises(SystemExit, match=r"--marginal-pairs: every K-th stored iteration needs K >= 1; got 0"):
            run([freq, "-g", "3", "-o", out, "-i", "40", "--marginal-pairs", "0"])
        with pytest.raises(SystemExit, match=r"--marginal-pairs: every K-th stored iteration needs K >= 1; got -3"):
            run([freq, "-g", "3", "-o", out, "-i", "40", "--marginals", "--marginal-pairs", "-3"])
        with pytest.raises(SystemExit, match=r"--marginal-pairs: every 4-th of 40 stored iterations \(-i\) are fewer than two batches of 6"):
            run([freq, "-g", "3", "-o", out, "-i", "40", "--marginal-pairs", "4"])
        # where --marginals is refused, so is the flag that implies it, with --marginals' words
        with pytest.raises(SystemExit, match=r"--marginals: 1 stored iterations \(-i\) are fewer than two batches of 1"):
            run([freq, "-g", "3", "-o", out, "-i", "1", "--marginal-pairs"])
        with pytest.raises(SystemExit, match=r"--diagnose: 40 stored iterations \(-i\) are fewer than two batches of 21"):
            run([freq, "-g", "3", "-o", out, "-i", "40", "--marginal-pairs", "--diagnose", "21"])
    assert not os.path.exists(out)
    parse = cli.build_parser().parse_args
    off = parse([freq, "-g", "3", "--marginals"])
    assert off.marginal_pairs is None and cli._marginal_pairs_stride(off) is None
    assert cli._marginals_batch_len(parse([freq, "-g", "3", "-i", "40", "--marginal-pairs"])) == 6             # --marginals is implied
    assert cli._marginal_pairs_stride(parse([freq, "-g", "3", "--marginal-pairs"])) == 5                       # 250 // max(50, 30)
    assert cli._marginal_pairs_stride(parse([freq, "-g", "3", "-i", "1000", "--marginal-pairs", "--diagnose", "5"])) == 20
    assert cli._marginal_pairs_stride(parse([freq, "-g", "3", "-i", "40", "--marginal-pairs", "3"])) == 3      # 14 used >= 12
    assert "--marginal-pairs" in cli.build_parser().format_help()
