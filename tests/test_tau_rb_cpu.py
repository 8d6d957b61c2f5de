"""Rao-Blackwellised tau marginals (dsm_ctx_trace_rb_marginals, desman --marginals): what can be checked without a
GPU -- the numpy restatement (tests/_tau_rb_ref.py) against an enumerated posterior, the dead-cell rule, the tables of
desman_amd/marginals.py, the symbols, and the refusals made before any device work."""
import itertools
import os
import re

import numpy as np
import pytest

from desman_amd import _lib, marginals
import _tau_rb_ref as R


def test_rows_sum_to_one_and_the_tolerance_is_what_the_design_derives():
    rng = np.random.RandomState(11)
    V, S, G = 9, 5, 4
    x = R.sparse_counts(rng, V, S)
    taus, gammas, etas = R.smooth_trace(rng, 1, V, S, G)
    res = R.conditionals(x, taus[0], gammas[0], etas[0])
    assert np.all(np.isfinite(res["q"])) and np.all(res["q"] >= 0)
    assert np.abs(res["q"].sum(axis=2) - 1.0).max() <= 4 * R.EPS
    assert not res["dead"].any() and res["pmax"] <= 0.85
    # G = 1: the rest is 0, q is the normalised likelihood of the four bases under gamma[:, 0]
    one = R.conditionals(x, taus[0][:, :1], np.ones((S, 1)), etas[0])
    L = (x[:, :, None, :] * np.log(etas[0])[None, None, :, :]).sum(axis=(1, 3))
    want = np.exp(L - L.max(axis=1, keepdims=True))
    assert np.allclose(one["q"][:, 0], want / want.sum(axis=1, keepdims=True), rtol=1e-9, atol=1e-300)
    # K: twice the per-total constant plus ten, in eps
    assert R.k_bound(64, 8) == pytest.approx(2 * (25 / 2 / R.LN_FLOOR + 1 / R.LN_FLOOR + 2 + 256) + 10)


@pytest.fixture(scope="module")
def exact_case():
    """V = 1, S = 2, G = 2, (gamma, eta) fixed: the 16-state posterior of tau (flat prior) enumerated, 4096 draws from it, and the
    restatement's conditionals at every draw"""
    rng = np.random.RandomState(5)
    x = np.array([[[3, 1, 0, 1], [0, 2, 2, 0]]], dtype=np.int64)
    gamma = np.array([[0.7, 0.3], [0.35, 0.65]])
    eta = np.full((4, 4), 0.06) + np.eye(4) * 0.76
    states = np.array(list(itertools.product(range(4), repeat=2)), dtype=np.int64)
    ll = np.empty(16)
    for k, st in enumerate(states):
        p = gamma @ eta[st]                                          # [S, 4]
        ll[k] = (x[0] * np.log(p)).sum()
    post = np.exp(ll - ll.max())
    post /= post.sum()
    exact = np.zeros((2, 4))
    for k, st in enumerate(states):
        for g in range(2):
            exact[g, st[g]] += post[k]
    draws = states[rng.choice(16, size=4096, p=post)]
    by_state = np.stack([R.conditionals(x, st[None, :], gamma, eta)["q"][0] for st in states])      # [16, G, 4]
    idx = draws[:, 0] * 4 + draws[:, 1]
    return dict(exact=exact, draws=draws, q=by_state[idx], post=post, states=states, by_state=by_state)


def test_the_rb_mean_matches_the_exact_marginals(exact_case):
    c = exact_case
    n = c["q"].shape[0]
    mean = c["q"].mean(axis=0)
    se = c["q"].std(axis=0, ddof=1) / np.sqrt(n)
    assert np.all(se > 0)
    assert np.all(np.abs(mean - c["exact"]) <= 6 * se), (mean, c["exact"], se)
    # and exactly, as an identity of the posterior: E[q] over the 16 states is the marginal
    assert np.allclose((c["post"][:, None, None] * c["by_state"]).sum(axis=0), c["exact"], rtol=0, atol=1e-14)


def test_the_rb_variance_is_not_above_the_one_hot_variance(exact_case):
    c = exact_case
    onehot = np.eye(4)[c["draws"]]                                   # [n, G, 4]
    assert np.all(c["q"].var(axis=0) <= onehot.var(axis=0))
    assert np.all(c["q"].var(axis=0) < 0.5 * onehot.var(axis=0))       # here far below: the conditionals barely move between states


def test_a_dead_cell_gives_the_one_hot_of_the_current_base_and_is_counted():
    """eta = the identity, one sample, G = 2.  Position 0 is read as A, C and G at once: with the other haplotype fixed, no base of the
    one being looked at supplies both missing bases -- all four totals are -inf for both haplotypes.  Position 1 is read as A and C
    while the haplotypes are (A, C): each cell has exactly one live base.  Position 2 has no reads: flat."""
    x = np.zeros((3, 1, 4), dtype=np.int64)
    x[0, 0, :3] = (2, 1, 1)
    x[1, 0, :2] = (4, 3)
    tau = np.array([[3, 2], [0, 1], [1, 1]], dtype=np.int64)
    gamma = np.array([[0.5, 0.5]])
    res = R.conditionals(x, tau, gamma, np.eye(4))
    assert res["dead"].tolist() == [[True, True], [False, False], [False, False]]
    assert np.array_equal(res["q"][0], np.eye(4)[[3, 2]]) and np.array_equal(res["q"][1], np.eye(4)[[0, 1]])
    assert np.array_equal(res["q"][2], np.full((2, 4), 0.25))
    assert not np.isnan(res["q"]).any() and res["A"][0].tolist() == [0.0, 0.0]
    m = R.marginals(x, np.stack([tau] * 4), np.stack([gamma] * 4), np.stack([np.eye(4)] * 4), L=1)
    assert m["dead"] == 8 and m["N"] == 4 and np.array_equal(m["sum"][0], 4 * np.eye(4)[[3, 2]])


def test_the_accumulation_follows_the_batch_rule_and_the_labels():
    rng = np.random.RandomState(3)
    qs = rng.dirichlet(np.ones(4), size=(7, 2, 3))                   # [n_it, V, G, 4]
    perm = np.stack([rng.permutation(3) for _ in range(7)])
    s, bsq = R.accumulate(qs, perm, 3)                                # B = 2, the first iteration is skipped
    want = np.zeros((2, 2, 3, 4))
    for t in range(1, 7):
        want[(t - 1) // 3][:, perm[t], :] += qs[t]
    assert np.allclose(s, want.sum(axis=0), rtol=0, atol=1e-15) and np.allclose(bsq, (want ** 2).sum(axis=0), rtol=0, atol=1e-15)
    assert R.batch_range(23, 5) == (4, 20, 3)


def test_the_tables_of_the_marginals_module():
    stats = dict(sum=np.array([[[2.0, 2.0, 0.0, 0.0], [0.4, 3.2, 0.4, 0.0]]]), bsq=np.array([[[2.0, 2.0, 0.0, 0.0], [0.08, 5.12, 0.1, 0.0]]]),
                 dead=3, B=2, N=4, L=2)
    m = marginals.rb_marginals(stats)
    assert np.array_equal(m["p"], stats["sum"] / 4.0) and m["dead"] == 3
    # sigma2 = (B bsq - sum^2) / (B (B - 1) L), clipped at 0; mcse = sqrt(sigma2 / N)
    assert m["mcse"][0, 0].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert m["mcse"][0, 1, 2] == pytest.approx(np.sqrt((2 * 0.1 - 0.16) / 4.0 / 4.0))
    cells = marginals.calls(m["p"], np.array([[1, 1]]))
    assert cells["call"].tolist() == [[0, 1]]                         # a tie goes to the lower base
    assert cells["prob"].tolist() == [[0.5, 0.8]] and cells["star"].tolist() == [[1, 1]] and cells["agree"].tolist() == [[0, 1]]
    assert cells["entropy"][0, 0] == pytest.approx(np.log(2.0)) and np.isfinite(cells["entropy"]).all()
    assert marginals.calls(m["p"], np.eye(4, dtype=np.int64)[[[1, 1]]])["star"].tolist() == [[1, 1]]      # one-hot MAP state
    s = marginals.summary(cells, dead=3)
    assert s == dict(cells=2, expected_wrong=pytest.approx(0.7), low=2, disagree=1, dead=3)
    few = marginals.rb_marginals(dict(sum=stats["sum"], bsq=stats["bsq"], B=0, N=0, L=9))
    assert np.isnan(few["p"]).all() and np.isnan(few["mcse"]).all()


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_ctx_trace_rb_marginals", "dsm_rbtau_debug_path"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(_lib.Context.trace_rb_marginals) and callable(_lib.rbtau_debug_path) and callable(HaploSNP_Sampler.tauMarginals)
    assert lib.dsm_ctx_trace_rb_marginals(None, None, 0, 0, 1, None, None, None) == -2       # (a null context)
    assert _lib.rbtau_debug_path(12, 8) == (16, 1) and _lib.rbtau_debug_path(64, 8) == (32, 2) and _lib.rbtau_debug_path(512, 32) == (64, 8)
    assert _lib.rbtau_debug_path(17, 1) == _lib.pairtau_debug_path(17, 1)              # the sweep's own tiling
    with pytest.raises(_lib.DesmanHipError):
        _lib.rbtau_debug_path(513, 8)
    with pytest.raises(_lib.DesmanHipError):
        _lib.rbtau_debug_path(16, 33)


def test_the_command_line_refuses_what_it_cannot_serve_before_any_chain(tmp_path, monkeypatch):
    from desman_amd import cli

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", boom)
    out = str(tmp_path / "out")
    freq = str(tmp_path / "never_read.freq")                   # the file does not exist: a run that got as far as loading would say so
    with pytest.raises(SystemExit, match=r"--marginals: 1 stored iterations \(-i\) are fewer than two batches of 1"):
        cli.main([freq, "-g", "3", "-o", out, "-i", "1", "--marginals"])
    with pytest.raises(SystemExit, match=r"--marginals: 0 stored iterations"):
        cli.main([freq, "-g", "3", "-o", out, "-i", "0", "--marginals"])
    with pytest.raises(SystemExit, match=r"--marginals: 1 stored iterations"):
        cli.main_replicates([[freq, "-g", "3", "-o", out, "-i", "1", "--marginals"]])
    with pytest.raises(SystemExit, match=r"--diagnose: 40 stored iterations \(-i\) are fewer than two batches of 21"):
        cli.main([freq, "-g", "3", "-o", out, "-i", "40", "--marginals", "--diagnose", "21"])
    assert not os.path.exists(out)
    parse = cli.build_parser().parse_args
    assert parse([freq, "-g", "3"]).marginals is False and cli._marginals_batch_len(parse([freq, "-g", "3"])) is None
    assert cli._marginals_batch_len(parse([freq, "-g", "3", "--marginals"])) == 15                      # floor(sqrt(250))
    assert cli._marginals_batch_len(parse([freq, "-g", "3", "-i", "40", "--marginals"])) == 6
    assert cli._marginals_batch_len(parse([freq, "-g", "3", "-i", "40", "--marginals", "--diagnose"])) == 6
    assert cli._marginals_batch_len(parse([freq, "-g", "3", "-i", "40", "--marginals", "--diagnose", "4", "--relabel", "--check"])) == 4
    assert "--marginals" in cli.build_parser().format_help()
