"""Pair moves of the sampled joint assignment (dsm_assign_tau_sampled_pairs, desman-assign --sampled --pairs): what can be checked
without a GPU -- the numpy restatement (tests/_assign_pairs_ref.py) against the restatement without pairs, against the exact joint
posterior at G = 2 and against the exact MAP states of the table that traps single-site chains; the command line; the symbols."""
import re

import numpy as np
import pytest

from desman_amd import _lib
from _assign_pairs_ref import MISTAKES, assign_pairs_numpy, pair_candidates
from _assign_sampled_ref import assign_sampled_numpy
from test_assign_cpu import _freq, _run_dir, assign_numpy, loglik_at

R = 32


def trapping_case():
    """(counts, gamma, eta) of the table that traps single-site chains: G = 8, S = 12, N = 32, Dirichlet(1) abundances, 240 reads per
    sample, generator seed 808 -- the draws of test_gpu_assign_sampled._case(8, 12, 32, 808, depth=240, conc=1), restated here so
    that this file needs nothing of a GPU test's (tests/test_gpu_assign_pairs.py asserts that the two tables are the same)"""
    G, S, N = 8, 12, 32
    rs = np.random.RandomState(808)
    gamma = rs.dirichlet(np.full(G, 1.0), size=S)
    eta = 0.08 * rs.dirichlet(np.ones(4), size=4) + 0.92 * np.eye(4)
    tau = rs.randint(0, 4, size=(N, G))
    p = np.einsum("sg,ngb->nsb", gamma, eta[tau])
    d = rs.poisson(240.0, size=(N, S))
    counts = np.array([[rs.multinomial(d[n, s], p[n, s] / p[n, s].sum()) for s in range(S)] for n in range(N)], dtype=np.int64)
    return counts, gamma, eta


def tied_columns_case():
    """Five haplotypes with identical gamma columns (S = 2, one position): all permutations of a state tie in the model, and rounding
    orders them differently under each pair's addition tree, so pair ascent without a bound on its rounds cycles among them (here
    (0,1,3,3,2) -> (3,3,0,1,2) -> (1,3,3,0,2) -> and back) while the coordinate ascent in between changes nothing."""
    gamma = np.array([[0.03196178073775709] * 5, [0.1680382192622429] * 5])
    counts = np.array([[[2, 2, 1, 1], [1, 1, 1, 2]]], dtype=np.int64)
    eta = np.array([[0.9406208977385623, 0.017006749312221518, 0.01655567279560716, 0.025816680153609124],
                    [0.014501572940754435, 0.9329171125615121, 0.023394419248320624, 0.029186895249412866],
                    [0.03401258447721449, 0.02488520963735962, 0.9239136243489102, 0.01718858153651569],
                    [0.02456627006423274, 0.028209725158762296, 0.016686591075770068, 0.9305374137012349]])
    return counts, gamma, eta


def test_the_polish_ends_on_a_table_whose_pair_ascent_cycles():
    """the rounds of the polish are bounded: coordinate sweeps and pair passes that changed something number at most 64 together"""
    counts, gamma, eta = tied_columns_case()
    run = assign_pairs_numpy(counts, gamma, eta, 1, 2, 4, pair_every=1)
    assert np.isfinite(run["map_ll"]).all() and run["close"] > 0             # (ties within rounding: no parity input)
    L = loglik_at(counts, gamma, eta, run["map_state"])
    assert (np.abs(run["map_ll"] - L) <= 1e-12 * np.abs(L)).all()


def test_without_pairs_it_is_the_existing_restatement():
    from test_assign_sampled_cpu import _case
    counts, gamma, eta = _case(4, 5, 9, 5, 31)
    counts[2] = 0
    want = assign_sampled_numpy(counts, gamma, eta, 0x1234567800000009, 2, 5)
    got = assign_pairs_numpy(counts, gamma, eta, 0x1234567800000009, 2, 5, pair_every=0)
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k
    other = assign_pairs_numpy(counts, gamma, eta, 0x1234567800000009, 2, 5, pair_every=2)
    assert not np.array_equal(other["ends"], got["ends"])
    for mistake in MISTAKES:
        wrong = assign_pairs_numpy(counts, gamma, eta, 0x1234567800000009, 2, 5, pair_every=2, mistake=mistake)
        assert not np.array_equal(wrong["ends"], other["ends"]), mistake


@pytest.mark.parametrize("S", [1, 3, 6])
def test_a_pair_step_at_two_haplotypes_draws_from_the_exact_joint_posterior(S):
    """G = 2, E = 1: the pair step of every sweep redraws both bases from the joint posterior whatever the state is, so the kept
    end-of-sweep states are draws from it.  Per position and state: |mean over the 32 seeds of the frequency - exact| <= 5 sd / sqrt(R)
    + 2 delta (the z convention of tests/_law.py), the exact posterior by enumeration of the 16 states in numpy.

    The table: a smooth eta (0.4 I + 0.6 Dirichlet(50) rows: no entry near 0) and about three reads per position, so that every one of
    the 16 states has posterior mass above 5e-4 -- asserted.  A state with mass between ~1e-12 and ~1e-4 is never among 32 x 96 draws:
    its frequency is constant over the seeds and off by that mass, which 2 delta cannot absorb (tests/test_assign_sampled_cpu.py:
    MINORS has the same condition).  Worst z: 2.98 (S = 1), 2.61 (S = 3), 3.35 (S = 6)."""
    rs = np.random.RandomState(40 + S)
    N, B, T = 10, 1, 24
    gamma = rs.dirichlet(np.ones(2), size=S)
    eta = 0.6 * rs.dirichlet(np.full(4, 50.0), size=4) + 0.4 * np.eye(4)
    tau = rs.randint(0, 4, size=(N, 2))
    p = np.einsum("sg,ngb->nsb", gamma, eta[tau])
    counts = np.array([[rs.multinomial(rs.poisson(3.0 / S), p[n, s]) for s in range(S)] for n in range(N)], dtype=np.int64)
    L = pair_candidates(counts.astype(np.float64), gamma, eta, np.zeros((N, 1, 2), dtype=np.int64), 0, 1)[:, 0, :]      # all 16 states
    post = np.exp(L - L.max(axis=1, keepdims=True))
    post /= post.sum(axis=1, keepdims=True)
    assert np.allclose(post.reshape(N, 4, 4).sum(axis=2), assign_numpy(counts, gamma, eta)["marg"][:, 0, :], rtol=0, atol=1e-12)
    run = assign_pairs_numpy(counts, gamma, eta, np.arange(R) + 300, B, T, pair_every=1)
    assert run["close"] == 0
    k = 4 * run["ends"][..., 0] + run["ends"][..., 1]                       # [R][N][T][4]
    freq = (k[..., None] == np.arange(16)).mean(axis=(2, 3))                # [R][N][16]
    err, sd = np.abs(freq.mean(axis=0) - post), freq.std(axis=0, ddof=1)
    delta = 1e-12 * run["lscale"].max(axis=0)[:, None]
    bad = err > 5 * sd / np.sqrt(R) + 2 * delta
    z = err[sd > 1e-6] / (sd[sd > 1e-6] / np.sqrt(R))
    print("S = %d: %d of %d state frequencies outside the bound, worst z %.2f, largest error %.3g" % (S, bad.sum(), bad.size, z.max(), err.max()))
    assert post.min() > 5e-4 and (post.max(axis=1) < 0.5).all()             # (conditions on the table: see above)
    assert not bad.any()


def test_pairs_mend_calls_on_the_table_that_traps_single_site_chains():
    """S = 12, G = 8, N = 32, Dirichlet(1) abundances, 240 reads per sample; B = 20, T = 100, seed 1.  Wrong polished calls of the
    restatement against the exact MAP states (numpy enumeration of 4^8 states): E = 5 must have strictly fewer than E = 0.
    Figures of the restatement: 14 wrong at E = 0, see the printed line for E = 5."""
    counts, gamma, eta = trapping_case()
    exact = assign_numpy(counts, gamma, eta)["map_state"]
    wrong = {}
    for E in (0, 5):
        run = assign_pairs_numpy(counts, gamma, eta, 1, 20, 100, pair_every=E)
        assert run["close"] == 0, E
        wrong[E] = int((~(run["map_state"] == exact).all(axis=1)).sum())
    print("trapping table, restatement: %d of 32 calls wrong at E = 0, %d at E = 5" % (wrong[0], wrong[5]))
    assert wrong[5] < wrong[0]


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    import inspect
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_assign_tau_sampled_pairs", "dsm_ctx_assign_tau_sampled_pairs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for fn in (_lib.assign_tau_sampled, _lib.Context.assign_tau_sampled, HaploSNP_Sampler.assignTauSampled):
        assert inspect.signature(fn).parameters["pair_every"].default == 0
    g, e = np.full((1, 2), 0.5), np.eye(4)
    assert lib.dsm_ctx_assign_tau_sampled_pairs(None, g, e, 2, 0, 1, 1, 1, None, None, None, None, None, None) == -2     # (a null context)
    assert _lib.SAMPLED_PAIRS == 5


def test_bad_pair_every_is_refused_before_any_device_work():
    counts = np.ones((2, 3, 4), dtype=np.int64)
    eta, g2 = 0.96 * np.eye(4) + 0.01, np.full((3, 2), 0.5)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*pair_every=-1"):
        _lib.assign_tau_sampled(counts, g2, eta, pair_every=-1)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*pair_every = 65537"):
        _lib.assign_tau_sampled(counts, g2, eta, pair_every=65537)
    with pytest.raises(ValueError):
        _lib.assign_tau_sampled(counts, g2, eta, pair_every=2 ** 31)


def test_cli_arguments(tmp_path, monkeypatch):
    from desman_amd import assign
    run = _run_dir(tmp_path, ["S0", "S1"])
    freq, _ = _freq(tmp_path, ["S0", "S1"])

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", boom)
    seen = {}
    monkeypatch.setattr(_lib, "assign_tau_sampled", lambda *a, **k: seen.update(k) or boom())
    with pytest.raises(SystemExit) as e:
        assign.main([run, freq, "--pairs"])
    assert "--pairs needs --sampled" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        assign.main([run, freq, "--pairs", "3", "--burn", "2"])
    assert "needs --sampled" in str(e.value.code)
    for bad in ("-1", "65537"):
        with pytest.raises(SystemExit) as e:
            assign.main([run, freq, "--sampled", "--pairs", bad])
        assert "0 <= E <= 65536" in str(e.value.code)
    parse = assign.build_parser().parse_args
    assert parse([run, freq, "--sampled"]).pairs is None
    assert parse([run, freq, "--sampled", "--pairs"]).pairs == 5 == assign.SAMPLED_PAIRS == _lib.SAMPLED_PAIRS
    assert parse([run, freq, "--sampled", "30", "--pairs", "7"]).pairs == 7
    for args, want in ((["--sampled"], 0), (["--sampled", "--pairs"], 5), (["--sampled", "--pairs", "0"], 0), (["--sampled", "--pairs", "9"], 9)):
        seen.clear()
        with pytest.raises(AssertionError, match="the library was called"):
            assign.main([run, freq, "-o", str(tmp_path / "o")] + args)
        assert seen["pair_every"] == want, args
    text = assign.build_parser().format_help()
    assert "--pairs" in text and text.count("not tuned") >= 3
