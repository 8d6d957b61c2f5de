"""Sampled joint haplotype assignment (dsm_assign_tau_sampled, desman-assign --sampled): what can be checked without a GPU -- the numpy
restatement of the chain (tests/_assign_sampled_ref.py) against the exact posterior (test_assign_cpu.assign_numpy), the refusals of the
command line and the declared symbols."""
import re

import numpy as np
import pytest

from desman_amd import _lib
from _assign_sampled_ref import assign_sampled_numpy
from test_assign_cpu import _freq, _run_dir, assign_numpy, loglik_at

R = 32                  # seeds
B, T = 8, 24            # burn-in and kept sweeps of the comparisons below


def _case(G, S, N, cell_depth, seed):
    """abundances in which every haplotype dominates some sample (0.8 on haplotype s mod G, the rest Dirichlet), an asymmetric eta,
    4 cell_depth reads per sample on average"""
    rs = np.random.RandomState(seed)
    gamma = 0.8 * np.eye(G)[np.arange(S) % G] + 0.2 * rs.dirichlet(np.ones(G), size=S)
    eta = 0.05 * rs.dirichlet(np.ones(4), size=4) + 0.95 * np.eye(4)
    tau = rs.randint(0, 4, size=(N, G))
    p = np.einsum("sg,ngb->nsb", gamma, eta[tau])
    d = rs.poisson(4 * cell_depth, size=(N, S))
    counts = np.array([[rs.multinomial(d[n, s], p[n, s] / p[n, s].sum()) for s in range(S)] for n in range(N)], dtype=np.int64)
    return counts, gamma, eta


def _mixing_case(G, S, N, cell_depth, minors, seed):
    """A table on which single-site moves reach the whole posterior, so that the chain's law can be held against the exact one:
      * M = G - len(minors) major haplotypes, each with 0.95 of the non-minor abundance in its own samples (s mod M) and a share of
        0.05 elsewhere: a major site's own samples decide its base by hundreds of nats whatever the other sites hold, so no corner
        start is trapped with a major's base on the wrong site (at 0.8 it is: DESIGN.md sec. 8a-2);
      * the last len(minors) haplotypes have abundance minors[k] x U(0.8, 1.2) in every sample: with few reads of their own their
        sites stay open, and a major site never gains by taking their bases."""
    rs = np.random.RandomState(seed)
    M = G - len(minors)
    gamma = np.zeros((S, G))
    for k, m in enumerate(minors):
        gamma[:, M + k] = m * rs.uniform(0.8, 1.2, size=S)
    rest = 1.0 - gamma[:, M:].sum(axis=1)
    gamma[:, :M] = (0.95 * np.eye(M)[np.arange(S) % M] + 0.05 * rs.dirichlet(np.ones(M), size=S)) * rest[:, None]
    eta = 0.05 * rs.dirichlet(np.ones(4), size=4) + 0.95 * np.eye(4)
    tau = rs.randint(0, 4, size=(N, G))
    p = np.einsum("sg,ngb->nsb", gamma, eta[tau])
    d = rs.poisson(4 * cell_depth, size=(N, S))
    counts = np.array([[rs.multinomial(d[n, s], p[n, s] / p[n, s].sum()) for s in range(S)] for n in range(N)], dtype=np.int64)
    return counts, gamma, eta


# cell depth -> abundances of the minor haplotypes.  Open: minors of 0.03 and 0.012 (G = 3: the first only) see 1 - 4 reads of their
# own among a position's 120, so their sites stay open (exact conf 0.13 - 0.9997).  Peaked: one minor of 0.08 sees ~115 of 1440 reads,
# ~230 nats: every conf is 1 to the last bit.  What the choice avoids is posterior mass between ~1e-12 and ~1e-4 on one state: 32 x 96
# kept states cannot see it (the estimate is constant over the seeds) and the 2 delta ~ 1e-9 asked of a constant statistic can; the
# test asserts that the exact conf of its table has no such value.
MINORS = {5: (0.03, 0.012), 60: (0.08,)}
_CACHE = {}


def _runs(G, cell_depth):
    key = (G, cell_depth)
    if key not in _CACHE:
        counts, gamma, eta = _mixing_case(G, 6, 24, cell_depth, MINORS[cell_depth][:G - 2], 100 + G + cell_depth)
        _CACHE[key] = (counts, gamma, eta, assign_numpy(counts, gamma, eta), assign_sampled_numpy(counts, gamma, eta, np.arange(R) + 1000, B, T))
    return _CACHE[key]


def _outside(x, exact, delta):
    """entries whose mean over the seeds is outside 5 sd / sqrt(R) + 2 delta of the exact value, and the worst z where sd > 1e-6"""
    err, sd = np.abs(x.mean(axis=0) - exact), x.std(axis=0, ddof=1)
    bad = err > 5 * sd / np.sqrt(R) + 2 * delta
    big = sd > 1e-6
    z = err[big] / (sd[big] / np.sqrt(R))
    return bad, (float(z.max()) if z.size else 0.0), float(err.max())


@pytest.mark.parametrize("G", [3, 5])
@pytest.mark.parametrize("cell_depth", [5, 60], ids=["open", "peaked"])
def test_restatement_follows_the_exact_posterior(G, cell_depth):
    """G = 3 and 5, S = 6, N = 24, R = 32 seeds; per entry of marg, and for conf: |mean over the seeds - exact| <= 5 sd / sqrt(R) +
    2 delta (the z convention of tests/_law.py); a statistic that is constant over the seeds is thereby held to 2 delta.

    B = 8, T = 24: on these tables (_mixing_case) the major sites settle in the first sweep and the open sites are redrawn from their
    full conditional at every sweep, so 8 sweeps of burn-in are ample (B = 4 gives the same verdict).  Worst z among the statistics
    that vary (sd > 1e-6): open G = 3 conf 2.02 (every marg entry is constant there: largest error 3.3e-15); open G = 5 marg 2.10,
    conf 2.46; peaked: every statistic is constant over the seeds, largest error 1.6e-33 (G = 3) and 2.1e-45 (G = 5) for marg, 0 for conf.
    On tables whose majors are less dominant the chain as specified does not pass: corner starts are trapped in swapped-base local
    maxima whatever B is (0.8 dominance, same shapes: 39 and 16 marg entries outside the bound at G = 3); DESIGN.md sec. 8a-2 has the
    figures and what `spread` does about it."""
    counts, gamma, eta, ex, run = _runs(G, cell_depth)
    assert not ((ex["conf"] > 0.9999) & (ex["conf"] < 1.0 - 1e-12)).any()    # (a condition on the table: see MINORS)
    assert ((ex["conf"] < 0.99).mean() > 0.5) if cell_depth == 5 else (ex["conf"] > 0.999).all()
    delta = 1e-12 * run["lscale"].max(axis=0)
    bad_m, z_m, e_m = _outside(run["marg"], ex["marg"], delta[:, None, None])
    bad_c, z_c, e_c = _outside(run["conf"], ex["conf"], delta)
    print("G = %d, depth %d: marg %d of %d outside (worst z %.3g, largest error %.3g); conf %d of %d outside (worst z %.3g, largest error "
          "%.3g); largest spread %.3f" % (G, cell_depth, bad_m.sum(), bad_m.size, z_m, e_m, bad_c.sum(), bad_c.size, z_c, e_c,
                                          run["spread"].max()))
    assert not bad_m.any() and not bad_c.any()


@pytest.mark.parametrize("G", [3, 5])
def test_map_state_of_the_peaked_case_is_the_exact_one(G):
    counts, gamma, eta, ex, run = _runs(G, 60)
    assert (ex["conf"] > 0.999).all()
    for r in range(R):
        assert np.array_equal(run["map_state"][r], ex["map_state"]), r
        L = loglik_at(counts, gamma, eta, run["map_state"][r])
        assert (np.abs(run["map_ll"][r] - L) <= 1e-12 * np.abs(L)).all()


def test_empty_position():
    counts, gamma, eta = _case(3, 6, 4, 5, 9)                              # (the 0.8-dominance table: any table does here)
    counts[1] = 0
    run = assign_sampled_numpy(counts, gamma, eta, 5, 2, 6)
    assert np.array_equal(run["marg"][1], np.full((3, 4), 0.25)) and run["spread"][1] == 0.0 and run["map_ll"][1] == 0.0
    assert run["conf"][1] == run["conf_count"][1] / 24.0 and 0 <= run["conf_count"][1] <= 24


def test_swapped_bases_come_back_flagged_or_right():
    """two haplotypes with equal gamma columns at depth 200: the states (A, C, x) and (C, A, x) tie exactly, single-site moves do not
    cross between them.  Either the spread says so (>= 0.5) or the marginals are the exact 50 / 50 within the z bound."""
    rs = np.random.RandomState(3)
    S, G, N = 6, 3, 8
    gamma = rs.dirichlet(np.ones(G), size=S)
    gamma[:, 1] = gamma[:, 0]
    gamma /= gamma.sum(axis=1, keepdims=True)
    eta = 0.05 * rs.dirichlet(np.ones(4), size=4) + 0.95 * np.eye(4)
    tau = np.tile(np.array([0, 1, 2]), (N, 1))
    p = np.einsum("sg,ngb->nsb", gamma, eta[tau])
    counts = np.array([[rs.multinomial(800, p[n, s]) for s in range(S)] for n in range(N)], dtype=np.int64)
    ex = assign_numpy(counts, gamma, eta)
    assert (np.abs(ex["marg"][:, 0, :2] - 0.5) < 1e-6).all()
    run = assign_sampled_numpy(counts, gamma, eta, np.arange(R) + 50, B, T)
    delta = 1e-12 * run["lscale"].max(axis=0)
    bad, z, err = _outside(run["marg"], ex["marg"], delta[:, None, None])
    flagged = run["spread"].min(axis=0) >= 0.5
    print("swapped bases: %d of %d positions flagged by spread >= 0.5 at every seed; marg outside the z bound at %d positions"
          % (flagged.sum(), N, bad.any(axis=(1, 2)).sum()))
    assert (flagged | ~bad.any(axis=(1, 2))).all()


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_sampled_call():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_assign_tau_sampled", "dsm_ctx_assign_tau_sampled", "dsm_assign_sampled_debug_set_chunk", "dsm_assign_sampled_debug_path"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    path = _lib.assign_sampled_debug_path(64, 12)                           # launches nothing: runs without a GPU
    assert path == dict(inst=0, lpv=64, nsl=1, gamma_chunk=12, positions_per_workgroup=1)
    assert _lib.assign_sampled_debug_path(300, 12)["gamma_chunk"] == 8
    with pytest.raises(_lib.DesmanHipError, match=r"error -4"):
        _lib.assign_sampled_debug_path(4, 33)


def test_bad_arguments_are_refused_before_any_device_work():
    counts = np.ones((2, 3, 4), dtype=np.int64)
    eta = 0.96 * np.eye(4) + 0.01
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*G=33 exceeds DSM_MAX_G=32"):
        _lib.assign_tau_sampled(counts, np.full((3, 33), 1.0 / 33), eta)
    with pytest.raises(_lib.DesmanHipError, match=r"error -2: .*kept=0"):
        _lib.assign_tau_sampled(counts, np.full((3, 2), 0.5), eta, kept=0)
    with pytest.raises(_lib.DesmanHipError, match=r"error -4: .*65537"):
        _lib.assign_tau_sampled(counts, np.full((3, 2), 0.5), eta, burn=65537 - 100, kept=100)
    with pytest.raises(ValueError):
        _lib.assign_tau_sampled(counts, np.full((4, 2), 0.5), eta)
    with pytest.raises(ValueError):
        _lib.assign_tau_sampled(counts, np.full((3, 2), 0.5), eta, want=["logz"])


@pytest.fixture
def no_gpu_calls(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "assign_tau", boom)
    monkeypatch.setattr(_lib, "assign_tau_sampled", boom)
    monkeypatch.setattr(_lib, "load", boom)


def test_cli_refusals(tmp_path, no_gpu_calls):
    from desman_amd import assign
    run = _run_dir(tmp_path, ["S0", "S1"])
    freq, _ = _freq(tmp_path, ["S0", "S1"])
    with pytest.raises(SystemExit) as e:
        assign.main([run, freq, "--burn", "5"])
    assert "--burn needs --sampled" in str(e.value.code)
    for args in (["--sampled", "0"], ["--sampled", "5", "--burn", "-1"], ["--sampled", "65536", "--burn", "1"]):
        with pytest.raises(SystemExit) as e:
            assign.main([run, freq] + args)
        assert "B + T <= 65536" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        assign.main([_run_dir(tmp_path, ["S0", "S1"], G=33), freq, "--sampled"])
    assert "the limit of --sampled is G = 32" in str(e.value.code)
    opts = assign.build_parser().parse_args([run, freq, "--sampled"])
    assert opts.sampled == 100 == _lib.SAMPLED_KEPT and assign.SAMPLED_BURN == 20 == _lib.SAMPLED_BURN
    text = assign.build_parser().format_help()
    assert "not tuned" in text and "--sampled" in text and "--burn" in text


def test_sampled_result_files(tmp_path):
    from desman_amd import assign
    N, G = 5, 3
    rs = np.random.RandomState(1)
    res = dict(map_state=rs.randint(0, 4, size=(N, G)).astype(np.uint8), draw_state=rs.randint(0, 4, size=(N, G)).astype(np.uint8),
               conf=rs.rand(N), spread=rs.rand(N), marg=rs.dirichlet(np.ones(4), size=(N, G)), map_ll=-rs.rand(N) * 100)
    names, pos = ["c%d" % (n // 2) for n in range(N)], np.arange(N) * 3 + 1
    assign.write_sampled_results(str(tmp_path), names, pos, res, 7, 9)
    import pandas as pd
    star = pd.read_csv(tmp_path / "Assigned_Tau_star.csv", index_col=0)
    assert list(star.columns) == ["Position"] + [str(i) for i in range(4 * G)] and list(star.index) == names
    assert np.array_equal(np.argmax(star.to_numpy()[:, 1:].reshape(N, G, 4), axis=2), res["map_state"])
    for fname, key in (("Assigned_Tau_conf.csv", "conf"), ("Assigned_Tau_spread.csv", "spread")):
        fr = pd.read_csv(tmp_path / fname, index_col=0, float_precision="round_trip")
        assert list(fr.columns) == ["Position", "0"] and np.array_equal(fr["0"].to_numpy(), res[key]) and np.array_equal(fr["Position"].to_numpy(), pos)
    assert open(tmp_path / "assign_fit.txt").read() == "AssignSampled,%d,%d,7,9,%f\n" % (G, N, res["map_ll"].sum())
