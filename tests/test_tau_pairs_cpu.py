"""Pair moves of the main chain (dsm_ctx_set_pair_moves, dsm_ctx_sample_tau_pairs, desman --pair-moves): what can be
checked without a GPU -- the numpy restatement of a pair pass (tests/_tau_pairs_ref.py) against the exact joint posterior at G = 2 and
as a move that leaves the exact posterior at G = 3 where it is; the symbols; the refusals made before any device work."""
import functools
import inspect
import os
import re
import types

import numpy as np
import pytest

from desman_amd import _lib
from _assign_pairs_ref import pair_candidates
import _tau_pairs_ref as P

CTR_SEED = 0xABCDEF0123456789                 # the key of tests/test_gpu_tau_pairs.py


def test_one_pass_at_two_haplotypes_draws_from_the_exact_joint_posterior():
    """G = 2: the one pair step of a pass redraws both digits from the joint posterior whatever the start.  4 seeds x 8192 copies of one
    position (three samples, a read or two each, a smooth eta so that all sixteen states expect >= 5 draws -- asserted), random starts.
    Pearson's chi-square of the 32768 draws against the enumerated posterior, 15 degrees of freedom, must stay below the 1 - 1e-6
    quantile (56.49): a true law fails once in a million tables; the seeds are fixed."""
    rs = np.random.RandomState(41)
    S, V = 3, 8192
    gamma = rs.dirichlet(np.ones(2), size=S)
    eta = 0.6 * rs.dirichlet(np.full(4, 50.0), size=4) + 0.4 * np.eye(4)
    p = np.einsum("sg,gb->sb", gamma, eta[[1, 2]])
    one = np.array([rs.multinomial(1 + (s == 0), p[s]) for s in range(S)], dtype=np.int64)
    L = pair_candidates(one[None].astype(np.float64), gamma, eta, np.zeros((1, 1, 2), dtype=np.int64), 0, 1)[0, 0]
    post = np.exp(L - L.max())
    post /= post.sum()
    counts = np.repeat(one[None], V, axis=0)
    draws = []
    for seed in (0x5EEDC0DE00000001, 0xABCDEF0100000000, 777, 0x0123456789ABCDEF):
        start = rs.randint(0, 4, size=(V, 2))
        new, nch, close = P.pair_pass(counts, gamma, eta, start, seed, 3)
        assert not close.any() and nch == int((new != start).sum())
        draws.append(4 * new[:, 0] + new[:, 1])
    draws = np.concatenate(draws)
    assert post.min() * len(draws) >= 5.0
    x2, bound = P.chi2_stat(draws, post), P.chi2_threshold(15)
    print("G = 2: chi-square %.2f of %d draws against the exact posterior, bound %.2f" % (x2, len(draws), bound))
    assert x2 < bound


def test_a_pass_leaves_the_exact_posterior_at_three_haplotypes_where_it_is():
    """G = 3, S = 4: starts drawn from the exact 64-state posterior are still distributed so after a pass over (0,1), (0,2), (1,2)
    (every step is a draw from a conditional of that posterior).  4096 copies of one position; chi-square with 63 degrees of freedom
    below its 1 - 1e-6 quantile (131.37).  The same case runs through the device in tests/test_gpu_tau_pairs.py."""
    counts, gamma, eta, start, post = P.stationarity_case()
    assert post.min() * len(start) >= 5.0 and abs(post.sum() - 1.0) < 1e-12
    bound = P.chi2_threshold(63)
    x0 = P.chi2_stat(16 * start[:, 0] + 4 * start[:, 1] + start[:, 2], post)
    new, nch, close = P.pair_pass(counts, gamma, eta, start, 0xABCDEF0123456789, 9)
    x1 = P.chi2_stat(16 * new[:, 0] + 4 * new[:, 1] + new[:, 2], post)
    print("G = 3: chi-square %.2f of the starts, %.2f after the pass, bound %.2f; %d digits changed" % (x0, x1, bound, nch))
    assert not close.any() and nch > len(start) and x0 < bound and x1 < bound
    # a pass that drew from the wrong law is told apart: the same uniforms used as if every state were equally likely
    flat = P.chi2_stat(np.random.RandomState(3).randint(0, 64, size=len(start)), post)
    assert flat > bound


def test_the_mistakes_of_the_keying_draw_other_uniforms():
    right = P.pair_uniforms(0xABCDEF0123456789, 5, 7, 3)
    iu = np.triu_indices(3, 1)
    for m in P.MISTAKES:
        wrong = P.pair_uniforms(0xABCDEF0123456789, 5, 7, 3, mistake=m)
        assert not np.array_equal(wrong[:, iu[0], iu[1]], right[:, iu[0], iu[1]]), m
    assert ((right >= 0) & (right < 1)).all()


def test_a_dead_pair_stays_and_a_position_without_reads_has_flat_totals():
    """eta = the identity, one sample, G = 3.  Position 0 is read as A, C and G at once while every haplotype is T: whichever pair is
    redrawn, the third haplotype stays T and two haplotypes cannot supply three bases -- all sixteen totals are -inf for every pair, and
    the position stays as it is.  Position 1 has no reads: its sixteen totals are 0."""
    gamma, eta = np.array([[0.5, 0.3, 0.2]]), np.eye(4)
    counts = np.array([[[3, 2, 4, 0]], [[0, 0, 0, 0]]], dtype=np.int64)
    tau = np.array([[3, 3, 3], [1, 2, 3]])
    for g, h in ((0, 1), (0, 2), (1, 2)):
        L = pair_candidates(counts.astype(np.float64), gamma, eta, tau[:, None, :], g, h)[:, 0, :]
        assert np.isneginf(L[0]).all() and (L[1] == 0.0).all()
    new, nch, close = P.pair_pass(counts, gamma, eta, tau, 1, 0)
    # (the count is per step, against the pair's digits before the step: a digit that moves twice counts twice)
    assert np.array_equal(new[0], tau[0]) and not close.any() and nch >= int((new[1] != tau[1]).sum())


# ---- what the move is for ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trapping_runs():
    """trapping_case() of tests/test_assign_pairs_cpu.py (G = 8, S = 12, 32 positions) under the restatement: gamma and eta at the
    generating values, tau from all digits 0, 100 single-site sweeps keyed as the Philox tau mode keys them (counter = the round), alone
    (E = 0) and with a pair pass after every fifth, keyed by that round's counter (E = 5).  -> last states, wrong-call counts against the
    exact MAP states (numpy enumeration of the 4^8 states), and whether any step was close.  The key is the one every test of this file
    and of tests/test_gpu_tau_pairs.py uses; it was not searched for."""
    from test_assign_cpu import assign_numpy
    from test_assign_pairs_cpu import trapping_case
    counts, gamma, eta = trapping_case()
    exact = assign_numpy(counts, gamma, eta)["map_state"]
    last, wrong, close = {}, {}, False
    for E in (0, 5):
        tau = np.zeros((counts.shape[0], gamma.shape[1]), dtype=np.int64)
        for r in range(100):
            tau, _, c = P.single_site_sweep(counts, gamma, eta, tau, CTR_SEED, r)
            close = close or bool(c.any())
            if E and (r + 1) % E == 0:
                tau, _, c = P.pair_pass(counts, gamma, eta, tau, CTR_SEED, r)
                close = close or bool(c.any())
        last[E] = tau
        wrong[E] = int((~(tau == exact).all(axis=1)).sum())
    return dict(last=last, wrong=wrong, close=close)


def test_pairs_free_the_positions_that_trap_the_single_site_sweep():
    """the restatement's two counts (the device must reproduce them: tests/test_gpu_tau_pairs.py): the single-site run leaves some
    position wrong, the run with pairs fewer"""
    run = trapping_runs()
    print("trapping table, restatement: %d of 32 positions wrong after 100 single-site sweeps, %d with a pair pass after every fifth"
          % (run["wrong"][0], run["wrong"][5]))
    assert not run["close"] and run["wrong"][0] > 0 and run["wrong"][5] < run["wrong"][0]


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    from desman_amd.vshard import ShardedChain
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dsm_ctx_set_pair_moves", "dsm_ctx_get_pair_moves", "dsm_ctx_sample_tau_pairs", "dsm_pairtau_debug_path"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for fn in (_lib.Context.set_pair_moves, _lib.Context.get_pair_moves, _lib.Context.sample_tau_pairs, _lib.pairtau_debug_path):
        assert callable(fn)
    assert inspect.signature(HaploSNP_Sampler.__init__).parameters["pair_every"].default == 0
    assert inspect.signature(ShardedChain.__init__).parameters["pair_every"].default == 0
    assert lib.dsm_ctx_set_pair_moves(None, 1) == -2 and lib.dsm_ctx_get_pair_moves(None, None) == -2      # (a null context)
    assert _lib.pairtau_debug_path(12, 8) == (16, 1) and _lib.pairtau_debug_path(64, 8) == (32, 2) and _lib.pairtau_debug_path(512, 32) == (64, 8)
    with pytest.raises(_lib.DesmanHipError):
        _lib.pairtau_debug_path(513, 8)
    src = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "desman_amd", "csrc", "dsm_device.h")).read()
    assert re.search(r"#define\s+DSM_STREAM_TPAR\s+0x%08Xu" % P.STREAM_TPAR, src) and P.STREAM_TPAR == int.from_bytes(b"TPAR", "big")


def test_the_command_line_refuses_what_it_cannot_serve_before_any_chain(tmp_path, monkeypatch):
    from desman_amd import cli

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", boom)
    out = str(tmp_path / "out")
    freq = str(tmp_path / "never_read.freq")                   # the file does not exist: a run that got as far as loading would say so
    for bad in ("0", "-3"):
        with pytest.raises(SystemExit) as e:
            cli.main([freq, "-g", "3", "-o", out, "--pair-moves", bad])
        assert "--pair-moves" in str(e.value) and "E >= 1; got %s" % bad in str(e.value)
    with pytest.raises(SystemExit, match="--pair-moves is not available for replicate chains"):
        cli.main_replicates([[freq, "-g", "3", "-o", out, "--pair-moves"]])
    assert not os.path.exists(out)
    parse = cli.build_parser().parse_args
    assert parse([freq, "-g", "3"]).pair_moves is None and cli._pair_moves_options(parse([freq, "-g", "3"])) == 0
    assert parse([freq, "-g", "3", "--pair-moves"]).pair_moves == 5 == cli.PAIR_MOVES
    assert cli._pair_moves_options(parse([freq, "-g", "3", "--pair-moves", "2", "--relabel", "--diagnose", "--check", "--predictive"])) == 2
    assert "--pair-moves [E]" in cli.build_parser().format_help()


def test_the_sampler_refuses_what_it_cannot_serve_before_any_device_work(monkeypatch):
    from desman_amd.HaploSNP_Sampler import HaploSNP_Sampler
    from desman_amd.vshard import ShardedChain

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "Context", boom)
    snps = np.ones((3, 2, 4), dtype=np.int64)
    for bad in (-1, 2.5, "5", True, None):
        with pytest.raises(ValueError, match="pair_every"):
            HaploSNP_Sampler(snps, 2, np.random.RandomState(1), pair_every=bad)
    with pytest.raises(AssertionError, match="the library was called"):      # a good value goes on to the context
        HaploSNP_Sampler(snps, 2, np.random.RandomState(1), pair_every=np.int64(4))
    on = types.SimpleNamespace(pair_every=5, max_iter=3, mt_state=np.zeros(625, dtype=np.uint32), G=3,
                               _push_state=boom, _bind_rng=boom)
    off = types.SimpleNamespace(pair_every=0, max_iter=3, mt_state=np.zeros(625, dtype=np.uint32), G=3, _push_state=boom, _bind_rng=boom)
    with pytest.raises(ValueError, match="update_batch: pair moves"):
        HaploSNP_Sampler.update_batch([off, on])
    with pytest.raises(ValueError, match="update_held: pair moves"):
        HaploSNP_Sampler.update_held(on, 1)
    with pytest.raises(AssertionError, match="the library was called"):      # without pair moves both go on
        HaploSNP_Sampler.update_held(off, 1)
    with pytest.raises(AssertionError, match="the library was called"):
        HaploSNP_Sampler.update_batch([off, off])
    with pytest.raises(ValueError, match="sharded chain: pair moves"):
        ShardedChain(snps, 0, 3, 2, 1, pair_every=5)
