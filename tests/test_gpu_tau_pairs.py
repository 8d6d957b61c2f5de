"""Pair moves of the main chain on the GPU (dsm_ctx_sample_tau_pairs, dsm_ctx_set_pair_moves, desman --pair-moves): one
pair pass against the numpy restatement (tests/_tau_pairs_ref.py) on every kernel instantiation, the keying, the law, the chain around
it, the refusals, what the move is for, and the command line.
Run on an MI355X with:  python -m pytest tests/test_gpu_tau_pairs.py -m gpu
"""
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _heldtau as H  # noqa: E402
import _tau_pairs_ref as P  # noqa: E402

from desman_amd import _lib  # noqa: E402
from desman_amd.synth import synth_counts, random_state  # noqa: E402

pytestmark = pytest.mark.gpu
MT_SEED, CTR_SEED = 4242, 0xABCDEF0123456789           # both key words non-zero and different: a dropped or swapped word shows
UNSUPPORTED = -4


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    c = _lib.Context(0)
    yield c
    c.close()


def _load(c, counts, tau, gamma, eta, rng=_lib.RNG_MT19937, every=None):
    c.set_counts(counts)
    c.set_state(tau, gamma, eta)
    c.seed(MT_SEED, ctr_seed=CTR_SEED)
    c.set_tau_rng(rng)
    if every is not None:
        c.set_pair_moves(every)


def _pass_on_device(c, counts, tau, gamma, eta, it):
    """(digits after the pass, changed digits) of dsm_ctx_sample_tau_pairs; neither the counter nor the MT19937 stream moves"""
    _load(c, counts, tau, gamma, eta)
    mt = c.get_mt_state()
    n = c.sample_tau_pairs(it)
    assert c.counters() == (CTR_SEED, 0) and np.array_equal(c.get_mt_state(), mt)
    got, g2, e2 = c.get_state()
    assert np.array_equal(g2, gamma) and np.array_equal(e2, eta) and (got.sum(axis=2) == 1).all()
    return P.digits(got), n


def _agree(c, counts, tau, gamma, eta, it, where):
    want, n_ref, close = P.pair_pass(counts, gamma, eta, P.digits(tau), CTR_SEED, it)
    assert close.mean() <= P.CLOSE_CAP, where                   # (on the restatement alone, before the device is looked at)
    got, n = _pass_on_device(c, counts, tau, gamma, eta, it)
    ok = ~close
    assert np.array_equal(got[ok], want[ok]), where
    if not close.any():
        assert n == n_ref, where
    return want, close


# ---- 1. one pass against the restatement: every instantiation, every edge of the shape -------------------------------------------------
# (V, S, G): V in {1, 63, 257} (a lone group, the grid-stride tail), S in {1, 9, 16, 17, 33, 64, 65, 130} and, for the instantiations those
# do not reach (64 lanes x 2 / 4 / 6 / 8 slots), 100 / 200 / 300 / 400; G in {2, 3, 8, 17, 32} (digits above bit 31, the word's top digit)
SHAPES = [(1, 1, 2), (63, 9, 3), (257, 16, 8), (63, 17, 17), (257, 33, 3), (63, 64, 8), (1, 65, 32), (63, 130, 2), (63, 17, 32),
          (257, 1, 3), (1, 100, 3), (63, 200, 2), (1, 300, 3), (63, 400, 2)]
DEPTH = 0.05       # of synth_counts' depth (about ten reads per sample): at full depth nearly every pair has one candidate with all the mass and
                   # the draw does not depend on its uniform -- a wrong keying or CDF would pass
INSTANTIATIONS = {(16, 1), (16, 2), (16, 3), (32, 2), (32, 3), (64, 2), (64, 3), (64, 4), (64, 6), (64, 8)}   # dsm_host.h: DSM_TAU_TILINGS


def test_the_shapes_reach_every_instantiation_of_the_launcher():
    assert {_lib.pairtau_debug_path(S, G) for _, S, G in SHAPES} == INSTANTIATIONS
    assert {V for V, _, _ in SHAPES} == {1, 63, 257} and {G for _, _, G in SHAPES} == {2, 3, 8, 17, 32}
    assert {1, 9, 16, 17, 33, 64, 65, 130} <= {S for _, S, _ in SHAPES}


@pytest.mark.parametrize("V,S,G", SHAPES)
def test_one_pass_is_the_restatement(ctx, V, S, G):
    counts, _, _ = synth_counts(V, S, G, seed=V + S, depth_scale=DEPTH)
    tau, gamma, eta = random_state(V, S, G, seed=G)
    want, _ = _agree(ctx, counts, tau, gamma, eta, 7, "V=%d S=%d G=%d" % (V, S, G))
    assert V < 8 or not np.array_equal(want, P.digits(tau))


@pytest.mark.parametrize("kind", ["identity", "zero-row", "zero counts", "dead position"])
def test_one_pass_on_the_edges_of_the_model(ctx, kind):
    """exact zeros in eta (candidates at -inf), a position whose sixteen candidates are all -inf for every pair (it stays), a table
    without reads (sixteen equal totals: the draw is the uniform's alone)"""
    V, S, G = 63, 9, 3
    counts, _, _ = synth_counts(V, S, G, seed=5)
    tau, gamma, eta = random_state(V, S, G, seed=6)
    if kind in ("identity", "zero-row"):
        eta = H.etas(kind, seed=3)
    elif kind == "zero counts":
        counts = np.zeros_like(counts)
    else:
        eta = np.eye(4)
        counts[0] = 0
        counts[0, 0] = [3, 2, 4, 0]                             # A, C and G read at once, every haplotype T: no pair can supply three bases
        tau[0] = P.onehot(np.array([[3, 3, 3]]))[0]
    want, close = _agree(ctx, counts, tau, gamma, eta, 2, kind)
    if kind == "dead position":
        assert not close[0] and np.array_equal(want[0], [3, 3, 3])
    if kind == "zero counts":
        assert not np.array_equal(want, P.digits(tau))


def test_every_mistake_of_the_keying_is_told_apart(ctx):
    V, S, G = 63, 9, 3
    counts, _, _ = synth_counts(V, S, G, seed=11, depth_scale=0.02)      # (shallow: the draws depend on their uniforms)
    tau, gamma, eta = random_state(V, S, G, seed=12)
    want, close = _agree(ctx, counts, tau, gamma, eta, 5, "the right keying")
    assert not close.any()
    got, _ = _pass_on_device(ctx, counts, tau, gamma, eta, 5)
    for m in P.MISTAKES:
        wrong, _, c = P.pair_pass(counts, gamma, eta, P.digits(tau), CTR_SEED, 5, mistake=m)
        assert not c.any() and not np.array_equal(wrong, got), m


def test_a_pass_leaves_the_exact_posterior_where_it_is(ctx):
    """the stationarity case of tests/test_tau_pairs_cpu.py through the device: 4096 copies of one position, G = 3, S = 4, starts drawn
    from the exact 64-state posterior; chi-square (63 degrees of freedom) of the states after one pass below the 1 - 1e-6 quantile"""
    counts, gamma, eta, start, post = P.stationarity_case()
    assert post.min() * len(start) >= 5.0
    got, n = _pass_on_device(ctx, counts, P.onehot(start), gamma, eta, 9)
    x2, bound = P.chi2_stat(16 * got[:, 0] + 4 * got[:, 1] + got[:, 2], post), P.chi2_threshold(63)
    print("device: chi-square %.2f after the pass, bound %.2f; %d digits changed" % (x2, bound, n))
    assert n > len(start) and x2 < bound


# ---- 2. the chain around it ------------------------------------------------------------------------------------------------------------
CHAIN = (257, 17, 3)


def _chain_case():
    V, S, G = CHAIN
    return synth_counts(V, S, G, seed=90)[0], random_state(V, S, G, seed=91)


def _everything(c):
    tr, st, star = c.get_trace(), c.get_state(), c.get_star()
    out = [tr[k] for k in ("gamma", "eta", "ll", "lp", "nchange")] + list(st) + [star["tau"], star["gamma"], star["eta"], np.array([star["lp"], star["it"]])]
    return out + [c.get_mt_state(), np.array(c.counters(), dtype=np.uint64), c.get_tau_sum()] + [c.get_tau_at(it) for it in range(-1, len(tr["ll"]))]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def chain_a(ctx):
    """chain A: E = 4, eight iterations in one call -- everything it reports, kept for the tests below"""
    counts, (tau, gamma, eta) = _chain_case()
    _load(ctx, counts, tau, gamma, eta, every=4)
    try:
        ctx.gibbs_update(8)
        return _everything(ctx)
    finally:
        ctx.set_pair_moves(0)


def test_switched_off_the_chain_is_the_chain_without_the_setting(ctx):
    counts, (tau, gamma, eta) = _chain_case()
    fresh = _lib.Context(0)                                     # dsm_ctx_set_pair_moves is never called on this one
    try:
        _load(fresh, counts, tau, gamma, eta)
        assert fresh.get_pair_moves() == 0
        fresh.gibbs_update(8)
        _load(ctx, counts, tau, gamma, eta, every=0)
        ctx.gibbs_update(8)
        assert _same(_everything(ctx), _everything(fresh))
    finally:
        fresh.close()


def test_the_iterations_before_the_first_pair_pass_are_those_without_pairs(ctx, ctx2):
    counts, (tau, gamma, eta) = _chain_case()
    _load(ctx, counts, tau, gamma, eta, every=4)
    _load(ctx2, counts, tau, gamma, eta, every=0)
    try:
        ctx.gibbs_update(3)
        ctx2.gibbs_update(3)
        assert _same(_everything(ctx), _everything(ctx2))
        ctx.gibbs_update(1)                                     # the fourth iteration is a pair iteration
        ctx2.gibbs_update(1)
        assert not np.array_equal(ctx.get_state()[0], ctx2.get_state()[0])
        assert np.array_equal(ctx.get_mt_state(), ctx2.get_mt_state()) and ctx.counters() == ctx2.counters() == (CTR_SEED, 4)
    finally:
        ctx.set_pair_moves(0)


def test_one_call_is_two_calls_is_a_run_resumed_from_a_checkpoint(ctx, ctx2, chain_a):
    counts, (tau, gamma, eta) = _chain_case()
    try:
        _load(ctx, counts, tau, gamma, eta, every=4)
        ctx.gibbs_update(3)
        a, ta = ctx.get_trace(), [ctx.get_tau_at(it) for it in range(3)]
        ck = ctx.checkpoint()
        ctx.gibbs_update(5)
        b, tb = ctx.get_trace(), [ctx.get_tau_at(it) for it in range(5)]
        for i, key in enumerate(("gamma", "eta", "ll", "lp", "nchange")):
            assert np.array_equal(np.concatenate([a[key], b[key]]), chain_a[i]), key
        assert _same(ta + tb, chain_a[-8:]) and _same(list(ctx.get_state()), chain_a[5:8])
        assert np.array_equal(ctx.get_mt_state(), chain_a[12]) and np.array_equal(np.array(ctx.counters(), dtype=np.uint64), chain_a[13])
        ctx2.set_counts(counts)                                 # the same five iterations after get / set of state, MT state and counters
        ctx2.restore(ck)
        ctx2.set_tau_rng(_lib.RNG_MT19937)
        ctx2.set_pair_moves(4)
        ctx2.gibbs_update(5)
        assert _same(_everything(ctx2), _everything(ctx))
    finally:
        ctx.set_pair_moves(0); ctx2.set_pair_moves(0)


def test_the_pair_iteration_is_the_sweep_then_the_restated_pass(ctx2, chain_a):
    """chain B runs three iterations with E = 4, then one with pairs off: its tau is the state before A's pair pass, row 0 of that
    call's gamma trace the gamma the sweep used, its eta after the first call the eta it used.  The restated pass on them with counter 3
    is A's stored tau of iteration 4, and A's nchange the sweep's count plus the pass's."""
    counts, (tau, gamma, eta) = _chain_case()
    _load(ctx2, counts, tau, gamma, eta, every=4)
    try:
        ctx2.gibbs_update(3)
        eta_old = ctx2.get_state()[2]
        ctx2.set_pair_moves(0)
        ctx2.gibbs_update(1)
    finally:
        ctx2.set_pair_moves(0)
    tr = ctx2.get_trace()
    assert np.array_equal(tr["gamma"][0], chain_a[0][3]) and np.array_equal(tr["eta"][0], chain_a[1][3])
    want, n_pass, close = P.pair_pass(counts, tr["gamma"][0], eta_old, P.digits(ctx2.get_state()[0]), CTR_SEED, 3)
    assert close.mean() <= P.CLOSE_CAP
    got = P.digits(chain_a[-8:][3])
    assert np.array_equal(got[~close], want[~close])
    if not close.any():
        assert chain_a[4][3] == tr["nchange"][0] + n_pass and n_pass > 0


def test_ll_and_lp_of_a_pair_iteration_describe_the_state_after_the_pass(ctx2, chain_a):
    counts, _ = _chain_case()
    gam, et, ll, lp = chain_a[0], chain_a[1], chain_a[2], chain_a[3]
    ctx2.set_counts(counts)
    for it in (3, 7):
        ctx2.set_state(chain_a[-8:][it], gam[it], et[it])
        l2, p2 = ctx2.loglik()
        assert abs(ll[it] - l2) <= 1e-10 * abs(l2) and abs(lp[it] - p2) <= 1e-10 * abs(p2), it
    best = int(chain_a[11][1])                                  # the MAP record: its iteration (0 = the entry state or iteration 0)
    assert chain_a[11][0] >= lp.max()
    if chain_a[11][0] == lp[best]:
        assert np.array_equal(chain_a[8], chain_a[-8:][best]) and np.array_equal(chain_a[9], gam[best])


def test_the_mt19937_stream_does_not_see_the_pairs(ctx2, chain_a):
    counts, (tau, gamma, eta) = _chain_case()
    _load(ctx2, counts, tau, gamma, eta, every=0)
    ctx2.gibbs_update(8)
    assert np.array_equal(ctx2.get_mt_state(), chain_a[12]) and not np.array_equal(ctx2.get_state()[0], chain_a[5])


def test_the_forms_without_a_pair_pass_say_so(ctx, ctx2):
    counts, (tau, gamma, eta) = _chain_case()
    V, S, G = CHAIN
    _load(ctx, counts, tau, gamma, eta, every=5)
    _load(ctx2, counts, tau, gamma, eta, every=0)
    try:
        lib = ctx.lib
        assert lib.dsm_ctx_set_pair_moves(ctx._h, -1) == -2 and ctx.get_pair_moves() == 5
        arr = (_lib.C.c_void_p * 2)(ctx2._h.value, ctx._h.value)
        last_error = lambda: lib.dsm_last_error().decode()
        assert lib.dsm_batch_gibbs_update(arr, 2, 1) == UNSUPPORTED and "pair moves" in last_error()
        assert lib.dsm_ctx_gibbs_update_held_tau(ctx._h, 1, 1, 0) == UNSUPPORTED and "pair moves" in last_error()
        ctx.set_tau_rng(_lib.RNG_PHILOX)
        with pytest.raises(_lib.DesmanHipError, match="error -4: .*pair moves"):
            ctx.gibbs_update_sharded(1, 0, V, lambda *a: 0)
        ctx.set_tau_rng(_lib.RNG_MT19937)
        assert all(np.array_equal(x, y) for x, y in zip(ctx.get_state(), (tau, gamma, eta))) and ctx.counters() == (CTR_SEED, 0)
        # the fixed-tau chain has no tau step: the setting is not looked at
        ctx.gibbs_update_fixed_tau(6, pool=0)
        ctx2.gibbs_update_fixed_tau(6, pool=0)
        assert _same(_everything(ctx), _everything(ctx2))
    finally:
        ctx.set_pair_moves(0); ctx.set_tau_rng(_lib.RNG_MT19937)


# ---- 3. what the move is for -----------------------------------------------------------------------------------------------------------
def test_pairs_free_the_positions_that_trap_the_single_site_sweep(ctx):
    """trapping_case() of tests/test_assign_pairs_cpu.py (G = 8, S = 12, 32 positions), gamma and eta held at the generating values, tau
    from all digits 0, 100 single-site sweeps in Philox tau mode -- alone, and with a pair pass after every fifth.  Wrong = the last
    state differs from the exact MAP state (dsm_assign_tau).  The device reproduces the restatement's two counts
    (tests/test_tau_pairs_cpu.py prints them), and the count with pairs is the smaller."""
    from test_tau_pairs_cpu import trapping_runs
    from test_assign_pairs_cpu import trapping_case
    counts, gamma, eta = trapping_case()
    V, G = counts.shape[0], gamma.shape[1]
    ref = trapping_runs()
    assert not ref["close"]
    wrong = {}
    try:
        for E in (0, 5):
            _load(ctx, counts, P.onehot(np.zeros((V, G), dtype=np.int64)), gamma, eta, rng=_lib.RNG_PHILOX)
            ctx.set_gamma_eta(gamma, eta)
            for r in range(100):
                ctx.sample_tau()
                if E and (r + 1) % E == 0:
                    ctx.sample_tau_pairs(r)
            last = P.digits(ctx.get_state()[0])
            assert np.array_equal(last, ref["last"][E]), E
            exact = ctx.assign_tau(gamma, eta)["map_state"]
            wrong[E] = int((~(last == exact).all(axis=1)).sum())
    finally:
        ctx.set_tau_rng(_lib.RNG_MT19937)
    print("trapping table, device: %d of 32 positions wrong without pairs, %d with a pair pass after every fifth sweep" % (wrong[0], wrong[5]))
    assert wrong == ref["wrong"] and wrong[5] < wrong[0]


# ---- 4. the command line ---------------------------------------------------------------------------------------------------------------
def _write_freq(path, counts, names, contigs, positions):
    V, S, _ = counts.shape
    cols = ["Position"] + ["%s-%s" % (n, b) for n in names for b in "ACGT"]
    data = np.concatenate([np.asarray(positions)[:, None], counts.reshape(V, S * 4)], axis=1)
    df = pd.DataFrame(data, index=list(contigs), columns=cols)
    df.index.name = "Contig"
    df.to_csv(path)


def test_desman_pair_moves(tmp_path, monkeypatch):
    from desman_amd import cli
    V, S, G, n = 120, 8, 3, 20
    counts, _, _ = synth_counts(V, S, G, seed=123)
    freq = str(tmp_path / "fit.freq")
    _write_freq(freq, counts, ["S%d" % s for s in range(S)], ["contig%d" % (v // 50) for v in range(V)], np.arange(V) * 7 + 3)
    seen = []
    report = cli._report

    def keep(rep, table, flt, chain, requested):
        seen.append((chain.pair_every, chain._ctx.get_pair_moves()))
        report(rep, table, flt, chain, requested)
    monkeypatch.setattr(cli, "_report", keep)
    plain, flags, pairs = (str(tmp_path / d) for d in ("plain", "flags", "pairs"))
    args = [freq, "-g", str(G), "-i", str(n), "-s", "7"]
    cli.main(args + ["-o", plain])
    cli.main(args + ["-o", flags, "--diagnose", "--relabel"])
    cli.main(args + ["-o", pairs, "--pair-moves", "--diagnose", "--relabel"])
    assert seen == [(0, 0), (0, 0), (5, 5)]                    # the setting reaches the context the chain runs on
    extra = ["Relabel.csv", "Tau_Mean_relabelled.csv", "Gamma_Mean_relabelled.csv", "SND_posterior.csv", "Haplotype_stability.csv",
             "Tau_MCSE.csv", "Tau_diag.csv", "Diag_scalars.csv"]
    assert sorted(os.listdir(pairs)) == sorted(os.listdir(flags)) == sorted(os.listdir(plain) + extra)
    read = lambda d, name: open(os.path.join(d, name), "rb").read()
    for name in os.listdir(plain):                             # without the flag the usual files are what they were
        if name != "log_file.txt":
            assert read(plain, name) == read(flags, name), name
    for name in os.listdir(pairs):
        assert len(read(pairs, name)) > 0, name
