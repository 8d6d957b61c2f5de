"""The deferred stage-1 items of the aggregated mu/E pass where test_gpu_big_launch_modes.py does not reach: every kind of item, the subset
table in copies, specification 3, the edges of the arrival protocol, the look a Gibbs call takes every 64 iterations, the chains whose
launch of stats_big_kernel is not a choice, mixed modes in a batch.  Every comparison is bit equality.

The cases and what each is there for are in tests/_deferred.py (CASES); their preconditions -- copies of the table, items of each kind in
the very passes drawn here, a sub-list longer than one stride -- are asserted on the CPU by test_deferred_cpu.py.

gap (of the issue this file answers)          test
1 copies of the subset table                  test_one_pass_is_the_oracles[copies | swizzle | copies32], test_chains_are_the_same_in_every_mode[copies]
2 item kind 2                                 test_one_pass_is_the_oracles[kind2 | S70 | long], test_chains_are_the_same_in_every_mode[kind2]
3 specification 3                             every test here is run under 2 and 3
4 S = 1, swizzle groups, G = 1, G = 9, long   test_one_pass_is_the_oracles[S1 | swizzle | G1 | G9 | long], test_chains_are_the_same_in_every_mode[S1]
5 the look every 64 iterations                test_the_look_every_64_iterations[shallow | mixed | overfit]
6 where the launch is not a choice            test_mode_0_is_ignored_where_the_launch_is_not_a_choice
  (batch)                                     test_batch_with_mixed_modes
"""
import numpy as np
import pytest

from desman_amd import _lib
from oracle import cbind

import _deferred as d
from test_gpu_big_launch_modes import MIXED, SHALLOW, _result, _same, _table

pytestmark = pytest.mark.gpu

MT = _lib.RNG_MT19937
SPECS = (2, 3)
N_IT = 6


def _ctx(table, mode, spec, neartie=-1, mt_seed=99, ctr_seed=d.CTR_SEED):
    counts, tau, gamma, eta = table
    c = _lib.Context(0)
    c.set_counts(counts)
    c.force_stats_spec(spec)                 # (the shape rule gives tables this small the per-read pass)
    c.set_state(tau, gamma, eta)
    c.set_tau_rng(MT)
    c.seed(mt_seed, ctr_seed=ctr_seed)
    c.set_big_launch(mode)
    c.set_tau_neartie(neartie)
    return c


def _launches(c):
    return c.get_timing()["stats_big"][1]


# ---------------------------------------------------------------- A. one pass against the oracle
_oracle = {}


def _oracle_pass(name, it, spec):
    if (name, it, spec) not in _oracle:
        counts, tau, gamma, eta = d.case_table(name)
        _oracle[name, it, spec] = cbind.stats_agg(cbind.onehot_to_idx(tau), gamma, eta, counts, d.CTR_SEED, it, spec=spec)
    return _oracle[name, it, spec]


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(d.CASES))
def test_one_pass_is_the_oracles(name, mode, spec):
    """sample_stats: stage 1, then stats_stage2_kernel -- which draws the lists' items itself in mode 0"""
    table = d.case_table(name)
    counts = table[0]
    c = _ctx(table, mode, spec)
    try:
        assert c.stats_spec() == spec
        closings = 0
        for it in d.PASS_ITS:
            mu, E = c.sample_stats(it)
            mu_ref, E_ref = _oracle_pass(name, it, spec)
            assert np.array_equal(E, E_ref), (it, "E")              # every item drawn once: none lost, none twice
            assert np.array_equal(mu, mu_ref), (it, "mu")
            assert int(mu.sum()) == int(counts.sum()) == int(E.sum())
            nz, seen = c.debug_big_lists()
            assert nz == 0, it
            if mode == 0:
                assert _launches(c) == 0
                closings += int((d.case_kinds(name, it, spec) >= 0).any())
                assert seen == closings, it                          # one closing of the lists per pass that handed items over
        assert mode == 0 or _launches(c) == len(d.PASS_ITS)
    finally:
        c.close()


# ---------------------------------------------------------------- B. whole chains in every mode
def _passes_with_items(table, spec, n):
    """[n] whether stage 1 hands an item over in each iteration (the oracle's kinds at the states a chain stepped one iteration at a time
    passes through)"""
    c = _ctx(table, 1, spec)
    out = []
    try:
        for it in range(n):
            t, g, e = c.get_state()
            assert c.counters() == (d.CTR_SEED, it)
            out.append(bool((d.item_kinds(table[0], t, g, e, d.CTR_SEED, it, spec) >= 0).any()))
            c.gibbs_update(1)
    finally:
        c.close()
    return out


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("name", d.CHAIN_CASES)
def test_chains_are_the_same_in_every_mode(name, spec):
    """gibbs_update: stage 1, then dirichlet_kernel with stage 2 fused -- which draws the lists' items itself where the launch is left out"""
    table = d.case_table(name)
    with_items = _passes_with_items(table, spec, N_IT)
    print(name, "spec", spec, "iterations that hand items over", with_items)
    assert with_items[0]
    runs = {}
    for mode in (1, 0, -1):
        c = _ctx(table, mode, spec)
        try:
            c.gibbs_update(N_IT)
            runs[mode] = _result(c)
            nz, seen = c.debug_big_lists()
            assert nz == 0
            assert _launches(c) == (0 if mode == 0 else N_IT)        # (-1: the first call after set_state launches)
            if mode == 0:
                assert seen == sum(with_items)
        finally:
            c.close()
    _same(runs[1], runs[0], "mode 0")
    _same(runs[1], runs[-1], "mode -1")


# ---------------------------------------------------------------- C. the look every 64 iterations
N_LONG = 130
_LOOK_TABLES = {"shallow": lambda: _table((64, 17, 3), SHALLOW), "mixed": lambda: _table(MIXED[0], MIXED[1], MIXED[2]), "overfit": d.overfit_table}
_WANT_LAUNCHES = {"shallow": 64, "mixed": 128}


def _launches_by_the_rule(with_items):
    """api.hip: gibbs_update + kernels_stats.hip: stats_big_take, automatic mode, first call after set_state: launched until a look (every 64
    iterations) finds that the device's count of non-empty lists has not moved since the last reading"""
    hot, moved, n = True, False, 0
    for it, items in enumerate(with_items):
        if it and it % 64 == 0:
            hot, moved = moved, False
        n += hot
        moved = moved or items
    return n


def _long_run(table, big, neartie, calls):
    c = _ctx(table, big, 2, neartie=neartie)
    out = dict(ll=[], lp=[], gamma=[], eta=[], nchange=[], taus=[], stars=[])
    try:
        for n in calls:
            c.gibbs_update(n)
            tr = c.get_trace()
            for k in ("ll", "lp", "gamma", "eta", "nchange"):
                out[k].append(tr[k])
            out["taus"] += [c.get_tau_at(it) for it in range(n)]
            out["stars"].append(c.get_star())
        for k in ("ll", "lp", "gamma", "eta", "nchange"):
            out[k] = np.concatenate(out[k])
        out["state"] = c.get_state()
        out["mt"] = c.get_mt_state()
        out["launches"] = _launches(c)
        out["lists"] = c.debug_big_lists()[0]
    finally:
        c.close()
    return out


@pytest.mark.parametrize("which", list(_LOOK_TABLES))
def test_the_look_every_64_iterations(which):
    """One call of 130 iterations in the automatic modes looks at the chain at iterations 64 and 128 -- a stream synchronisation while the
    MT19937 words of later sweeps are being generated on the side stream -- and may change there whether stats_big_kernel is launched
    and which instantiation of the sweep runs.  Neither may change the chain."""
    table = _LOOK_TABLES[which]()
    counts, tau0, gamma0, eta0 = table
    V, S, G = counts.shape[0], counts.shape[1], tau0.shape[1]
    assert V * S <= 64 * 17 and G <= 3
    auto = _long_run(table, -1, -1, [N_LONG])
    others = {"both forced, one call": _long_run(table, 1, 0, [N_LONG]), "both forced, 64 + 64 + 2": _long_run(table, 1, 0, [64, 64, 2]),
              "no launch, near-tie sweep": _long_run(table, 0, 1, [N_LONG])}
    for what, r in others.items():
        for k in ("ll", "lp", "gamma", "eta", "nchange", "mt"):
            assert np.array_equal(auto[k], r[k]), (what, k)
        assert len(r["taus"]) == N_LONG and all(np.array_equal(a, b) for a, b in zip(auto["taus"], r["taus"])), what
        assert all(np.array_equal(a, b) for a, b in zip(auto["state"], r["state"])), what
        assert r["lists"] == 0
    # the MAP record: whole for the runs of one call; of the split run, the call that holds the record's iteration has the same record
    star = auto["stars"][0]
    for what in ("both forced, one call", "no launch, near-tie sweep"):
        s = others[what]["stars"][0]
        assert s["lp"] == star["lp"] and s["it"] == star["it"] and all(np.array_equal(s[k], star[k]) for k in ("tau", "gamma", "eta")), what
    if star["lp"] in auto["lp"]:
        k = int(np.argmax(auto["lp"] == star["lp"]))
        call, off = (0, 0) if k < 64 else (1, 64) if k < 128 else (2, 128)
        s = others["both forced, 64 + 64 + 2"]["stars"][call]
        assert s["lp"] == star["lp"] and s["it"] + off == star["it"] and all(np.array_equal(s[k_], star[k_]) for k_ in ("tau", "gamma", "eta"))
    else:                                                            # the entry state
        s = others["both forced, 64 + 64 + 2"]["stars"][0]
        assert np.array_equal(star["tau"], tau0) and np.array_equal(s["tau"], tau0)
    # every sweep against the oracle on the GSL stream: the words generated ahead survive the look's synchronisation
    mt = cbind.MT19937(99)
    ref, eta_prev = tau0.copy(), np.ascontiguousarray(eta0)
    for it in range(N_LONG):
        n_ref = cbind.sample_tau_u(ref, np.ascontiguousarray(auto["gamma"][it]), eta_prev, counts, mt.uniform(V * G))
        assert np.array_equal(auto["taus"][it], ref) and auto["nchange"][it] == n_ref, it
        eta_prev = np.ascontiguousarray(auto["eta"][it])
    # the launches the rule implies
    with_items = _passes_with_items(table, 2, N_LONG)
    want = _launches_by_the_rule(with_items)
    print(which, "iterations that hand items over:", sum(with_items), "launches by the rule:", want, "made:", auto["launches"])
    if which == "shallow":
        assert not any(with_items)
    if which == "mixed":
        assert with_items[0] and not any(with_items[N_IT:])
    if which in _WANT_LAUNCHES:
        assert want == _WANT_LAUNCHES[which]
    assert auto["launches"] == want
    assert others["both forced, one call"]["launches"] == others["both forced, 64 + 64 + 2"]["launches"] == N_LONG
    assert others["no launch, near-tie sweep"]["launches"] == 0
    if which == "overfit":
        # the look did change the sweep's instantiation: no rare haplotype at the start (the plain sweep), one at a look
        start = d.rare_count(gamma0)
        looks = [d.rare_count(auto["gamma"][63]), d.rare_count(auto["gamma"][127])]
        print("rare haplotypes at the start", start, "at the looks", looks)
        assert start == 0 and G > 2
        assert any(0 < n < G for n in looks), looks


# ---------------------------------------------------------------- D. where the launch is not a choice
_DEEP = 40.0


def _fixed_case(kind):
    """(table, specification forced, specification run, how to run 4 iterations)"""
    if kind == "G10":
        return d._generating((40, 17, 10), _DEEP, 7), 2, 2, lambda c, n: c.gibbs_update(n)
    if kind == "spec4":
        return d._generating((40, 17, 3), _DEEP, 7), 4, 4, lambda c, n: c.gibbs_update(n)
    if kind == "spec1":
        return d._generating((40, 17, 3), _DEEP, 7), 1, 1, lambda c, n: c.gibbs_update(n)
    if kind == "held":
        return d._generating((40, 17, 3), _DEEP, 7), 2, 2, lambda c, n: c.gibbs_update_held_tau(n, 1)
    return d._generating((40, 17, 3), _DEEP, 7), 2, 2, lambda c, n: c.gibbs_update_fixed_tau(n, pool=0)


@pytest.mark.parametrize("kind", ["G10", "spec4", "spec1", "held", "fixed"])
def test_mode_0_is_ignored_where_the_launch_is_not_a_choice(kind):
    """G >= 10 (stage 2 is a launch of its own, without the lists), specification 4 (pooled counts), specification 1 (no lists at all), the
    partly held and the fixed-tau chain: no consumer but stats_big_kernel, so mode 0 must not take the launch away"""
    table, spec, runs_spec, run = _fixed_case(kind)
    n = 4
    assert d.handed_over(*table) > 0
    res = {}
    for mode in (1, 0):
        c = _ctx(table, mode, spec)
        try:
            assert c.stats_spec() == runs_spec
            run(c, n)
            res[mode] = _result(c)
            assert c.debug_big_lists()[0] == 0
            assert _launches(c) == (0 if runs_spec == 1 else n), mode
        finally:
            c.close()
    _same(res[1], res[0], "mode 0")


# ---------------------------------------------------------------- E. batch
@pytest.mark.parametrize("spec", SPECS)
def test_batch_with_mixed_modes(spec):
    """test_gpu_big_launch_modes.py: test_batched_chains_without_the_launch under either specification, and with the chains' modes mixed:
    a batch launches stats_big_kernel_b if any of its chains wants the launch"""
    shape = (40, 64, 8)
    counts, tau, _, eta = _table(shape, _DEEP)
    rng = np.random.default_rng(5)
    starts = [np.ascontiguousarray(rng.dirichlet(np.ones(shape[2]), size=shape[1])) for _ in range(3)]
    alone = []
    for k, g0 in enumerate(starts):
        c = _ctx((counts, tau, g0, eta), 1, spec, mt_seed=200 + k, ctr_seed=d.CTR_SEED + k)
        try:
            c.gibbs_update(N_IT)
            alone.append(_result(c))
        finally:
            c.close()
    for modes in ((0, 0, 0), (0, -1, 1)):
        ctxs = [_ctx((counts, tau, g0, eta), modes[k], spec, mt_seed=200 + k, ctr_seed=d.CTR_SEED + k) for k, g0 in enumerate(starts)]
        try:
            _lib.Context.batch_gibbs_update(ctxs, N_IT)
            for k, c in enumerate(ctxs):
                _same(alone[k], _result(c), "chain %d of the batch %r" % (k, modes))
                nz, seen = c.debug_big_lists()
                assert nz == 0 and seen >= N_IT                      # (a launch counts every non-empty list, the inline phase one per iteration)
                if modes == (0, 0, 0):
                    assert seen == N_IT
        finally:
            for c in ctxs:
                c.close()
