"""The preconditions of the deferred-item cases (tests/_deferred.py: CASES), asserted on the CPU from the inputs and the oracle alone: the
number of copies of the subset table, the kinds of item the lean stage 1 hands over in the very passes test_gpu_deferred_items.py draws
(iterations 0 and 5 under CTR_SEED, specifications 2 and 3), the length of the longest deferred sub-list.  A case that loses its
precondition -- another generator, another rule -- fails here, by name, and not by a GPU test that silently stops covering its path."""
import numpy as np
import pytest

import _deferred as d
from oracle import cbind

SPECS = (2, 3)


@pytest.mark.parametrize("name", sorted(d.CASES))
def test_copies_of_the_subset_table(name):
    V, S, G = d.CASES[name][0]
    assert d.ntab_rep(V, S, G) == d.WANT_REP[name]


def test_the_rule_of_the_copies_by_hand():
    """three values worked out from kernels_stats.hip: stats_ntab_rep by hand, and the two shapes with copies that differ"""
    assert d.ntab_rep(400, 5, 2) == 64           # 300 atomics per counter; 2 lines: 2 x 32 < 384
    assert d.ntab_rep(400, 24, 3) == 32          # 150 per counter; 12 lines x 32 = 384
    assert d.ntab_rep(700, 20, 3) == 64          # 262 per counter; 10 lines x 32 = 320 < 384
    assert d.ntab_rep(400, 64, 8) == 1           # 4.7 per counter
    assert d.ntab_rep(341, 20, 3) == 1 and d.ntab_rep(342, 20, 3) > 1      # the edge: 3 V / 2^G <= 128
    assert d.WANT_REP["copies"] != d.WANT_REP["copies32"] and min(d.WANT_REP["copies"], d.WANT_REP["swizzle"], d.WANT_REP["copies32"]) > 1


def test_the_swizzle_cases_reach_the_second_group():
    for name in ("swizzle", "copies32"):
        S = d.CASES[name][0][1]
        assert 16 < S <= 32 and (S - 1) >> 4 == 1
    for spec in SPECS:
        for it in d.PASS_ITS:
            k = d.case_kinds("swizzle", it, spec)
            assert (k[:, :16] >= 0).any() and (k[:, 16:] >= 0).any()        # items handed over in both groups of samples


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("it", d.PASS_ITS)
@pytest.mark.parametrize("name", sorted(d.CASES))
def test_kinds_handed_over(name, it, spec):
    counts, tau, gamma, eta = d.case_table(name)
    kinds = d.case_kinds(name, it, spec)
    n = d.kind_counts(kinds)
    print(name, "it", it, "spec", spec, "items of kind 0, 1, 2:", n)
    assert kinds.shape == counts.shape and ((kinds >= -1) & (kinds <= 2)).all()
    assert (kinds[counts == 0] == -1).all()
    # the rule that needs no draw is a lower bound of kinds 0 and 1, item by item
    deferred, kind0 = d.first_rule(counts, tau, gamma, eta)
    assert (kinds[kind0] == 0).all() and (kinds[deferred & ~kind0] == 1).all()
    if name == "G1":
        # one haplotype: one true base carries all the weight, no read of another base is ever drawn -- nothing can be handed over.
        # The case is there for the trivial stage 2 behind a launch that reads the (empty) lists.
        assert sum(n) == 0
        return
    assert sum(n) > 0
    for k in d.WANT_KINDS.get(name, ()):
        assert n[k] >= 1, "no item of kind %d" % k


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("it", d.PASS_ITS)
def test_a_sublist_longer_than_one_stride(it, spec):
    """256 threads stride over a sub-list: by pigeonhole over the 64 sub-lists of a kind, and by the geometry at S = 64"""
    kinds = d.case_kinds("long", it, spec)
    assert max(d.kind_counts(kinds)) > d.BIG_NL * 256
    assert d.longest_sublist(kinds) > 256


def test_kind_2_is_the_search_that_leaves_too_many_reads():
    """item_kind against the oracle's own mult4 on single items: flat weights, the heaviest base below a third of the total"""
    W = np.array([0.26, 0.25, 0.25, 0.24])
    tau = np.zeros((1, 4, 4), dtype=np.int64)
    tau[0, np.arange(4), np.arange(4)] = 1                                 # haplotype g carries base g
    eta = np.full((4, 4), 0.25)
    gamma = np.ascontiguousarray(W[None, :])
    for x, want in ((100, {-1}), (240, {2}), (300, {1}), (2000, {0})):
        counts = np.zeros((1, 1, 4), dtype=np.int64)
        counts[0, 0, 2] = x
        got = {int(d.item_kinds(counts, tau, gamma, eta, d.CTR_SEED, it, spec)[0, 0, 2]) for it in range(20) for spec in SPECS}
        # (the rarer outcome is the heaviest base, 0.26 of the weight) x = 100: mean 26, 74 +- 4 others <= 128; 240: mean 62.4 <= 64,
        # 178 +- 7 others; 300: mean 78 in (64, 128]; 2000: mean 520
        assert got == want, (x, got)


def test_rare_count():
    g = np.array([[0.5, 0.01, 0.0100001, 0.4799999], [0.9, 0.005, 0.002, 0.093]])
    assert d.rare_count(g) == 1                                            # 0.01 is (float)0.01 rounded down: at the bound
    assert d.rare_count(np.array([[0.99, 0.01]])) == 1 and d.rare_count(np.array([[0.98, 0.02]])) == 0
    assert d.rare_count(d.overfit_table()[2]) == 0


def test_stats_agg_is_unchanged_by_the_kinds_entry_point():
    counts, tau, gamma, eta = d.case_table("kind2")
    idx = cbind.onehot_to_idx(tau)
    mu, E = cbind.stats_agg(idx, gamma, eta, counts, d.CTR_SEED, 0)
    d.item_kinds(counts, tau, gamma, eta, d.CTR_SEED, 0)
    mu2, E2 = cbind.stats_agg(idx, gamma, eta, counts, d.CTR_SEED, 0)
    assert np.array_equal(mu, mu2) and np.array_equal(E, E2) and int(mu.sum()) == int(counts.sum()) == int(E.sum())
