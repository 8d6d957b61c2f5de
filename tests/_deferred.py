"""What stage 1 of the aggregated mu/E pass hands over, restated on the CPU (test data, not kernel code), and the cases the deferred-item
tests share (test_deferred_cpu.py asserts their preconditions without a GPU, test_gpu_deferred_items.py runs them).

  ntab_rep        kernels_stats.hip: stats_ntab_rep -- copies of the subset table
  first_rule      dsm_binom.h: s1_item / mult4<false> -- the items handed over by the mean of the rarer outcome alone (kinds 0 and 1):
                  a lower bound that needs no draw
  item_kinds      every item's kind (0, 1, 2 or -1) from the oracle's own twin of the lean item (oracle/stats_agg.c: item_kind), kind 2
                  -- the search was made and left more than DSM_XS = 128 reads of the other bases -- included: it depends on the draw
  rare_count      kernels_gibbs.hip: tau_rare_from_host -- haplotypes at or below (float)0.01 in every sample
  longest_sublist the geometry of the deferred lists while stage 1 runs one wavefront per position (S = 64)
"""
import functools

import numpy as np

from desman_amd.synth import synth_counts, random_state
from oracle import cbind

LEAN_CAP = 64.0                 # DSM_LEAN_CAP: stage 1 defers an item whose rarer outcome has a mean above this
BINV_MEAN_CAP = 128.0           # DSM_BINV_MEAN_CAP: ... onto the list of kind 0 (rejection sampler) above this, kind 1 (long search) below
XS = 128                        # DSM_XS
BIG_NL = 64                     # DSM_BIG_NL: sub-lists per kind
MARGIN = 1.0 + 1e-9             # (the device sums the weights in another order)
NT_RARE = np.float32(0.01)      # DSM_NT_RARE


def ntab_rep(V, S, G):
    """kernels_stats.hip: stats_ntab_rep -- copies of the subset table"""
    if 3.0 * V / (1 << G) <= 128.0:
        return 1
    lines = ((1 << G) * S * 4 + 63) // 64
    rep = 2
    while lines * rep < 384 and rep < 64 and 2 * rep * (1 << G) * S * 4 <= (64 << 20):
        rep *= 2
    return rep


def first_rule(counts, tau, gamma, eta, pooled=False):
    """Lower bound on the items stage 1 defers from the state (tau one-hot [V, G, 4], gamma, eta), by the rule of dsm_binom.h (mult4 /
    s1_item): the item (cell, observed base b) with count x and weights W[a] = eta[a, b] Gamma_a splits off the reads not of the heaviest
    base by one binomial, and is deferred when x w > DSM_LEAN_CAP, w = the smaller side's share of the weight (kind 0 above
    DSM_BINV_MEAN_CAP, else kind 1; items that go through and then find more than DSM_XS such reads are deferred too and not counted
    here: item_kinds).  pooled (spec 4): the counts of the positions with one tau word are summed in the word's lowest position first.
    Returns bool [entries, S, 4] x 2: deferred, of kind 0."""
    x = counts
    if pooled:
        _, first, inv = np.unique(np.argmax(tau, axis=2), axis=0, return_index=True, return_inverse=True)
        x = np.zeros((len(first),) + counts.shape[1:], dtype=np.int64)
        np.add.at(x, inv.reshape(-1), counts)
        tau = tau[first]
    gam = np.einsum("sg,vga->vsa", gamma, tau.astype(np.float64))
    W = eta[None, None, :, :] * gam[:, :, :, None]                # [v, s, true base a, observed base b]
    T, wm = W.sum(axis=2), W.max(axis=2)
    mean = x * np.minimum(T - wm, wm) / T
    return mean > LEAN_CAP * MARGIN, mean > BINV_MEAN_CAP * MARGIN


def handed_over(counts, tau, gamma, eta):
    """number of items the first rule hands over at this state"""
    return int(np.count_nonzero(first_rule(counts, tau, gamma, eta)[0]))


def item_kinds(counts, tau, gamma, eta, ctr_seed, it, spec=2):
    """int8 [V, S, 4]: the kind under which stage 1 hands each (position, sample, observed base) item over in the pass of iteration `it`
    under the counter key `ctr_seed` -- 0, 1, 2 -- or -1 (the oracle's twin of the lean item: cbind.stats_kinds)"""
    return cbind.stats_kinds(cbind.onehot_to_idx(tau), np.ascontiguousarray(gamma), np.ascontiguousarray(eta), counts, ctr_seed, it, spec=spec)


def kind_counts(kinds):
    """(items of kind 0, 1, 2)"""
    return tuple(int(np.count_nonzero(kinds == k)) for k in (0, 1, 2))


def rare_count(gamma):
    """kernels_gibbs.hip: tau_rare_from_host -- haplotypes whose largest abundance over the samples is <= (float)0.01"""
    return int(np.count_nonzero(np.asarray(gamma).max(axis=0).astype(np.float32) <= NT_RARE))


def longest_sublist(kinds):
    """items on the longest of the 3 x 64 sub-lists when stage 1 runs one wavefront per position (S = 64: one 64-lane chunk per position,
    fewer tasks than the persistent grid has wavefronts): workgroup = 4 positions, sub-list = kind x (workgroup mod 64)"""
    sub = (np.arange(kinds.shape[0]) // 4) % BIG_NL
    per = np.zeros((3, BIG_NL), dtype=np.int64)
    for k in range(3):
        np.add.at(per[k], sub, (kinds == k).sum(axis=(1, 2)))
    return int(per.max())


# ---------------------------------------------------------------- the shared cases
CTR_SEED = 0x0123456789ABCDEF
PASS_ITS = (0, 5)               # the iteration numbers the one-pass tests draw under


def _generating(shape, scale, seed, diag=0.96):
    """the table with the state it was generated from (test_gpu_big_launch_modes.py: _table)"""
    V, S, G = shape
    counts, tt, gg = synth_counts(V, S, G, seed, depth_scale=scale)
    tau = np.zeros((V, G, 4), dtype=np.int64)
    np.put_along_axis(tau, tt.astype(np.int64)[..., None], 1, axis=2)
    eta = diag * np.eye(4) + (1.0 - diag) / 4.0
    eta /= eta.sum(axis=1, keepdims=True)
    return counts, tau, np.ascontiguousarray(gg), eta


def _random(shape, scale, seed, state_seed):
    """the table with a random state: flat weights, the heaviest base often below half of the total"""
    V, S, G = shape
    counts, _, _ = synth_counts(V, S, G, seed, depth_scale=scale)
    return (counts,) + random_state(V, S, G, seed=state_seed)


def _flat(shape, scale, seed, state_seed):
    """the table with random_state's haplotypes at equal abundances and the symmetric error matrix: where the three haplotypes of a
    position carry three bases other than the observed one the three weights are EQUAL -- the heaviest base a third of the total"""
    V, S, G = shape
    counts, _, _ = synth_counts(V, S, G, seed, depth_scale=scale)
    tau, _, _ = random_state(V, S, G, seed=state_seed)
    return counts, tau, np.full((S, G), 1.0 / G), 0.96 * np.eye(4) + 0.01


# Kind 2 needs the search to be made (x q <= 64, q = the heaviest base's share of the weight, which is the rarer outcome: q < 1/2) and
# to leave x - k > 128 reads, k ~ Binomial(x, q): 128 / (1 - q) < x <= 64 / q, so q < 1/3 or barely above.  Three haplotypes give a
# cell at most three non-zero weights, q >= 1/3: at (64, 17, 3) only q within a few per cent of 1/3 and 185 <= x <= 192 will do.
# random_state's abundances and error matrix do not get there (240 000 states at six depths: 144 with such an item in one pass, none in
# all four passes), so the case takes random_state's haplotypes flat (_flat) at 3 x depth, where counts near 190 are common; with four
# haplotypes (S70) random_state itself does.
# name -> (shape, depth_scale, state, table seed, state seed); seeds and depths chosen on the CPU until the oracle meets the preconditions
# test_deferred_cpu.py asserts.  copies32 is not in the issue's table: by the restated rule (700, 20, 3) keeps 64 copies like (400, 5, 2)
# (10 lines x 32 = 320 < 384), so a third shape, smaller than (700, 20, 3), brings the second value of rep: 12 lines x 32 = 384.
CASES = {
    "copies":   ((400, 5, 2), 40.0, "generating", 7, None),         # (at 10 x depth the generating state hands nothing over: error reads
    "swizzle":  ((700, 20, 3), 40.0, "generating", 7, None),        # of a cell have a mean of at most ~50)
    "copies32": ((400, 24, 3), 40.0, "generating", 7, None),
    "kind2":    ((64, 17, 3), 3.0, "flat", 7, 9),
    "S1":       ((48, 1, 2), 40.0, "generating", 7, None),
    "G1":       ((48, 5, 1), 40.0, "generating", 7, None),
    "G9":       ((40, 17, 9), 40.0, "generating", 7, None),
    "S70":      ((32, 70, 4), 40.0, "random", 7, 71),
    "long":     ((400, 64, 8), 20.0, "random", 900, 600),
}
WANT_REP = {"copies": 64, "swizzle": 64, "copies32": 32, "kind2": 1, "S1": 1, "G1": 1, "G9": 1, "S70": 1, "long": 1}
WANT_KINDS = {"kind2": (0, 1, 2), "S70": (2,)}          # kinds the case is there for (every case: at least one item handed over)
CHAIN_CASES = ("copies", "kind2", "S1")


@functools.lru_cache(maxsize=None)
def case_table(name):
    shape, scale, state, seed, state_seed = CASES[name]
    if state == "generating":
        return _generating(shape, scale, seed)
    return (_flat if state == "flat" else _random)(shape, scale, seed, state_seed)


@functools.lru_cache(maxsize=None)
def case_kinds(name, it, spec):
    counts, tau, gamma, eta = case_table(name)
    return item_kinds(counts, tau, gamma, eta, CTR_SEED, it, spec)


# ---------------------------------------------------------------- the tables of the 130-iteration chains
def overfit_table():
    """(64, 2, 3): counts of two strains with few errors (0.2 % per wrong base, 4 x depth), started from the two strains and a third
    haplotype of random bases at 5 % in both samples: no rare haplotype at the start.  The chain leaves the spare haplotype the error
    reads only -- its abundance falls below (float)0.01 in both samples within the first 64 iterations (the CPU oracle's chain: rare
    from iteration ~60 on, 0.0006 at the end).  With more samples the largest of the spare abundances stays at 2 ... 6 % (S = 4 ... 17,
    six seeds each), so the table has two."""
    V, S, G = 64, 2, 3
    err = 0.002
    counts, tt, gg = synth_counts(V, S, 2, 12, eta=(1.0 - 4.0 * err) * np.eye(4) + err, depth_scale=4.0)
    rng = np.random.default_rng(5)
    idx = np.concatenate([tt.astype(np.int64), rng.integers(0, 4, size=(V, 1))], axis=1)
    tau = np.zeros((V, G, 4), dtype=np.int64)
    np.put_along_axis(tau, idx[..., None], 1, axis=2)
    gamma = np.concatenate([gg * 0.95, np.full((S, 1), 0.05)], axis=1)
    eta = 0.96 * np.eye(4) + 0.01
    return counts, tau, np.ascontiguousarray(gamma / gamma.sum(axis=1, keepdims=True)), eta
