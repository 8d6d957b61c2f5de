"""What tests/test_ref_sweep_cpu.py and tests/test_gpu_ref_sweep.py share: the reference's own compiled sweep (oracle/cbind.py:
RefSampleTau -- sampletau/c_sample_tau.c unmodified, its GSL generator calls forwarded to the oracle's MT19937) as the thing to compare
with, and the tables on which a restatement of that file can go wrong: counts that the `(float)` cast of c_sample_tau.c:164 rounds,
operands that send log 0 = -inf and 0 * -inf = NaN through :136-169, one-hot rows with two 1s (:116-122).

Everything here is exact: tau equal element by element, nchange equal.  No tolerance appears anywhere."""
import math

import numpy as np
import pytest

from desman_amd.synth import synth_counts, random_state
from oracle import cbind

N_SWEEPS = 3


def reference():
    """the RefSampleTau object, or a skip -- only when the library AND the reference tree are both missing; with either one there a
    missing or failed build raises (cbind.RefSampleTau.build) and the test fails"""
    why = cbind.RefSampleTau.why_unavailable()
    if why is not None:
        pytest.skip(why)
    return cbind.RefSampleTau()


def ref_sweeps(ref, tau, pi, eta, counts, seed, n=N_SWEEPS):
    """n consecutive c_sample_tau calls on a copy of tau: c_initRNG, then c_setRNG(seed) unless seed is None (the stream
    gsl_rng_alloc leaves).  Returns the list of (tau after the call, nchange)."""
    ref.c_initRNG()
    if seed is not None:
        ref.c_setRNG(seed)
    t = np.ascontiguousarray(tau, dtype=np.int64).copy()
    out = []
    for _ in range(n):
        nch = ref.c_sample_tau(t, pi, eta, counts)
        out.append((t.copy(), nch))
    ref.c_freeRNG()
    return out


def assert_same(got, want, what=""):
    """lists of (tau, nchange): every sweep equal, element by element"""
    assert len(got) == len(want)
    for i, ((t, n), (tr, nr)) in enumerate(zip(got, want)):
        assert n == nr, "%s sweep %d: nchange %d, the reference's %d" % (what, i, n, nr)
        assert np.array_equal(t, tr), "%s sweep %d: %d of %d one-hot words differ from the reference's" % (what, i, int((t != tr).sum()), t.size)


def state(V, S, G, start, seed, shallow=None):
    """(counts, tau one-hot, pi, eta): synthetic counts with a random start or the state that generated them.  shallow (default: for
    the random start): about six reads per position over all samples -- flat conditionals, every uniform decides its draw; the usual
    depth (40 .. 500 reads per cell) gives sharp ones, candidate totals thousands of nats apart."""
    shallow = (start == "random") if shallow is None else shallow
    counts, tau_true, gamma_true = synth_counts(V, S, max(G, 2), seed=seed, depth_scale=6.0 / (270.0 * S) if shallow else 1.0)
    tau, pi, eta = random_state(V, S, G, seed=seed + 1)
    if start == "generating":
        tau = cbind.idx_to_onehot(np.ascontiguousarray(tau_true[:, :G]))
        pi = np.ascontiguousarray(gamma_true[:, :G] / gamma_true[:, :G].sum(axis=1, keepdims=True))
        eta = 0.96 * np.eye(4) + 0.01
    return np.ascontiguousarray(counts, dtype=np.int64), np.ascontiguousarray(tau, dtype=np.int64), np.ascontiguousarray(pi), np.ascontiguousarray(eta)


# --------------------------------------------------------------------------------------------------------------- the (float) cast
FLOAT_CAST_SEED = 20
_B = 1 << 24
# (reads of base 0, reads of base 1) of the deciding cell: the cast rounds 2^24 + 1 to 2^24, 2^24 + 3 to 2^24 + 4 (ties to even) and
# leaves 2^24 - 1; k 40000 + 16777217 is the deep-count row of tests/test_gpu_parity.py, next to its even neighbour
_PAIRS = [(_B + 1, _B), (_B, _B + 1), (_B + 3, _B + 2), (_B + 2, _B + 3), (_B - 1, _B + 1), (_B + 1, _B - 1), (_B + 3, _B + 1), (_B + 1, _B + 3)] + \
         [(k * 40000 + 16777217, k * 40000 + 16777216) for k in (1, 2, 3, 4)] + [(k * 40000 + 16777216, k * 40000 + 16777217) for k in (1, 2, 3, 4)]


def float_cast_table():
    """A table whose step g = 0 is decided by the cast.  Haplotype 0 chooses between bases 0 and 1, the other two sit on bases 2 and 3,
    whose error rows treat bases 0 and 1 alike; one cell per position carries ~2^24 reads of base 0 and of base 1, every other cell the
    same number of each.  Candidates 0 and 1 then differ by (x0 - x1) log(p_hi / p_lo) of the deep cell alone -- with x0 - x1 = 1 that is
    odds of about 2 : 1 in exact arithmetic and 1 : 1 after the cast (or 4 : 1 where the cast doubles the difference)."""
    V, S, G = 32, 17, 3
    rng = np.random.default_rng(5)
    eta = np.array([[0.60, 0.30, 0.05, 0.05], [0.30, 0.60, 0.05, 0.05], [0.02, 0.02, 0.90, 0.06], [0.02, 0.02, 0.06, 0.90]])
    pi = np.ascontiguousarray(rng.dirichlet([5.0, 3.0, 2.0], size=S))
    idx = np.stack([np.arange(V) % 2, np.full(V, 2), np.full(V, 3)], axis=1).astype(np.uint8)
    counts = np.zeros((V, S, 4), dtype=np.int64)
    pair = rng.integers(0, 6, size=(V, S))
    counts[:, :, 0] = counts[:, :, 1] = pair
    counts[:, :, 2:] = rng.integers(0, 6, size=(V, S, 2))
    for v in range(V):
        counts[v, v % S, 0], counts[v, v % S, 1] = _PAIRS[v % len(_PAIRS)]
    return counts, cbind.idx_to_onehot(idx), pi, np.ascontiguousarray(eta)


def numpy_sweep(tau, pi, eta, counts, u, cast):
    """One sweep of c_sample_tau.c:130-188 in plain numpy fp64, with the counts through float32 first (cast=True) or as exact doubles.
    Returns (new digits [V,G], for every step the distance of u from the nearest of the three cdf edges)."""
    idx = cbind.onehot_to_idx(tau).astype(np.int64)
    V, G = idx.shape
    x = counts.astype(np.float32).astype(np.float64) if cast else counts.astype(np.float64)
    dist = np.empty((V, G))
    for v in range(V):
        for g in range(G):
            rest = sum(eta[idx[v, h]][None, :] * pi[:, h, None] for h in range(G) if h != g) if G > 1 else np.zeros((pi.shape[0], 4))
            lp = np.array([(x[v] * np.log(rest + eta[a][None, :] * pi[:, g, None])).sum() for a in range(4)])
            p = np.exp(lp - lp.max())
            p /= p.sum()
            edges = np.cumsum(p)[:3]
            idx[v, g] = int((u[v * G + g] >= edges).sum())
            dist[v, g] = np.abs(u[v * G + g] - edges).min()
    return idx, dist


# --------------------------------------------------------------------------------------------------------------- degenerate operands
DEGENERATE = ["eta_identity", "eta_zero_row", "gamma_zeros", "gamma_eps", "no_reads", "all_neg_inf_and_nan"]


def degenerate_table(kind):
    """(counts, tau, pi, eta, MT19937 seed) of one case of DESIGN.md sec. 4 "Degenerate inputs"; every table has cells without reads of a
    base next to mixture values of exactly zero where the case has any"""
    V, S, G = 36, 17, 4
    rs = np.random.RandomState(100 + DEGENERATE.index(kind))
    counts, _, _ = synth_counts(V, S, G, seed=40 + DEGENERATE.index(kind), depth_scale=0.02)   # a few reads per cell: flat conditionals
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    counts[rs.rand(V, S) < 0.1] = 0                                   # cells without a read
    counts[rs.rand(V, S, 4) < 0.2] = 0                                # and without a read of one base: 0 * log(.)
    pi = rs.dirichlet(np.ones(G), size=S)
    eta = 0.96 * np.eye(4) + 0.01
    if kind == "eta_identity":                                        # exact zeros off the diagonal: log 0 wherever nobody carries the base
        eta = np.eye(4)
    elif kind == "eta_zero_row":
        eta[2, :] = 0.0
    elif kind == "gamma_zeros":                                       # Eta_Sampler.py:355-369: the gene's mask leaves exact zeros
        pi[:, [1, 3]] = 0.0
        pi = pi / pi.sum(axis=1, keepdims=True)
        pi[5, :] = 0.0                                                # and a sample nobody is in
        eta = np.eye(4) * 0.9 + np.array([[0, 0.1, 0, 0], [0.1, 0, 0, 0], [0, 0, 0, 0.1], [0, 0, 0.1, 0]])
    elif kind == "gamma_eps":
        pi[rs.rand(S, G) < 0.4] = 2.22e-16
    elif kind == "no_reads":
        counts[::2] = 0
        counts[1] = 0
    elif kind == "all_neg_inf_and_nan":
        # one haplotype carries everything and eta is the identity: a candidate's mixture is 1 at its own base and exactly 0 elsewhere.
        # Even positions have reads of all four bases in every sample (every candidate total is -inf, the softmax is NaN throughout and
        # the walk ends on the forced last edge); odd positions miss a base somewhere (0 * -inf = NaN inside a total).
        eta = np.eye(4)
        pi = np.zeros((S, G)); pi[:, 0] = 1.0
        counts = rs.randint(1, 30, size=(V, S, 4)).astype(np.int64)
        counts[1::2, :, :][rs.rand(V // 2, S, 4) < 0.3] = 0
    tau = cbind.idx_to_onehot(rs.randint(4, size=(V, G)).astype(np.uint8))
    return counts, tau, np.ascontiguousarray(pi), np.ascontiguousarray(eta), 900 + DEGENERATE.index(kind)


# --------------------------------------------------------------------------------------------------------------- u on a cdf edge
def eta_with_first_edge_at(u):
    """An error matrix for a table of ONE read (base 0, one sample, one haplotype) whose first cdf edge is the double u exactly, for
    0.5 < u < 0.7.  Candidate 0 has total log 1 = 0, candidate 1 log t, candidates 2 and 3 log 0 = -inf, so normaliseLog4
    (c_sample_tau.c:48-70) leaves p0 = 1 / (0 + 1 + exp(log t) + 0 + 0); t is searched, a few ulps around 1 / u - 1, with the same libm
    (math.log, math.exp) until that expression equals u bit for bit.  sample4's `u < edge` then passes the first edge and returns 1; a
    `<=` would return 0."""
    assert 0.5 < u < 0.7
    t = 1.0 / u - 1.0
    lo = t
    for _ in range(64):
        lo = math.nextafter(lo, 0.0)
    for _ in range(129):
        s = 0.0 + 1.0
        s += math.exp(math.log(lo))
        if 1.0 / s == u:
            eta = np.full((4, 4), 0.1)                                # bases without a read: 0 * log 0.1, no NaN
            eta[:, 0] = [1.0, lo, 0.0, 0.0]
            return eta
        lo = math.nextafter(lo, 1.0)
    raise AssertionError("no t within 64 ulps puts the first edge on u = %r" % u)
