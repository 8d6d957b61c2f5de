"""The definition of dsm_ctx_trace_ppc (include/desman_hip.h) restated in numpy, for the tests: posterior predictive
p-values per sample and per position from replicate tables drawn at stored iterations.  It shares no code with the kernel: Philox comes
from tests/_philox.py, xoshiro128+ and everything else stands here.

A cell of up to C reads is drawn read by read from 32-bit words against integer thresholds -- adds, multiplies, one division,
conversions and compares only -- so its x_rep are the device's, bit for bit; the sums T run in the definition's order (``tiling``), so
the comparisons T_rep >= T_obs come out the same way.  A deeper cell is drawn by numpy's binomial (``rng``): the same law, other draws."""
import numpy as np

from _philox import philox4x32_10

STREAM_PPCR = 0x50504352                      # 'PPCR' (dsm_device.h: DSM_STREAM_PPCR)
MAX_R = 1024                                  # DSM_PPC_MAX_R: the counter word of (t, r) is t * MAX_R + r
READS = 128                                   # DSM_PPC_READS


def tiling(S):
    """(lanes per position, sample slots per lane) for S samples"""
    lpv = 1
    while lpv < 64 and lpv < S:
        lpv *= 2
    need = (S + 63) // 64
    return lpv, (1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8)


def cell_p(tau_digits, gamma, eta):
    """p [V, S, 4] of one iteration, in the order of check.cell_terms: g ascending into the four mixture weights, then the true bases"""
    d = np.asarray(tau_digits, dtype=np.int64)
    gamma, eta = np.asarray(gamma, dtype=np.float64), np.asarray(eta, dtype=np.float64).reshape(4, 4)
    V, S = d.shape[0], gamma.shape[0]
    m = np.zeros((4, V, S))
    for g in range(d.shape[1]):
        for a in range(4):
            m[a] += np.where((d[:, g] == a)[:, None], gamma[None, :, g], 0.0)
    return np.stack([((m[0] * eta[0, b] + m[1] * eta[1, b]) + m[2] * eta[2, b]) + m[3] * eta[3, b] for b in range(4)], axis=2)


def pearson(x, p):
    """X [V, S] of the tables x [V, S, 4] against p: 0 for an empty cell, +inf where p_b = 0 < x_b"""
    x = np.asarray(x, dtype=np.float64)
    N = x.sum(axis=2)
    X = np.zeros(N.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(4):
            e = N * p[:, :, b]
            dl = x[:, :, b] - e
            X += np.where(p[:, :, b] > 0, dl * dl / e, np.where(x[:, :, b] > 0, np.inf, 0.0))
    return np.where(N > 0, X, 0.0)


def sum_over_samples(X):
    """T_v [V] = sum_s X[v][s]: lane l adds its samples l, l + L, ... in ascending order, the lanes meet by the xor butterfly"""
    V, S = X.shape
    lpv, nsl = tiling(S)
    pad = np.zeros((V, lpv * nsl))
    pad[:, :S] = X
    lane = np.zeros((V, lpv))
    for j in range(nsl):
        lane = lane + pad[:, j * lpv:(j + 1) * lpv]
    idx, off = np.arange(lpv), lpv // 2
    while off > 0:
        lane = lane + lane[:, idx ^ off]
        off //= 2
    return lane[:, 0]


def sum_over_positions(X):
    """T_s [S] = sum_v X[v][s]: the 256 / L positions of a tile in ascending order, then the tiles in ascending order"""
    V, S = X.shape
    ppb = 256 // tiling(S)[0]
    tiles = (V + ppb - 1) // ppb
    pad = np.zeros((tiles * ppb, S))
    pad[:V] = X
    pad = pad.reshape(tiles, ppb, S)
    part = np.zeros((tiles, S))
    for g in range(ppb):
        part = part + pad[:, g]
    tot = np.zeros(S)
    for z in range(tiles):
        tot = tot + part[z]
    return tot


def _xo_seed(words):
    s = [words[:, i].astype(np.uint32).copy() for i in range(4)]
    zero = (s[0] | s[1] | s[2] | s[3]) == 0
    s[0][zero] = 1
    return s


def _xo_next(s):
    """one step of xoshiro128+ on the state s (four uint32 arrays, updated in place); returns the words"""
    res = s[0] + s[3]
    t = s[1] << np.uint32(9)
    s[2] ^= s[0]
    s[3] ^= s[1]
    s[1] ^= s[2]
    s[0] ^= s[3]
    s[2] ^= t
    s[3][:] = (s[3] << np.uint32(11)) | (s[3] >> np.uint32(21))
    return res


def thresholds(p):
    """th [..., 3] uint64 of p [..., 4] by the read loop's rule, and c_3"""
    c0 = 0.0 + p[..., 0]
    c1 = c0 + p[..., 1]
    c2 = c1 + p[..., 2]
    c3 = c2 + p[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = 4294967296.0 / c3
        th = np.stack([c0 * scale, c1 * scale, c2 * scale], axis=-1)
    th = np.where(np.isnan(th), 0.0, np.minimum(np.floor(th), 4294967295.0))
    return th.astype(np.uint64), c3


def draw_replicate(N, p, key, t, r, rng=None, reads=READS):
    """x_rep [V, S, 4] of replicate r at stored iteration t: N [V, S] reads per cell, p [V, S, 4]"""
    V, S = N.shape
    N = N.astype(np.int64)
    th, c3 = thresholds(p)
    live = (N > 0) & (c3 > 0)
    x = np.zeros((V, S, 4), dtype=np.int64)
    j = np.arange(V * S, dtype=np.uint64)
    ctr = np.stack([j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), np.full_like(j, (int(t) * MAX_R + int(r)) & 0xFFFFFFFF),
                    np.full_like(j, STREAM_PPCR)], axis=1)
    shallow = (live & (N <= reads)).reshape(-1)
    if shallow.any():
        ids = np.flatnonzero(shallow)
        s = _xo_seed(philox4x32_10(ctr[ids], [int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF]))
        n, thr, pp = N.reshape(-1)[ids], th.reshape(-1, 3)[ids], p.reshape(-1, 4)[ids]
        k = np.zeros((ids.size, 3), dtype=np.int64)
        with np.errstate(over="ignore"):
            for i in range(int(n.max())):
                w = _xo_next(s).astype(np.uint64)
                k += ((w[:, None] < thr) & (i < n)[:, None])
        last = np.where(pp[:, 3] > 0, 3, np.where(pp[:, 2] > 0, 2, np.where(pp[:, 1] > 0, 1, 0)))
        for b in range(3):
            k[:, b] = np.where(last <= b, n, k[:, b])
        x.reshape(-1, 4)[ids] = np.stack([k[:, 0], k[:, 1] - k[:, 0], k[:, 2] - k[:, 1], n - k[:, 2]], axis=1)
    deep = live & (N > reads)
    if deep.any():
        assert rng is not None, "cells above %d reads need an rng" % reads
        tail = [p[..., 1] + (p[..., 2] + p[..., 3]), p[..., 2] + p[..., 3], p[..., 3]]
        rem = np.where(deep, N, 0)
        for b in range(3):
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(tail[b] > 0, p[..., b] / (p[..., b] + tail[b]), 1.0)
            q = np.where(p[..., b] > 0, q, 0.0)
            kb = rng.binomial(rem, np.clip(q, 0.0, 1.0))
            x[..., b] = np.where(deep, kb, x[..., b])
            rem = rem - kb
        x[..., 3] = np.where(deep, rem, x[..., 3])
    return x


def ppc(counts, tau_digits, gamma, eta, ts, R, key, rng=None, reads=READS):
    """What dsm_ctx_trace_ppc returns for the used iterations ``ts`` (their stored numbers; row i of tau_digits [n, V, G] -- or [V, G]: one
    tau for all --, gamma [n, S, G] and eta [n, 4, 4] belongs to ts[i]) and R replicates under the 64-bit key (counter seed xor salt):
    dict of ge_sample, ge_position, rep_sample, rep_position, obs_sample, obs_position"""
    counts = np.asarray(counts, dtype=np.int64)
    V, S = counts.shape[:2]
    tau_digits = np.asarray(tau_digits)
    N = counts.sum(axis=2)
    out = dict(ge_sample=np.zeros(S, dtype=np.int64), ge_position=np.zeros(V, dtype=np.int64), rep_sample=np.zeros((S, 2)),
               rep_position=np.zeros((V, 2)), obs_sample=np.zeros(S), obs_position=np.zeros(V))
    for i, t in enumerate(ts):
        p = cell_p(tau_digits if tau_digits.ndim == 2 else tau_digits[i], gamma[i], eta[i])
        Xo = pearson(counts, p)
        obs_s, obs_v = sum_over_positions(Xo), sum_over_samples(Xo)
        a_s, a_v = np.zeros((S, 2)), np.zeros((V, 2))
        for r in range(R):
            Xr = pearson(draw_replicate(N, p, key, t, r, rng=rng, reads=reads), p)
            Ts, Tv = sum_over_positions(Xr), sum_over_samples(Xr)
            out["ge_sample"] += Ts >= obs_s
            out["ge_position"] += Tv >= obs_v
            a_s[:, 0] += Ts; a_s[:, 1] += Ts * Ts
            a_v[:, 0] += Tv; a_v[:, 1] += Tv * Tv
        out["rep_sample"] += a_s
        out["rep_position"] += a_v
        out["obs_sample"] += obs_s
        out["obs_position"] += obs_v
    return out


# ---- the calibration and power cases of tests/test_check_reps_cpu.py and tests/test_gpu_check_reps.py ------------------------------------
CASE_V, CASE_S, CASE_G, CASE_R = 2000, 6, 3, 100
CASE_SEED = 20263                             # chosen once, on the restatement, among 20261 .. 20273 (test_check_reps_cpu.py records the margins it leaves)
CASE_KEY = 0x5EEDC0DE00000001
SPOILED = 2                                   # the sample whose A and C counts are swapped at every tenth position


def known_case(seed=CASE_SEED, spoiled=False):
    """(counts [V, S, 4], digits [1, V, G], gamma [1, S, G], eta [1, 4, 4]): a table drawn from the model at known parameters, a few
    hundred reads per cell; ``spoiled``: sample SPOILED has its A and C counts swapped at 10 % of the positions"""
    rs = np.random.RandomState(seed)
    V, S, G = CASE_V, CASE_S, CASE_G
    digits = rs.randint(0, 4, size=(1, V, G))
    gamma = rs.dirichlet(np.ones(G), size=(1, S))
    eta = (0.96 * np.eye(4) + 0.01)[None]
    p = cell_p(digits[0], gamma[0], eta[0])
    N = rs.randint(200, 500, size=(V, S))
    counts = np.zeros((V, S, 4), dtype=np.int64)
    for v in range(V):
        for s in range(S):
            counts[v, s] = rs.multinomial(N[v, s], p[v, s] / p[v, s].sum())
    if spoiled:
        rows = np.arange(0, V, 10)
        counts[rows, SPOILED, 0], counts[rows, SPOILED, 1] = counts[rows, SPOILED, 1].copy(), counts[rows, SPOILED, 0].copy()
    return counts, digits, gamma, eta


def calibration_figures(ge_position, n):
    """(the p-value of the position p-values' ten-bin chi-square against the uniform law, the share of them below 0.05, and the ends of
    the exact binomial band at 1 - 1e-6 of that share): with known parameters ge is uniform on 0 .. n, so p = ge / n < 0.05 has
    probability ceil(0.05 n) / (n + 1)"""
    import scipy.stats as st
    from _law import chi2_uniform
    ge = np.asarray(ge_position)
    p = ge / float(n)
    q = np.ceil(0.05 * n) / (n + 1.0)
    lo, hi = st.binom.ppf(5e-7, ge.size, q) / ge.size, st.binom.ppf(1.0 - 5e-7, ge.size, q) / ge.size
    return chi2_uniform(p, nbins=10), float((p < 0.05).mean()), float(lo), float(hi)
