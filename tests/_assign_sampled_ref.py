"""Numpy restatement of the sampled joint assignment (include/desman_hip.h: dsm_assign_tau_sampled), vectorised over
positions and chains.  It shares no code with the kernel: the uniforms come from tests/_philox.py, the logarithm and the exponential
from numpy, and the sums over samples run in numpy's own order.

Besides the outputs of the call it returns ``close``: the number of decisions that fp64 rounding could legitimately take the other way
-- steps whose uniform lies within 2 delta of a CDF edge, and polish steps at which a candidate lies within 2 delta of the current base's
total without being equal to it bit for bit -- with delta = 1e-12 max(1, max |L_a|) of the step, the project's log-likelihood tolerance
(DESIGN.md sec. 8a).  A parity test asserts close == 0 for its input: then the device must take every decision the same way."""
import numpy as np

from _philox import philox4x32_10

STREAM_ASMP = 0x41534D50                      # 'ASMP' (dsm_device.h: DSM_STREAM_ASMP); chain c draws from stream 'ASMP' + c
POLISH_CAP = 64
MISTAKES = ("it + 1", "high key word dropped", "chains swapped")


def _uniforms(keys, pos, t, G, mistake):
    """[N][4][G] uniforms of sweep t for rows with position indices pos [N] and keys [N][2]"""
    N = len(pos)
    keys = np.asarray(keys, dtype=np.uint64).copy()
    if mistake == "high key word dropped":
        keys[:, 1] = 0
    if mistake == "it + 1":
        t = t + 1
    i = pos.astype(np.uint64)[:, None, None] * np.uint64(G) + np.arange(G, dtype=np.uint64)[None, None, :]
    i = np.broadcast_to(i, (N, 4, G))
    c = np.arange(4, dtype=np.uint64)
    if mistake == "chains swapped":
        c = c[::-1].copy()
    stream = np.broadcast_to((np.uint64(STREAM_ASMP) + c)[None, :, None], (N, 4, G))
    ctr = np.stack([i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), np.full((N, 4, G), t, dtype=np.uint64), stream], axis=3)
    key = np.broadcast_to(keys[:, None, None, :], (N, 4, G, 2)).reshape(-1, 2)
    return philox4x32_10(ctr.reshape(-1, 4), key)[:, 0].astype(np.float64).reshape(N, 4, G) / 4294967296.0


def candidates(X, gamma, eta, state, g):
    """L [..][4] of the four candidates of site g; X [N][S][4] float counts, state [N][C][G]"""
    G = gamma.shape[1]
    m = np.zeros(state.shape[:2] + (gamma.shape[0], 4))                     # [N][C][S][a]
    for h in range(G):
        if h != g:
            m = m + (state[:, :, h, None] == np.arange(4))[:, :, None, :] * gamma[None, None, :, h, None]
    rest = ((m[..., 0, None] * eta[0] + m[..., 1, None] * eta[1]) + m[..., 2, None] * eta[2]) + m[..., 3, None] * eta[3]    # [N][C][S][b]
    pr = rest[:, :, :, None, :] + eta[None, None, None, :, :] * gamma[None, None, :, g, None, None]                          # [N][C][S][a][b]
    seen = (X > 0)[:, None, :, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(seen, X[:, None, :, None, :] * np.log(pr), 0.0)
    return term.sum(axis=(2, 4))


def assign_sampled_numpy(counts, gamma, eta, seed, burn, kept, mistake=None):
    """the outputs of dsm_assign_tau_sampled as a dict, plus conf_count (conf as an integer out of 4 kept), lscale [N] (max |L_a| over
    the steps of a position, at least 1) and close (see above).  ``seed`` may be a sequence of R seeds: the R calls run side by side and
    every array gains a leading axis [R] (close stays one number)."""
    counts = np.asarray(counts, dtype=np.int64)
    gamma, eta = np.asarray(gamma, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    seeds = [int(s) for s in np.atleast_1d(np.asarray(seed, dtype=object))]
    R, N0 = len(seeds), counts.shape[0]
    keys = np.repeat(np.array([[s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF] for s in seeds], dtype=np.uint64), N0, axis=0)
    out = _run(np.tile(counts, (R, 1, 1)), np.tile(np.arange(N0), R), keys, gamma, eta, int(burn), int(kept), mistake)
    if np.ndim(seed) == 0:
        return out
    return {k: (v if k == "close" else v.reshape((R, N0) + v.shape[1:])) for k, v in out.items()}


def _run(counts, pos, keys, gamma, eta, B, T, mistake):
    N, G = counts.shape[0], gamma.shape[1]
    X = counts.astype(np.float64)
    state = np.broadcast_to(np.arange(4)[None, :, None], (N, 4, G)).copy()
    bestL = np.full((N, 4), -np.inf)
    bestS = np.zeros((N, 4, G), dtype=np.int64)
    qsum = np.zeros((N, 4, G, 4))
    ends = np.zeros((T, N, 4, G), dtype=np.int64)
    lscale = np.ones(N)
    close = 0
    for t in range(B + T):
        U = _uniforms(keys, pos, t, G, mistake)
        for g in range(G):
            L = candidates(X, gamma, eta, state, g)                          # [N][4][4]
            mx = L.max(axis=2)
            live = mx > -np.inf
            with np.errstate(invalid="ignore", over="ignore"):
                e = np.where(np.isneginf(L), 0.0, np.exp(L - np.where(live, mx, 0.0)[..., None]))
            tot = ((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3]
            q = np.where(live[..., None], e / np.where(live, tot, 1.0)[..., None], 0.0)
            c0 = q[..., 0]; c1 = c0 + q[..., 1]; c2 = c1 + q[..., 2]
            u = U[:, :, g]
            a = np.where(u < c0, 0, np.where(u < c1, 1, np.where(u < c2, 2, 3)))
            a = np.where(live, a, state[:, :, g])
            absL = np.where(np.isfinite(L), np.abs(L), 0.0).max(axis=2)
            delta = 1e-12 * np.maximum(1.0, absL)
            near = (np.abs(np.stack([c0, c1, c2], axis=2) - u[..., None]) <= 2 * delta[..., None]).any(axis=2)
            close += int((near & live).sum())
            lscale = np.maximum(lscale, absL.max(axis=1))
            state[:, :, g] = a
            La = np.where(live, np.take_along_axis(L, a[..., None], axis=2)[..., 0], -np.inf)
            better = La > bestL
            bestL = np.where(better, La, bestL)
            bestS[better] = state[better]
            if t >= B:
                qsum[:, :, g, :] += q
        if t >= B:
            ends[t - B] = state
    # the best state of the four chains: ties to the lowest chain
    curL = np.full(N, -np.inf)
    cur = np.zeros((N, G), dtype=np.int64)
    for c in range(4):
        better = bestL[:, c] > curL
        curL = np.where(better, bestL[:, c], curL)
        cur[better] = bestS[better, c]
    dead = np.isneginf(curL)
    # polish: arg-max candidate per site, ties keep the base, else the lowest a
    active = ~dead
    nsw = np.zeros(N, dtype=np.int64)
    while active.any():
        changed = np.zeros(N, dtype=bool)
        for g in range(G):
            L = candidates(X, gamma, eta, cur[:, None, :], g)[:, 0, :]         # [N][4]
            d = cur[:, g]
            Ld = L[np.arange(N), d]
            best, a = Ld.copy(), d.copy()
            for k in range(4):
                up = L[:, k] > best
                best = np.where(up, L[:, k], best)
                a = np.where(up, k, a)
            delta = 1e-12 * np.maximum(1.0, np.where(np.isfinite(L), np.abs(L), 0.0).max(axis=1))
            with np.errstate(invalid="ignore"):
                tie = (np.abs(L - Ld[:, None]) <= 2 * delta[:, None]) & (L != Ld[:, None])
            close += int((tie.any(axis=1) & active).sum())
            move = active & (a != d)
            cur[move, g] = a[move]
            changed |= move
            curL = np.where(active, best, curL)
        nsw += active
        active = active & changed & (nsw < POLISH_CAP)
    count = (ends == cur[None, :, None, :]).all(axis=3).sum(axis=(0, 2))    # [N]
    count = np.where(dead, 0, count)
    marg = (((qsum[:, 0] + qsum[:, 1]) + qsum[:, 2]) + qsum[:, 3]) / (4.0 * T)
    spread = ((qsum.max(axis=1) - qsum.min(axis=1)) / float(T)).max(axis=(1, 2))
    z = dead[:, None]
    return dict(map_state=np.where(z, 0, cur).astype(np.uint8), map_ll=curL, conf=count / (4.0 * T), conf_count=count,
                marg=np.where(dead[:, None, None], 0.0, marg), spread=np.where(dead, 0.0, spread),
                draw_state=np.where(z, 0, state[:, 0, :]).astype(np.uint8), close=close, lscale=lscale)
