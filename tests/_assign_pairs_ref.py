"""Numpy restatement of the sampled joint assignment with pair moves (include/desman_hip.h: dsm_assign_tau_sampled_pairs; DESIGN.md
sec. 8a-2), vectorised over positions and chains.  It shares no code with the kernel: the uniforms come from tests/_philox.py, the
logarithm and the exponential from numpy, and the sums over samples run in numpy's own order.  The single-site step and its uniforms
are those of tests/_assign_sampled_ref.py.

``close`` has that file's meaning, extended to pair steps: a pair step is close when its uniform lies within 2 delta of one of the
fifteen CDF edges, a pair-polish step when a candidate lies within 2 delta of the current pair's total without being equal to it bit
for bit, and a pair step that sets the best state is close when its two largest totals lie within 2 delta of each other without being
equal; delta = 1e-12 max(1, max |L_k|) of the step.

``mistake`` switches the keying of the PAIR uniforms only (the single-site ones stay right: tests/test_gpu_assign_sampled.py has
those), so a device that keyed its pair steps that way is told apart by its pair draws alone."""
import numpy as np

from _assign_sampled_ref import POLISH_CAP, _uniforms, candidates
from _philox import philox4x32_10

STREAM_APAR = 0x41504152                      # 'APAR' (dsm_device.h: DSM_STREAM_APAR); the pair steps of chain c draw from 'APAR' + c
MISTAKES = ("it + 1", "high key word dropped", "chains swapped", "g and h swapped in j")


def _pair_uniforms(keys, pos, t, G, mistake):
    """[N][4][G][G] uniforms of the pair pass of sweep t ([..][g][h]; g < h is used)"""
    N = len(pos)
    keys = np.asarray(keys, dtype=np.uint64).copy()
    if mistake == "high key word dropped":
        keys[:, 1] = 0
    if mistake == "it + 1":
        t = t + 1
    g = np.arange(G, dtype=np.uint64)[:, None]
    h = np.arange(G, dtype=np.uint64)[None, :]
    gh = (h * np.uint64(G) + g) if mistake == "g and h swapped in j" else (g * np.uint64(G) + h)
    j = pos.astype(np.uint64)[:, None, None, None] * np.uint64(G * G) + gh[None, None, :, :]
    j = np.broadcast_to(j, (N, 4, G, G))
    c = np.arange(4, dtype=np.uint64)
    if mistake == "chains swapped":
        c = c[::-1].copy()
    stream = np.broadcast_to((np.uint64(STREAM_APAR) + c)[None, :, None, None], (N, 4, G, G))
    ctr = np.stack([j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), np.full((N, 4, G, G), t, dtype=np.uint64), stream], axis=4)
    key = np.broadcast_to(keys[:, None, None, None, :], (N, 4, G, G, 2)).reshape(-1, 2)
    return philox4x32_10(ctr.reshape(-1, 4), key)[:, 0].astype(np.float64).reshape(N, 4, G, G) / 4294967296.0


def pair_candidates(X, gamma, eta, state, g, h):
    """L [..][16] of the candidates k = 4 a + a' of the pair (g, h); X [N][S][4] float counts, state [N][C][G]"""
    G = gamma.shape[1]
    m = np.zeros(state.shape[:2] + (gamma.shape[0], 4))                     # [N][C][S][a]
    for k in range(G):
        if k != g and k != h:
            m = m + (state[:, :, k, None] == np.arange(4))[:, :, None, :] * gamma[None, None, :, k, None]
    rest = ((m[..., 0, None] * eta[0] + m[..., 1, None] * eta[1]) + m[..., 2, None] * eta[2]) + m[..., 3, None] * eta[3]    # [N][C][S][b]
    with_g = rest[:, :, :, None, :] + eta[None, None, None, :, :] * gamma[None, None, :, g, None, None]                      # [N][C][S][a][b]
    pr = with_g[:, :, :, :, None, :] + eta[None, None, None, None, :, :] * gamma[None, None, :, h, None, None, None]         # [N][C][S][a][a'][b]
    seen = (X > 0)[:, None, :, None, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(seen, X[:, None, :, None, None, :] * np.log(pr), 0.0)
    L = term.sum(axis=(2, 5))                                               # [N][C][a][a']
    return L.reshape(L.shape[:2] + (16,))


def assign_pairs_numpy(counts, gamma, eta, seed, burn, kept, pair_every=0, mistake=None):
    """the outputs of dsm_assign_tau_sampled_pairs as a dict, plus conf_count, lscale and close as assign_sampled_numpy returns them and
    ends [N][T][4][G], the kept end-of-sweep states.
    ``seed`` may be a sequence of R seeds: every array gains a leading axis [R] (close stays one number)."""
    counts = np.asarray(counts, dtype=np.int64)
    gamma, eta = np.asarray(gamma, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    seeds = [int(s) for s in np.atleast_1d(np.asarray(seed, dtype=object))]
    R, N0 = len(seeds), counts.shape[0]
    keys = np.repeat(np.array([[s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF] for s in seeds], dtype=np.uint64), N0, axis=0)
    out = _run(np.tile(counts, (R, 1, 1)), np.tile(np.arange(N0), R), keys, gamma, eta, int(burn), int(kept), int(pair_every), mistake)
    if np.ndim(seed) == 0:
        return out
    return {k: (v if k == "close" else v.reshape((R, N0) + v.shape[1:])) for k, v in out.items()}


def _absmax(L):
    return np.where(np.isfinite(L), np.abs(L), 0.0).max(axis=-1)


def _run(counts, pos, keys, gamma, eta, B, T, E, mistake):
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
        U = _uniforms(keys, pos, t, G, None)
        for g in range(G):
            L = candidates(X, gamma, eta, state, g)                          # [N][4][4]
            mx = L.max(axis=2)
            live = mx > -np.inf
            with np.errstate(invalid="ignore", over="ignore"):
                e = np.where(np.isneginf(L), 0.0, np.exp(L - np.where(live, mx, 0.0)[..., None]))
            tot = ((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3]
            q = np.where(live[..., None], e / np.where(live, tot, 1.0)[..., None], 0.0)
            cdf = np.cumsum(q[..., :3], axis=2)
            u = U[:, :, g]
            a = (u[..., None] >= cdf).sum(axis=2)
            a = np.where(live, a, state[:, :, g])
            absL = _absmax(L)
            delta = 1e-12 * np.maximum(1.0, absL)
            near = (np.abs(cdf - u[..., None]) <= 2 * delta[..., None]).any(axis=2)
            close += int((near & live).sum())
            lscale = np.maximum(lscale, absL.max(axis=1))
            state[:, :, g] = a
            La = np.where(live, np.take_along_axis(L, a[..., None], axis=2)[..., 0], -np.inf)
            better = La > bestL
            bestL = np.where(better, La, bestL)
            bestS[better] = state[better]
            if t >= B:
                qsum[:, :, g, :] += q
        if E > 0 and (t + 1) % E == 0 and G > 1:
            UP = _pair_uniforms(keys, pos, t, G, mistake)
            for g in range(G):
                for h in range(g + 1, G):
                    L = pair_candidates(X, gamma, eta, state, g, h)          # [N][4][16]
                    mx = L.max(axis=2)
                    live = mx > -np.inf
                    with np.errstate(invalid="ignore", over="ignore"):
                        e = np.where(np.isneginf(L), 0.0, np.exp(L - np.where(live, mx, 0.0)[..., None]))
                    tot = np.zeros(e.shape[:2])
                    for k in range(16):
                        tot = tot + e[..., k]
                    q = np.where(live[..., None], e / np.where(live, tot, 1.0)[..., None], 0.0)
                    cdf = np.zeros(q.shape[:2] + (15,))
                    run = np.zeros(q.shape[:2])
                    for k in range(15):
                        run = run + q[..., k]
                        cdf[..., k] = run
                    u = UP[:, :, g, h]
                    kn = (u[..., None] >= cdf).sum(axis=2)
                    # (an edge below its predecessor cannot occur: q >= 0, so the count above is the first k with u < cdf_k)
                    kn = np.where(live, kn, 4 * state[:, :, g] + state[:, :, h])
                    absL = _absmax(L)
                    delta = 1e-12 * np.maximum(1.0, absL)
                    near = (np.abs(cdf - u[..., None]) <= 2 * delta[..., None]).any(axis=2)
                    close += int((near & live).sum())
                    lscale = np.maximum(lscale, absL.max(axis=1))
                    # best-state tracking looks at all sixteen: the largest total, the lowest k among equals
                    kmax = np.argmax(L, axis=2)
                    better = mx > bestL
                    top = np.sort(L, axis=2)
                    with np.errstate(invalid="ignore"):
                        near_top = (top[..., 15] - top[..., 14] <= 2 * delta) & (top[..., 15] != top[..., 14])
                    close += int((near_top & better).sum())
                    bestL = np.where(better, mx, bestL)
                    state[:, :, g] = kmax >> 2
                    state[:, :, h] = kmax & 3
                    bestS[better] = state[better]
                    state[:, :, g] = kn >> 2
                    state[:, :, h] = kn & 3
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
    # polish: rounds of (coordinate ascent to its fixed point, one pass of pair ascent) until a pair pass changes nothing; the
    # coordinate sweeps and pair passes that changed something number at most POLISH_CAP together: the polish of a position ends with
    # the POLISH_CAP-th of them, whichever kind it is.  E = 0: the one ascent.
    rows = np.arange(N)
    open_ = ~dead
    nsw = np.zeros(N, dtype=np.int64)
    while open_.any():
        active = open_.copy()
        while active.any():
            changed = np.zeros(N, dtype=bool)
            for g in range(G):
                L = candidates(X, gamma, eta, cur[:, None, :], g)[:, 0, :]     # [N][4]
                d = cur[:, g]
                Ld = L[rows, d]
                best, a = Ld.copy(), d.copy()
                for k in range(4):
                    up = L[:, k] > best
                    best = np.where(up, L[:, k], best)
                    a = np.where(up, k, a)
                delta = 1e-12 * np.maximum(1.0, _absmax(L))
                with np.errstate(invalid="ignore"):
                    tie = (np.abs(L - Ld[:, None]) <= 2 * delta[:, None]) & (L != Ld[:, None])
                close += int((tie.any(axis=1) & active).sum())
                move = active & (a != d)
                cur[move, g] = a[move]
                changed |= move
                curL = np.where(active, best, curL)
            nsw += active & changed
            capped = active & changed & (nsw >= POLISH_CAP)
            open_ &= ~capped
            active = active & changed & ~capped
        if E == 0:
            break
        moved = np.zeros(N, dtype=bool)
        for g in range(G):
            for h in range(g + 1, G):
                L = pair_candidates(X, gamma, eta, cur[:, None, :], g, h)[:, 0, :]       # [N][16]
                k0 = 4 * cur[:, g] + cur[:, h]
                L0 = L[rows, k0]
                best, kn = L0.copy(), k0.copy()
                for k in range(16):
                    up = L[:, k] > best
                    best = np.where(up, L[:, k], best)
                    kn = np.where(up, k, kn)
                delta = 1e-12 * np.maximum(1.0, _absmax(L))
                with np.errstate(invalid="ignore"):
                    tie = (np.abs(L - L0[:, None]) <= 2 * delta[:, None]) & (L != L0[:, None])
                close += int((tie.any(axis=1) & open_).sum())
                move = open_ & (kn != k0)
                cur[move, g] = kn[move] >> 2
                cur[move, h] = kn[move] & 3
                moved |= move
                curL = np.where(open_, best, curL)
        nsw += open_ & moved
        open_ &= moved & (nsw < POLISH_CAP)
    count = (ends == cur[None, :, None, :]).all(axis=3).sum(axis=(0, 2))    # [N]
    count = np.where(dead, 0, count)
    marg = (((qsum[:, 0] + qsum[:, 1]) + qsum[:, 2]) + qsum[:, 3]) / (4.0 * T)
    spread = ((qsum.max(axis=1) - qsum.min(axis=1)) / float(T)).max(axis=(1, 2))
    z = dead[:, None]
    return dict(map_state=np.where(z, 0, cur).astype(np.uint8), map_ll=curL, conf=count / (4.0 * T), conf_count=count,
                marg=np.where(dead[:, None, None], 0.0, marg), spread=np.where(dead, 0.0, spread),
                draw_state=np.where(z, 0, state[:, 0, :]).astype(np.uint8), close=close, lscale=lscale,
                ends=np.ascontiguousarray(ends.transpose(1, 0, 2, 3)))      # [N][T][4][G]: the kept end-of-sweep states
