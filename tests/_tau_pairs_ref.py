"""Numpy restatement of one pair pass of the main chain on a tau table (include/desman_hip.h: dsm_ctx_sample_tau_pairs; DESIGN.md
sec. 8i), vectorised over positions.  It shares no code with the kernel: the sixteen totals are tests/_assign_pairs_ref.py:
pair_candidates, the uniforms tests/_philox.py, the exponential numpy's, and the sums over samples run in numpy's own order.

The pass visits the pairs (g, h), g < h, in lexicographic order; step (v, g, h) draws the pair's two digits by inverse CDF over the
sixteen q_k, k = 4 a + a', with the uniform word 0 / 2^32 of Philox(counter = (lo32 j, hi32 j, it, 'TPAR'), key = (lo32, hi32) of the
chain's counter seed), j = v G^2 + g G + h.

``close`` [V] marks the positions with a step whose uniform lies within 2 delta of one of the fifteen CDF edges, delta = 1e-12 max(1,
max |L_k|) of the step: there fp64 rounding may legitimately decide the other way, and a parity test leaves the position out.

``mistake`` switches the keying, so that a device keyed that way is told apart."""
import numpy as np
from scipy import stats as st

from _assign_pairs_ref import pair_candidates
from _assign_sampled_ref import candidates
from _philox import philox4x32_10, tau_uniforms

STREAM_TPAR = 0x54504152                      # 'TPAR' (dsm_device.h: DSM_STREAM_TPAR)
STREAM_APAR = 0x41504152                      # 'APAR': the assign kernel's pair stream, here one of the mistakes
MISTAKES = ("it + 1", "high key word dropped", "g and h swapped in j", "stream APAR")
CLOSE_CAP = 0.01                              # a parity test asserts on the restatement alone that at most this share is close


def digits(onehot):
    """[V][G][4] one-hot -> [V][G] digits"""
    return np.argmax(np.asarray(onehot), axis=2).astype(np.int64)


def onehot(dig):
    d = np.asarray(dig, dtype=np.int64)
    out = np.zeros(d.shape + (4,), dtype=np.int64)
    np.put_along_axis(out, d[..., None], 1, axis=2)
    return out


def pair_uniforms(ctr_seed, it, V, G, mistake=None):
    """[V][G][G] uniforms of the pass keyed (ctr_seed, it) ([..][g][h]; g < h is used)"""
    lo, hi = int(ctr_seed) & 0xFFFFFFFF, (int(ctr_seed) >> 32) & 0xFFFFFFFF
    if mistake == "high key word dropped":
        hi = 0
    if mistake == "it + 1":
        it = (int(it) + 1) & 0xFFFFFFFF
    g = np.arange(G, dtype=np.uint64)[:, None]
    h = np.arange(G, dtype=np.uint64)[None, :]
    gh = (h * np.uint64(G) + g) if mistake == "g and h swapped in j" else (g * np.uint64(G) + h)
    j = np.arange(V, dtype=np.uint64)[:, None, None] * np.uint64(G * G) + gh[None]
    stream = STREAM_APAR if mistake == "stream APAR" else STREAM_TPAR
    ctr = np.stack([j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), np.full(j.shape, int(it), dtype=np.uint64),
                    np.full(j.shape, stream, dtype=np.uint64)], axis=3)
    return philox4x32_10(ctr.reshape(-1, 4), [lo, hi])[:, 0].astype(np.float64).reshape(V, G, G) / 4294967296.0


def pair_pass(counts, gamma, eta, tau, ctr_seed, it, mistake=None):
    """one pair pass: counts [V][S][4], tau [V][G] digits -> (new tau [V][G], changed digits, close [V] bool)"""
    gamma, eta = np.asarray(gamma, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    X = np.asarray(counts).astype(np.float64)
    V, G = X.shape[0], gamma.shape[1]
    state = np.array(tau, dtype=np.int64).reshape(V, 1, G)
    close = np.zeros(V, dtype=bool)
    nchange = 0
    if G < 2:
        return state[:, 0, :], 0, close
    U = pair_uniforms(ctr_seed, it, V, G, mistake)
    for g in range(G):
        for h in range(g + 1, G):
            L = pair_candidates(X, gamma, eta, state, g, h)[:, 0, :]         # [V][16]
            mx = L.max(axis=1)
            live = mx > -np.inf
            with np.errstate(invalid="ignore", over="ignore"):
                e = np.where(np.isneginf(L), 0.0, np.exp(L - np.where(live, mx, 0.0)[:, None]))
            tot = np.zeros(V)
            for k in range(16):
                tot = tot + e[:, k]
            q = np.where(live[:, None], e / np.where(live, tot, 1.0)[:, None], 0.0)
            cdf = np.zeros((V, 15))
            run = np.zeros(V)
            for k in range(15):
                run = run + q[:, k]
                cdf[:, k] = run
            u = U[:, g, h]
            kn = (u[:, None] >= cdf).sum(axis=1)
            old = 4 * state[:, 0, g] + state[:, 0, h]
            kn = np.where(live, kn, old)                                    # all sixteen -inf: the pair stays, its uniform is spent
            delta = 1e-12 * np.maximum(1.0, np.where(np.isfinite(L), np.abs(L), 0.0).max(axis=1))
            close |= live & (np.abs(cdf - u[:, None]) <= 2 * delta[:, None]).any(axis=1)
            nchange += int(((kn >> 2) != (old >> 2)).sum() + ((kn & 3) != (old & 3)).sum())
            state[:, 0, g] = kn >> 2
            state[:, 0, h] = kn & 3
    return state[:, 0, :], nchange, close


def single_site_sweep(counts, gamma, eta, tau, ctr_seed, it):
    """one single-site sweep in Philox tau mode (dsm_ctx_sample_tau after dsm_ctx_set_tau_rng(DSM_RNG_PHILOX)): the candidates of
    tests/_assign_sampled_ref.py, the keying of tests/_philox.py: tau_uniforms.  -> (new tau, changed digits, close [V])"""
    gamma, eta = np.asarray(gamma, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    X = np.asarray(counts).astype(np.float64)
    V, G = X.shape[0], gamma.shape[1]
    state = np.array(tau, dtype=np.int64).reshape(V, 1, G)
    U = tau_uniforms(ctr_seed, it, V, G).reshape(V, G)
    close = np.zeros(V, dtype=bool)
    nchange = 0
    for g in range(G):
        L = candidates(X, gamma, eta, state, g)[:, 0, :]                    # [V][4]
        mx = L.max(axis=1)
        live = mx > -np.inf
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.where(np.isneginf(L), 0.0, np.exp(L - np.where(live, mx, 0.0)[:, None]))
        tot = ((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3]
        q = e / np.where(live, tot, 1.0)[:, None]
        cdf = np.cumsum(q[:, :3], axis=1)
        u = U[:, g]
        a = (u[:, None] >= cdf).sum(axis=1)
        assert live.all()                                                   # (the tables of these tests have no dead step)
        delta = 1e-12 * np.maximum(1.0, np.where(np.isfinite(L), np.abs(L), 0.0).max(axis=1))
        close |= (np.abs(cdf - u[:, None]) <= 2 * delta[:, None]).any(axis=1)
        nchange += int((a != state[:, 0, g]).sum())
        state[:, 0, g] = a
    return state[:, 0, :], nchange, close


def joint_posterior3(counts1, gamma, eta):
    """the exact posterior over the 64 states of ONE position at G = 3 (state index 16 a_0 + 4 a_1 + a_2): counts1 [S][4]"""
    X = np.asarray(counts1, dtype=np.float64)[None]
    L = np.concatenate([pair_candidates(X, gamma, eta, np.array([[[0, 0, c]]]), 0, 1)[0, 0][:, None] for c in range(4)],
                       axis=1)                                              # [16 = 4 a_0 + a_1][a_2]
    L = L.reshape(-1)
    p = np.exp(L - L.max())
    return p / p.sum()


def chi2_threshold(df):
    """the 1 - 1e-6 quantile of chi-square with df degrees of freedom: a true law fails once in a million tables"""
    return float(st.chi2.ppf(1.0 - 1e-6, df))


def chi2_stat(index, pmf):
    """Pearson's statistic of the draws ``index`` (state numbers) against the exact pmf"""
    n = len(index)
    obs = np.bincount(np.asarray(index, dtype=np.int64), minlength=len(pmf)).astype(np.float64)
    exp = n * np.asarray(pmf)
    return float(((obs - exp) ** 2 / exp).sum())


def stationarity_case(V=4096):
    """G = 3, S = 4: V copies of one position with one read per sample under a smooth eta (0.4 I + 0.6 Dirichlet(50) rows), so that
    every one of the 64 states expects at least 5 of the V draws -- asserted by the users --, and a start per copy drawn from the exact
    posterior.  -> (counts [V][S][4], gamma, eta, start [V][3] digits, posterior [64])"""
    rs = np.random.RandomState(77)
    G, S = 3, 4
    gamma = rs.dirichlet(np.full(G, 2.0), size=S)
    eta = 0.6 * rs.dirichlet(np.full(4, 50.0), size=4) + 0.4 * np.eye(4)
    truth = np.array([0, 2, 3])
    p = np.einsum("sg,gb->sb", gamma, eta[truth])
    one = np.array([rs.multinomial(1, p[s]) for s in range(S)], dtype=np.int64)
    post = joint_posterior3(one, gamma, eta)
    idx = rs.choice(64, size=V, p=post)
    start = np.stack([idx >> 4, (idx >> 2) & 3, idx & 3], axis=1)
    return np.repeat(one[None], V, axis=0), gamma, eta, start, post
