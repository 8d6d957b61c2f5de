"""Every sweep tiling, rank class and LDS size of the accessory-gene kernels (desman_amd/csrc/genes.hip) against the
CPU oracle (oracle/ref_genes.py, which tests/test_oracle_golden.py pins to the reference).

gene_sweep_kernel<LPV, NSL> is picked from the sample count S (pick_tile): LPV lanes share a variant row, every lane
carries NSL samples; sweep_geometry then drops lane groups per workgroup until the LDS fits 64 KB.  Each case below
asserts, through dsm_genes_debug_tile, the tiling it was written for, so the table cannot drift away from the code
without a failure.  gene_nmft_kernel<GMAX> and kl_update_kernel<GMAX> (GMAX = 4, 8, 16, 32) have their cases here
and in tests/test_gpu_genes.py::test_kl_assign_matches_oracle."""
import numpy as np
import pytest

from _genes_util import _case, _device

pytestmark = pytest.mark.gpu

LDS_FIXED = (2 * 256 + 16) * 8          # log table [256] double2 + epsilon [16]


def sweep_geometry(S, G, lpv, nsl):
    """lane groups per workgroup and dynamic LDS of a sweep launch, as genes.hip: sweep_geometry decides them"""
    tile = G * lpv * nsl * 8
    gpb = 256 // lpv
    while gpb > 1 and LDS_FIXED + gpb * tile > 64 * 1024:
        gpb >>= 1
    return gpb, LDS_FIXED + gpb * tile


# S, G, (LPV, NSL), groups per workgroup, LDS bytes, C, vmax, max_eta, epsilon entries set to 0 (None: the synthetic epsilon)
TILINGS = [
    (33, 5, (16, 3), 16, 34944, 6, 8, 2, None),               # 15 padded slots
    (48, 17, (16, 3), 8, 56448, 4, 8, 2, None),               # full tile; second uniform fetch at g = 16
    (16, 32, (16, 1), 8, 36992, 4, 8, 2, None),               # G at the limit: fetches at g = 0 and 16, the tau word is full
    (49, 4, (32, 2), 8, 20608, 6, 8, 2, ((0, 2), (2, 1))),    # 15 padded slots, zeros in epsilon
    (64, 8, (32, 2), 8, 36992, 8, 8, 2, None),                # the headline shape
    (96, 6, (32, 3), 8, 41088, 6, 8, 2, None),                # full tile
    (97, 3, (64, 2), 4, 16512, 6, 8, 2, None),                # 31 padded slots
    (128, 16, (64, 2), 2, 36992, 4, 8, 2, None),              # full; groups per workgroup halved once
    (193, 4, (64, 4), 4, 36992, 6, 8, 2, None),               # lower edge
    (256, 7, (64, 4), 4, 61568, 6, 8, 2, None),               # full
    (257, 5, (64, 6), 2, 34944, 6, 8, 2, ((0, 3), (1, 2))),   # slot 4 has one live lane, slot 5 none; zeros in epsilon
    (384, 12, (64, 6), 1, 41088, 4, 4, 2, None),              # full; one group per workgroup, LDS <= 64 KB
    (385, 3, (64, 8), 4, 53376, 6, 8, 2, None),               # slot 7 wholly padded
    (512, 32, (64, 8), 1, 135296, 4, 2, 2, None),             # both documented limits; one group per workgroup, LDS > 64 KB
    (24, 3, (16, 2), 16, 16512, 6, 8, 8, None),               # max_eta at its limit: eight copy-number states
]


def _zero_eps(eps, zeros):
    e = np.array(eps, dtype=np.float64, copy=True)
    for a, b in zeros:
        assert a != b
        e[a, b] = 0.0
    return np.ascontiguousarray(e / e.sum(axis=1)[:, None])


@pytest.mark.parametrize("S,G,tile,gpb,lds,C,vmax,max_eta,zeros", TILINGS, ids=["S%d-G%d" % (t[0], t[1]) for t in TILINGS])
def test_batched_update_every_tiling(S, G, tile, gpb, lds, C, vmax, max_eta, zeros):
    """as test_batched_update_edge_shapes: dsm_genes_update on explicit uniforms == eta_update_batched -- copy-number
    trajectory, final tau and MAP record exactly, log-likelihood trace to 1e-10 -- and, before it, the likelihood-only
    form of the sweep kernel (dsm_genes_loglik) against gene_loglik of the start state.

    Zeros in epsilon: a candidate base whose epsilon row has a zero makes a mixture value 0 wherever no other haplotype
    carries the gene (0 log 0 in every sample without reads of that base, padded sample slots included).  The entries
    sit in rows other than the last, the base such a step falls back to, so every state the chain keeps has finite
    values in the oracle: asserted below, ahead of the device call."""
    from oracle import ref_genes as rg
    from oracle import cbind
    k = _case(C, S, G, vmax, seed=S * 100 + G, mean_lo=0.5, mean_hi=3.0)
    if zeros is not None:
        k['eps'] = _zero_eps(k['eps'], zeros)
        assert (k['eps'] == 0.0).sum() == 2 and np.allclose(k['eps'].sum(axis=1), 1.0, rtol=0, atol=1e-15)
    rng = np.random.default_rng(S)
    Vtot = int(k['gene_off'][-1])
    eta0 = rng.integers(0, max_eta, size=(C, G))
    eta0[0, :] = 0                                           # a gene currently in no haplotype
    eta0[1, :] = 0; eta0[1, 0] = 1                           # a gene in exactly one
    tau0 = cbind.idx_to_onehot(rng.integers(0, 4, size=(Vtot, G)))
    n_iter = 2
    u_tau = rng.integers(0, 2 ** 32, size=(n_iter, G, 2, Vtot * G), dtype=np.uint32)
    u_eta = rng.random((n_iter, C, G))
    # ---- oracle first: its own values must be finite (zeros in epsilon: no 0 log 0, no log 0 anywhere)
    prior = rg.eta_log_prior(max_eta, 0.01)
    taus0 = [np.ascontiguousarray(tau0[k['gene_off'][c]:k['gene_off'][c + 1]]) for c in range(C)]
    eta = eta0.copy()
    taus = [t.copy() for t in taus0]
    eta_star = np.zeros_like(eta); llstar = np.zeros(C)
    with np.errstate(divide='raise', invalid='raise'):
        ll0 = np.array([rg.gene_loglik(eta0[c], taus0[c], k['variants'][c], k['cov'][c], k['gamma'], k['eps'], k['delta_gs'], prior)
                        for c in range(C)])
        ref_store, ref_trace = rg.eta_update_batched(eta, taus, k['variants'], k['gene_off'], k['cov'], k['gamma'], k['eps'],
                                                     k['delta_gs'], prior, n_iter, u_tau, u_eta, eta_star, llstar)
    assert np.isfinite(ll0).all() and np.isfinite(ref_trace).all() and np.isfinite(llstar).all()
    assert (ref_store != eta0[None]).any()                   # the chain moves
    # ---- device
    dev, _ = _device(k, eta0, tau0, max_eta)
    lpv, nsl, gpb_dev, lds_dev = dev.debug_tile()
    assert (lpv, nsl) == tile
    assert (gpb_dev, lds_dev) == sweep_geometry(S, G, lpv, nsl) == (gpb, lds)
    np.testing.assert_allclose(dev.loglik(), ll0, rtol=1e-10)
    store, trace = dev.update(n_iter, reset_star=True, u_tau_ext=u_tau, u_eta_ext=u_eta)
    eta_dev, tau_dev = dev.get_state()
    np.testing.assert_array_equal(store, ref_store)
    np.testing.assert_array_equal(tau_dev, np.concatenate(taus))
    np.testing.assert_allclose(trace, ref_trace, rtol=1e-10)
    star_dev, llstar_dev = dev.get_star()
    np.testing.assert_array_equal(star_dev, eta_star)


def test_debug_tile_needs_data_and_model():
    from desman_amd import _lib
    dev = _lib.Genes(0)
    with pytest.raises(_lib.DesmanHipError):
        dev.debug_tile()                                      # no data
    dev.set_data(np.zeros((4, 3, 4), dtype=np.int64), np.array([0, 1, 4], dtype=np.int32), np.ones((2, 3)))
    with pytest.raises(_lib.DesmanHipError):
        dev.debug_tile()                                      # no model
    dev.set_model(np.full((3, 2), 0.5), np.eye(4) * 0.96 + 0.01, np.ones((2, 3)), 2, np.array([-0.01, -4.6]), np.zeros(2), np.zeros(2))
    assert dev.debug_tile() == (16, 1, 16, LDS_FIXED + 16 * 2 * 16 * 8)


NMFT_SEED = {}                                               # (S, G) -> seed of the data and the starts; default below


@pytest.mark.parametrize("S,G", [(20, 8), (40, 9), (64, 16), (33, 17), (100, 32), (300, 32)])
def test_gene_nmft_start_every_rank_class(S, G):
    """per-gene factorize_tau, GMAX = 8, 16 (G = 9: blocked row sums), 16, 32, 32 and 32 with 79 KB of LDS: arg-max tau
    equals the oracle's, update counts within one.  A variant row is left out only where the oracle's own two largest
    tau entries of some haplotype are within 1e-9 relative (the device's log differs in the last bit): at most 1 %."""
    from oracle import ref_genes as rg
    from oracle import ref_numpy as rn
    from oracle import cbind
    C = 5
    seed = NMFT_SEED.get((S, G), S + G)
    k = _case(C, S, G, 2 if S >= 300 else 8, seed=seed, mean_lo=0.5, mean_hi=3.0)
    rng = np.random.default_rng(seed)
    eta0 = (rng.random((C, G)) < 0.6).astype(np.int64)
    eta0[:, 0] = 1
    eta0[0, :] = 0; eta0[0, G - 1] = 1                       # a gene in exactly one haplotype (the last)
    eta0[2, :] = 0                                           # a gene in none: skipped
    off = k['gene_off']
    Vtot = int(off[-1])
    if S == 300:
        assert (G * S + 32 + 256) * 8 > 64 * 1024             # the kernel's dynamic LDS: gamma [G][S], t1 [GMAX], red [256]
    # ---- oracle, with the factors it stops at (the near ties are judged on these)
    rs_dev, rs_ref, rs_chk = (np.random.RandomState(5) for _ in range(3))
    ref, tied = {}, 0
    for c in range(C):
        lo, hi = off[c], off[c + 1]
        if hi == lo or eta0[c].sum() == 0:
            continue
        gr = rg.mask_gamma(k['gamma'], eta0[c])
        t, n = rg.gene_nmft_tau(rs_ref, k['variants'][c], gr, G)
        F = cbind.nmft_freq(k['variants'][c])
        tf = rn.nmft_random_initialize_tau(rs_chk, hi - lo, G)
        n2, _ = cbind.nmft_factorize_tau(F, tf, np.ascontiguousarray(gr.T), 5000, 1.0e-5)
        assert n2 == n
        top = np.sort(tf.reshape(4, hi - lo, G), axis=0)[::-1]
        keep = ~((top[0] - top[1]) < 1.0e-9 * top[0]).any(axis=1)
        tied += int((~keep).sum())
        ref[c] = (t, n, keep)
    assert tied <= 0.01 * Vtot, (tied, Vtot)
    # ---- device
    dev, _ = _device(k, eta0, np.zeros((Vtot, G, 4), dtype=np.int64), 2)
    start = np.full((Vtot, 4, G), 0.25)
    for c in range(C):
        lo, hi = off[c], off[c + 1]
        if hi > lo and eta0[c].sum() > 0:
            d = rs_dev.dirichlet(np.full(4, 0.01), size=(hi - lo) * G).reshape(hi - lo, G, 4)
            start[lo:hi] = np.transpose(d, (0, 2, 1))
    n_dev = dev.nmft_tau(start)
    _, tau_dev = dev.get_state()
    assert len(ref) == 3
    for c in range(C):
        lo, hi = off[c], off[c + 1]
        if c not in ref:
            assert n_dev[c] == -1
            continue
        t, n, keep = ref[c]
        np.testing.assert_array_equal(tau_dev[lo:hi][keep], t[keep])
        assert abs(int(n_dev[c]) - n) <= 1, (c, n_dev[c], n)
