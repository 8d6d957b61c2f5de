"""Case tables of tests/test_gpu_nmft_forms.py and tests/test_nmft_forms_cpu.py: one case per instantiation of the NMFT update
kernels (desman_amd/csrc/kernels_nmft.hip), with a Python restatement of the rules that pick the instantiation from the shape.
The GPU test asserts through Context.nmft_debug_path that every case takes the kernel it was written for, so neither this
restatement nor the tables can drift away from the code without a failure."""
import numpy as np

LOG_TAB_N = 256                     # log_table.h: DSM_LOG_TAB_N (double2 entries)
NM_XQ = 16 * 18                     # doubles per wavefront of the transposition tile (NM_XS = 18)
LDS_MAX = 160 * 1024
P_WAVES = 12                        # NMFT_P_WAVES: wavefronts of the persistent kernel's large form
N_UPD, N_UPD_TAU, N_UPD_P12 = 7, 5, 5    # updates of the first call (odd: the pair buffers end swapped), of the factorize_tau call after it
MIN_CHANGE = 1e-5


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the dispatch rules, restated
def mfma_shape(S, G):
    nt, kb = ceil_div(S, 16), ceil_div(G, 4)
    return (nt, kb) if 1 <= nt <= 8 and 1 <= kb <= 4 else None


def mfma_lds(nt, kb, fix):
    gp, spad = 4 * kb, 16 * nt
    loop = 2 * LOG_TAB_N + (1 if fix else 2) * gp * (spad + 1) + gp + 4 * 2 * 16 * gp + 4 * NM_XQ
    red = 4 if fix else 4 * (gp + 2) * spad
    return 8 * max(loop, red)


def split_lds(nt, kb, ncb, xpar):
    nq, gp, spad = 8 // ncb, 4 * kb, 16 * nt * ncb
    return 8 * (2 * LOG_TAB_N + 2 * gp * (spad + 1) + gp + nq * 3 * 16 * gp + 8 * (2 if xpar else 1) * NM_XQ + 8 + nq * gp)


def split_xpar(nt, kb, ncb):
    return split_lds(nt, kb, ncb, True) <= LDS_MAX


def wide_shape(S, G):
    tiles, kb = ceil_div(S, 16), ceil_div(G, 4)
    if tiles <= 8 or tiles > 32 or not 1 <= kb <= 4:
        return None
    for nt, ncb in ((3, 4), (4, 4), (5, 4), (6, 4), (8, 4)):
        if nt * ncb >= tiles:
            return (nt, kb, ncb) if split_lds(nt, kb, ncb, False) <= LDS_MAX else None
    return None


def persist_shape(V, S, G, fix, cus):
    """(NT, KB, wavefronts, workgroups, LDS) of the persistent loop, None where its gate says no"""
    m = mfma_shape(S, G)
    if m is None or m[0] > 6 or m[1] > 3:
        return None
    nt, kb = m
    nquad = ceil_div(V, 4)
    nwv = 4 if ceil_div(nquad, 4) <= cus else P_WAVES
    if nt > 4 and (nwv != 4 or not fix):
        return None
    grid = ceil_div(nquad, nwv)
    if grid < 2 or grid > cus:
        return None
    gp, spad, nout = 4 * kb, 16 * nt, G * S + G + 1
    lds = 8 * (2 * LOG_TAB_N + 2 * gp * (spad + 1) + gp + nwv * 2 * 16 * gp + nwv * max((gp + 2) * spad, NM_XQ) + ((nout + 1) & ~1) + 2 * G * S + 2)
    return (nt, kb, nwv, grid, lds) if lds <= LDS_MAX else None


def pass_b_tile(V, S, G):
    """(variants per workgroup step, workgroups, LDS) of nmft_pass_b_kernel"""
    sp = S + 1
    lds = lambda n: 8 * (G * sp + G + 8 * n * G + 4 * n * sp)
    vt = max(1, min(8, 8192 // (4 * sp)))
    while vt > 1 and lds(vt) > LDS_MAX:
        vt -= 1
    return vt, min(ceil_div(V, vt), 2048), lds(vt)


def pass_b_tile_unlowered(S, G):
    """LDS of pass B at the variants per step the sample count alone asks for (what the launcher refused above 160 KB)"""
    sp = S + 1
    vt = max(1, min(8, 8192 // (4 * sp)))
    return vt, 8 * (G * sp + G + 8 * vt * G + 4 * vt * sp)


def pass_a_form(S, G):
    spad = 32
    while spad < S and spad < 256:
        spad <<= 1
    return spad, (4 if G <= 4 else 8 if G <= 8 else 16 if G <= 16 else 32)


def expected_path(V, S, G, fix, cus, persist=True):
    """what Context.nmft_debug_path(fix) returns, but for the fields the CU count caps ('grid' is exact while the table is
    smaller than two update-kernel workgroups per CU, which every case here is) and the `gstep` flag"""
    blank = {"NT": 0, "KB": 0, "NCB": 0, "NWV": 0, "xpar": False, "VT": 0}
    p = persist_shape(V, S, G, fix, cus) if persist else None
    if p:
        return dict(blank, family="persist", NT=p[0], KB=p[1], NWV=p[2], grid=p[3], lds=p[4])
    m = mfma_shape(S, G)
    if m:
        nblk = ceil_div(ceil_div(V, 4), 4)
        assert nblk <= 2 * cus
        return dict(blank, family="mfma", NT=m[0], KB=m[1], grid=nblk, lds=mfma_lds(m[0], m[1], fix))
    w = wide_shape(S, G)
    if w:
        nt, kb, ncb = w
        nblk = ceil_div(ceil_div(V, 4), 8 // ncb)
        assert nblk <= cus
        xp = split_xpar(nt, kb, ncb)
        return dict(blank, family="split", NT=nt, KB=kb, NCB=ncb, grid=nblk, lds=split_lds(nt, kb, ncb, xp), xpar=xp)
    spad, gm = pass_a_form(S, G)
    vt, grid, lds = pass_b_tile(V, S, G)
    return dict(blank, family="two-pass", NT=spad, KB=gm, grid=grid, lds=lds, VT=vt)


# ---------------------------------------------------------------- the case tables
def edge_shape(nt, kb):
    """NT + KB even: 15 padded sample columns and a full haplotype block; odd: full sample tiles and three padded haplotype
    columns -- every NT sees both sample edges, every KB both haplotype edges"""
    return (16 * nt - 15, 4 * kb) if (nt + kb) % 2 == 0 else (16 * nt, 4 * kb - 3)


V_MFMA = 203                       # 51 quads, a three-variant tail, a three-wavefront last workgroup
MFMA_CASES = [(nt, kb) + edge_shape(nt, kb) for nt in range(1, 9) for kb in range(1, 5)]          # NT, KB, S, G
MFMA_IDS = ["mfma-NT%d-KB%d" % c[:2] for c in MFMA_CASES]
# the edge rule gives even NT at KB = 1 a single haplotype, whose runs stop after two updates: one padded-haplotype run of full
# length for KB = 1 (three haplotypes), on a tile count that keeps F in registers and on one that does not
MFMA_CASES += [(2, 1, 32, 3), (4, 1, 64, 3)]
MFMA_IDS += ["mfma-NT2-KB1-G3", "mfma-NT4-KB1-G3"]

P12_CASES = [(nt, kb) + edge_shape(nt, kb) for nt in range(1, 5) for kb in range(1, 4)]
P12_IDS = ["persist12-NT%d-KB%d" % c[:2] for c in P12_CASES]
P12_CASES += [(2, 1, 32, 3)]                       # (as above)
P12_IDS += ["persist12-NT2-KB1-G3"]


def v_p12(cus):
    return 16 * cus + 3            # one quad more than the four-wavefront form holds


V_SPLIT = 45                       # 12 quads, a one-variant tail, two quads per workgroup
SPLIT_S = [(3, 129), (3, 192), (4, 193), (4, 256), (5, 257), (5, 320), (6, 321), (6, 384), (8, 385), (8, 512)]      # NT, S: both edges
SPLIT_G = [1, 4, 5, 8, 9, 12, 13, 16]                                                                            # both edges of KB 1..4
SPLIT_ALL = [(nt, ceil_div(G, 4), S, G) for nt, S in SPLIT_S for G in SPLIT_G]
SPLIT_CASES = [c for c in SPLIT_ALL if wide_shape(c[2], c[3]) is not None]
SPLIT_REFUSED = [c for c in SPLIT_ALL if wide_shape(c[2], c[3]) is None]          # LDS: they take the two-pass kernels
SPLIT_CASES += [(3, 1, 129, 3), (8, 1, 512, 3)]    # G = 1 stops after two updates: KB = 1 with padded haplotype columns at full length
SPLIT_IDS = ["split-NT%d-KB%d-S%d-G%d" % c for c in SPLIT_CASES]

V_TWO = 77
TWO_CASES = ([(S, 17) for S in (1, 31, 33, 100, 200, 300, 512)] + [(S, 32) for S in (16, 64)] +
             [(S, G) for G in (13, 16) for S in (385, 512)])                                     # S, G
# the LDS limit of pass B at S = 512: 26 haplotypes are the most that fit at the three variants per step S = 512 asks for; above,
# the launcher lowers the variants per step (27: two, 32: one)
G_FIT_512 = max(G for G in range(1, 33) if pass_b_tile_unlowered(512, G)[1] <= LDS_MAX)
TWO_LDS_CASES = [(512, G_FIT_512), (512, 27), (512, 32)]


def two_id(S, G):
    spad, gm = pass_a_form(S, G)
    return "twopass-GM%d-SPAD%d-VT%d-S%d-G%d" % (gm, spad, pass_b_tile(V_TWO, S, G)[0], S, G)


TWO_IDS = [two_id(*c) for c in TWO_CASES]
TWO_LDS_IDS = [two_id(*c) for c in TWO_LDS_CASES]


# ---------------------------------------------------------------- data, starts, oracle
def case_seed(V, S, G):
    return 100003 * (V % 997) + 101 * S + G


def oracle_call(F, tau, gam, fix, max_iter, check=True):
    """one factorize / factorize_tau call of the C oracle on copies -> updates run, trace, factors, objective; everything finite
    (check = False: None instead of a failure where something is not)"""
    from oracle import cbind
    tc, gc = np.array(tau, copy=True), np.array(gam, copy=True)
    with np.errstate(invalid='raise', divide='raise'):
        n, tr = (cbind.nmft_factorize_tau if fix else cbind.nmft_factorize)(F, tc, gc, max_iter=max_iter, min_change=MIN_CHANGE)
        obj = cbind.nmft_objective(F, tc, gc)
    finite = np.isfinite(tr).all() and np.isfinite(tc).all() and np.isfinite(gc).all() and np.isfinite(obj)
    if not check and not finite:
        return None
    assert finite
    return n, tr, tc, gc, obj


_CASES = {}
OBJ_FLOOR = 1.0                     # ~1e10 times the rounding floor of the objective's sum (4 V S terms of at most half an ulp of 1 each)


def _second_call_ok(F, first):
    r = oracle_call(F, first[2], first[3], True, N_UPD_TAU, check=False)
    return r is not None and r[1].min() > OBJ_FLOOR


def case_data(V, S, G, K=1, n_first=N_UPD):
    """counts, F, K starts (tau0, gamma0) and the oracle's first call from each, refs[k][fix] = oracle_call(...): fixed seeds,
    computed once per case and shared (read only).  factorize_tau does not clamp, so from a raw Dirichlet(0.01) start a variant
    row can underflow to 0 / 0 in the reference itself; and with one sample and gamma fixed near a one-hot column the model can
    reproduce F exactly, the objective falling to its rounding floor (1.7e-16 at 203 x 1 x 4, second chain), where no relative
    bound on it means anything.  Chain k takes the first seed of base + 1 + k, + 1000, ... from which the oracle's first call and
    the factorize_tau call after it stay finite with every objective above OBJ_FLOOR."""
    key = (V, S, G, K, n_first)
    if key in _CASES:
        return _CASES[key]
    from desman_amd.synth import synth_counts
    from oracle import cbind
    from oracle import ref_numpy as rn
    seed = case_seed(V, S, G)
    counts, _, _ = synth_counts(V, S, G, seed=seed)
    F = cbind.nmft_freq(counts)
    starts, refs = [], []
    for k in range(K):
        for bump in range(20):
            tau0, gam0 = rn.nmft_random_initialize(np.random.RandomState(seed + 1 + k + 1000 * bump), V, S, G)
            ref = {fix: oracle_call(F, tau0, gam0, fix, n_first, check=False) for fix in (True, False)}
            if all(r is not None and r[1].min() > OBJ_FLOOR and _second_call_ok(F, r) for r in ref.values()):
                break
        else:
            raise AssertionError("no finite start for %r" % (key,))
        for a in (tau0, gam0, ref[True][2], ref[True][3], ref[False][2], ref[False][3]):
            a.setflags(write=False)
        starts.append((tau0, gam0)); refs.append(ref)
    for a in (counts, F):
        a.setflags(write=False)
    _CASES.clear()                                   # one case at a time: the tests of a case run back to back
    _CASES[key] = (counts, F, starts, refs)
    return _CASES[key]


def stops_early(G):
    """one haplotype: gamma is all ones and the first update is the fixed point, so the stop test fires after the second update (after
    the first in the factorize_tau call that follows) -- on the device at the same update.  Every other case with gamma updating
    runs all the updates it is asked for."""
    return G == 1
