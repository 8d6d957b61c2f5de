"""ctypes binding of libdesman_hip.so -- the only native boundary of the package.

The product path has NO CPU fallback: if the HIP library is missing, cannot be
loaded, or no gfx950 device is visible, every compute entry point raises.
Signatures mirror include/desman_hip.h one to one.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DESMAN_HIP_LIB: another build of the same library (A/B builds of scripts/dbg: `make -C desman_amd/csrc EXTRA=... LIBNAME=...`)
LIB_PATH = os.environ.get("DESMAN_HIP_LIB") or os.path.join(_HERE, "lib", "libdesman_hip.so")
AB_LIB_PATH = os.path.join(_HERE, "lib", "libdesman_hip_ab.so")     # the experiment build (`make -C desman_amd/csrc ab`): A/B switches compiled in
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "desman_hip.h")

DSM_OK = 0
RNG_MT19937, RNG_PHILOX = 0, 1
SND_STAR, SND_SELF, SND_GIVEN = 0, 1, 2     # DSM_SND_*: the reference of Context.trace_snd
STATS_AGG = 2        # version of the aggregated mu/E specification that runs by default (oracle/stats_agg.c); 3 = the table exp / log variant
K_NAMES = ("stats", "dirichlet", "tau", "finalize", "mt", "nmft_a", "nmft_gamma", "nmft_b", "stats2", "stats_big", "stats_pat")


class DesmanHipError(RuntimeError):
    pass


_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_vp, _i, _d = C.c_void_p, C.c_int, C.c_double

# name -> (restype, argtypes); every symbol include/desman_hip.h declares
SIGNATURES = {
    "dsm_last_error": (C.c_char_p, []),
    "dsm_device_count": (_i, []),
    "dsm_version": (C.c_char_p, []),
    "dsm_initRNG": (_i, []),
    "dsm_setRNG": (_i, [C.c_ulong]),
    "dsm_freeRNG": (_i, []),
    "dsm_sample_tau": (_i, [_i64p, _f64p, _f64p, _i64p, _i, _i, _i]),
    "c_initRNG": (None, []),
    "c_setRNG": (None, [C.c_ulong]),
    "c_freeRNG": (None, []),
    "c_sample_tau": (_i, [_i64p, _f64p, _f64p, _i64p, _i, _i, _i]),
    "dsm_getRNG_state": (_i, [_u32p]),
    "dsm_setRNG_state": (_i, [_u32p]),
    "dsm_ctx_create": (_i, [C.POINTER(_vp), _i]),
    "dsm_ctx_destroy": (_i, [_vp]),
    "dsm_ctx_sync": (_i, [_vp]),
    "dsm_ctx_set_counts": (_i, [_vp, _i64p, _i, _i]),
    "dsm_ctx_set_state": (_i, [_vp, _i64p, _f64p, _f64p, _i]),
    "dsm_ctx_get_state": (_i, [_vp, _vp, _vp, _vp]),
    "dsm_ctx_set_gamma_eta": (_i, [_vp, _vp, _vp]),
    "dsm_ctx_set_priors": (_i, [_vp, _d, _d, _d]),
    "dsm_ctx_seed": (_i, [_vp, C.c_ulong, C.c_uint64]),
    "dsm_ctx_set_tau_rng": (_i, [_vp, _i]),
    "dsm_ctx_get_mt_state": (_i, [_vp, _u32p]),
    "dsm_ctx_set_mt_state": (_i, [_vp, _u32p]),
    "dsm_mt_seed_state": (_i, [C.c_ulong, _u32p]),
    "dsm_ctx_debug_mt_fill": (_i, [_vp, C.c_size_t, _u32p]),
    "dsm_ctx_sample_tau": (_i, [_vp, C.POINTER(_i), _vp]),
    "dsm_ctx_sample_stats": (_i, [_vp, C.c_uint32, _u64p, _u64p]),
    "dsm_ctx_stats_spec": (_i, [_vp]),
    "dsm_ctx_sweep_stats": (_i, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _i]),
    "dsm_ctx_set_tau_screen": (_i, [_vp, _i]),
    "dsm_ctx_set_tau_neartie": (_i, [_vp, _i]),
    "dsm_ctx_set_big_launch": (_i, [_vp, _i]),
    "dsm_ctx_debug_big_lists": (_i, [_vp, _vp, _vp]),
    "dsm_ctx_set_nmft_fused": (_i, [_vp, _i]),
    "dsm_ctx_set_nmft_persist": (_i, [_vp, _i]),
    "dsm_ctx_tau_launch_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "dsm_ctx_debug_log2f": (_i, [_vp, _vp, _vp, C.c_size_t]),
    "dsm_debug_fdiv": (_i, [_i, _f64p, _f64p, _f64p, _i]),
    "dsm_release_device_caches": (_i, []),
    "dsm_ctx_force_stats_spec": (_i, [_vp, _i]),
    "dsm_ctx_debug_stage1": (_i, [_vp, C.c_uint32, _vp, _u64p]),
    "dsm_ctx_debug_binom": (_i, [_vp, _i, C.c_uint32, _f64p, C.c_uint64, _i, _u32p, _i]),
    "dsm_ctx_draw_gamma_eta": (_i, [_vp, C.c_uint32, _u64p, _u64p, _f64p, _f64p]),
    "dsm_ctx_loglik": (_i, [_vp, C.POINTER(_d), C.POINTER(_d)]),
    "dsm_ctx_gibbs_update": (_i, [_vp, _i]),
    "dsm_ctx_gibbs_update_fixed_tau": (_i, [_vp, _i, _i, _i]),
    "dsm_ctx_sample_tau_held": (_i, [_vp, _i, C.POINTER(_i)]),
    "dsm_ctx_gibbs_update_held_tau": (_i, [_vp, _i, _i, _i]),
    "dsm_ctx_set_pair_moves": (_i, [_vp, _i]),
    "dsm_ctx_get_pair_moves": (_i, [_vp, C.POINTER(_i)]),
    "dsm_ctx_sample_tau_pairs": (_i, [_vp, C.c_uint32, C.POINTER(_i)]),
    "dsm_pairtau_debug_path": (_i, [_i, _i, C.POINTER(_i)]),
    "dsm_ctx_debug_fixtau_pool": (_i, [_vp, C.POINTER(_i), _vp, _vp, _vp]),
    "dsm_ctx_debug_fixtau_sample_stats": (_i, [_vp, C.c_uint32, _u64p, _u64p]),
    "dsm_ctx_get_counters": (_i, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "dsm_ctx_set_counters": (_i, [_vp, C.c_uint64, C.c_uint32]),
    "dsm_ctx_get_screen_state": (_i, [_vp, _u32p]),
    "dsm_ctx_set_screen_state": (_i, [_vp, _u32p]),
    "dsm_ctx_gibbs_update_sharded": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "dsm_ctx_gibbs_update_sharded_comm": (_i, [_vp, _i, _i, _i, _vp]),
    "dsm_comm_unique_id": (_i, [_vp]),
    "dsm_comm_create": (_i, [C.POINTER(_vp), _vp, _i, _i, _i]),
    "dsm_comm_destroy": (_i, [_vp]),
    "dsm_comm_rank": (_i, [_vp]),
    "dsm_comm_world": (_i, [_vp]),
    "dsm_comm_allgather_f64": (_i, [_vp, _f64p, _f64p, C.c_size_t]),
    "dsm_comm_allreduce_f64": (_i, [_vp, _vp, C.c_size_t, _i]),
    "dsm_comm_barrier": (_i, [_vp]),
    "dsm_device_read": (_i, [_i, _vp, _vp, C.c_size_t]),
    "dsm_device_write": (_i, [_i, _vp, _vp, C.c_size_t]),
    "dsm_batch_gibbs_update": (_i, [C.POINTER(_vp), _i, _i]),
    "dsm_batch_update_tau": (_i, [C.POINTER(_vp), _i, _i, C.POINTER(_vp), C.POINTER(_vp)]),
    "dsm_batch_nmft_factorize": (_i, [C.POINTER(_vp), _i, _i, _d, _i, C.POINTER(_i), _vp]),
    "dsm_ctx_update_tau": (_i, [_vp, _i, _f64p, _f64p]),
    "dsm_ctx_get_trace": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "dsm_ctx_get_star": (_i, [_vp, _vp, _vp, _vp, C.POINTER(_d), C.POINTER(_i)]),
    "dsm_ctx_get_tau_sum": (_i, [_vp, _i64p]),
    "dsm_ctx_get_tau_at": (_i, [_vp, _i, _i64p]),
    "dsm_ctx_trace_snd": (_i, [_vp, _i, _vp, _i, _i, _i, _vp]),
    "dsm_ctx_get_tau_sum_perm": (_i, [_vp, _vp, _i, _i, _vp]),
    "dsm_ctx_debug_set_trace": (_i, [_vp, _vp, _i]),
    "dsm_ctx_trace_batch_stats": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "dsm_diag_debug_set_parts": (_i, [_i]),
    "dsm_ctx_trace_fit_stats": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "dsm_fit_debug_set_parts": (_i, [_i]),
    "dsm_fit_debug_path": (_i, [_vp, _i, C.POINTER(_i)]),
    "dsm_ctx_trace_ppc": (_i, [_vp, _i, _i, _i, _i, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsm_ppc_debug_set_parts": (_i, [_i]),
    "dsm_ppc_debug_set_chunk": (_i, [_i, _i]),
    "dsm_ppc_debug_path": (_i, [_vp, _i, _i, C.POINTER(_i)]),
    "dsm_ctx_debug_set_param_trace": (_i, [_vp, _vp, _vp, _i]),
    "dsm_ctx_trace_rb_marginals": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, C.POINTER(C.c_longlong)]),
    "dsm_rbtau_debug_path": (_i, [_i, _i, C.POINTER(_i)]),
    "dsm_ctx_trace_rb_pairs": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, C.POINTER(C.c_longlong)]),
    "dsm_rbpair_debug_path": (_i, [_i, _i, C.POINTER(_i)]),
    "dsm_rbpair_debug_set_chunk": (_i, [_i]),
    "dsm_nmft_set": (_i, [_vp, _f64p, _f64p, _i]),
    "dsm_nmft_get": (_i, [_vp, _vp, _vp]),
    "dsm_nmft_factorize": (_i, [_vp, _i, _d, _i, C.POINTER(_i), _vp]),
    "dsm_nmft_objective": (_i, [_vp, C.POINTER(_d)]),
    "dsm_nmft_debug_path": (_i, [_vp, _i, C.POINTER(_i)]),
    "dsm_nmft_get_tau": (_i, [_vp, _i64p]),
    "dsm_lrt_step": (_i, [_i, _f64p, _i32p, _i32p, _f64p, _d, _i, _i, _f64p, _f64p, _f64p]),
    "dsm_assign_tau": (_i, [_i, _i64p, _i, _i, _i, _f64p, _f64p, C.c_uint64, _vp, _vp, _vp, _vp, _vp]),
    "dsm_ctx_assign_tau": (_i, [_vp, _f64p, _f64p, _i, C.c_uint64, _vp, _vp, _vp, _vp, _vp]),
    "dsm_assign_debug_set_chunk": (_i, [_i]),
    "dsm_ctx_trace_predictive": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "dsm_pred_debug_set_chunk": (_i, [_i]),
    "dsm_pred_debug_set_parts": (_i, [_i]),
    "dsm_assign_tau_sampled": (_i, [_i, _i64p, _i, _i, _i, _f64p, _f64p, C.c_uint64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsm_ctx_assign_tau_sampled": (_i, [_vp, _f64p, _f64p, _i, C.c_uint64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsm_assign_tau_sampled_pairs": (_i, [_i, _i64p, _i, _i, _i, _f64p, _f64p, C.c_uint64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsm_ctx_assign_tau_sampled_pairs": (_i, [_vp, _f64p, _f64p, _i, C.c_uint64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsm_assign_sampled_debug_set_chunk": (_i, [_i]),
    "dsm_assign_sampled_debug_path": (_i, [_i, _i, C.POINTER(_i)]),
    "dsm_fit_gamma": (_i, [_i, _i64p, _i, _i, _i, _i64p, _f64p, _i, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsm_ctx_fit_gamma": (_i, [_vp, _i, _vp, _f64p, _i, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsm_abund_debug_set_chunk": (_i, [_i]),
    "dsm_fit_gamma_interval": (_i, [_i, _i64p, _i, _i, _i, _i64p, _f64p, _f64p, _d, _i, _d, _d, _vp, _vp, _vp]),
    "dsm_ctx_fit_gamma_interval": (_i, [_vp, _i, _vp, _f64p, _f64p, _d, _i, _d, _d, _vp, _vp, _vp]),
    "dsm_fit_gamma_eta": (_i, [_i, _i64p, _i, _i, _i, _i64p, _f64p, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsm_ctx_fit_gamma_eta": (_i, [_vp, _i, _vp, _f64p, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsm_abund_debug_set_eta_batch": (_i, [_i]),
    "dsm_abund_debug_set_eta_stage_max": (_i, [C.c_longlong]),
    "dsm_genes_create": (_i, [C.POINTER(_vp), _i]),
    "dsm_genes_destroy": (_i, [_vp]),
    "dsm_genes_set_data": (_i, [_vp, _vp, _i, _i, _i, _i32p, _f64p]),
    "dsm_genes_set_model": (_i, [_vp, _f64p, _f64p, _f64p, _i, _i, _f64p, _f64p, _f64p]),
    "dsm_genes_set_state": (_i, [_vp, _vp, _vp]),
    "dsm_genes_get_state": (_i, [_vp, _vp, _vp]),
    "dsm_genes_seed": (_i, [_vp, C.c_ulong, C.c_uint64]),
    "dsm_genes_set_gene_base": (_i, [_vp, _i]),
    "dsm_genes_get_mt_state": (_i, [_vp, _u32p]),
    "dsm_genes_set_mt_state": (_i, [_vp, _u32p]),
    "dsm_genes_nmft_tau": (_i, [_vp, _vp, _f64p, _i, _d, _vp]),
    "dsm_genes_sweep_all": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "dsm_genes_step_candidates": (_i, [_vp, _i, _i, _f64p, _vp]),
    "dsm_genes_step_choose": (_i, [_vp, _i, _i, _i]),
    "dsm_genes_update": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "dsm_genes_loglik": (_i, [_vp, _vp]),
    "dsm_genes_get_star": (_i, [_vp, _vp, _vp]),
    "dsm_genes_set_star": (_i, [_vp, _vp, _vp]),
    "dsm_genes_debug_tile": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_size_t)]),
    "dsm_kl_assign": (_i, [_i, _f64p, _f64p, _f64p, _i, _i, _i, _i, _d, C.POINTER(_i), C.POINTER(_d)]),
    "dsm_ctx_set_timing": (_i, [_vp, _i]),
    "dsm_ctx_get_timing": (_i, [_vp, _vp, _vp]),
    "dsm_kernel_name": (C.c_char_p, [_i]),
}

EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t)
_lib = None


def _digest(a):
    """128-bit digest of an array's bytes (xxh3 when the module is there: ~10 GB/s; blake2b otherwise)."""
    try:
        import xxhash
        return xxhash.xxh3_128_digest(memoryview(a).cast("B"))
    except ImportError:
        import hashlib
        return hashlib.blake2b(memoryview(a).cast("B"), digest_size=16).digest()


def load():
    """Load libdesman_hip.so (once).  Raises DesmanHipError if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DesmanHipError(
                "libdesman_hip.so not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C desman_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:
            raise DesmanHipError("cannot load %s: %s" % (LIB_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError = ABI drift: fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc):
    if rc != DSM_OK:
        raise DesmanHipError("libdesman_hip: error %d: %s" % (rc, load().dsm_last_error().decode()))
    return rc


def mt_seed_state(seed):
    """the 625-word MT19937 state gsl_rng_set(mt19937, seed) produces (position = 624)."""
    st = np.empty(625, dtype=np.uint32)
    check(load().dsm_mt_seed_state(int(seed) & 0xFFFFFFFFFFFFFFFF, st))
    return st


def release_device_caches():
    """frees the per-process, per-device caches of the library (MT19937 jump tables, placed subset tables); no context may be busy"""
    check(load().dsm_release_device_caches())


def debug_fdiv(kind, a, b):
    """test hook: a / b as the NMFT update divides (0 = fdiv_ext, 1 = fdiv_lo, 2 = fdiv; kernels_nmft.hip)"""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    out = np.empty_like(a)
    check(load().dsm_debug_fdiv(int(kind), a, b, out, a.size))
    return out


def lrt_step(ffreq, maxA, maxB, eta, upperP, optimise, p, device=0):
    """one inner step of the likelihood-ratio variant filter on the GPU -> (p, MLL, BLL)."""
    ffreq = np.ascontiguousarray(ffreq, dtype=np.float64)
    V = ffreq.shape[0]
    p = np.ascontiguousarray(p, dtype=np.float64).copy()
    MLL = np.empty(V); BLL = np.empty(V)
    check(load().dsm_lrt_step(int(device), ffreq, np.ascontiguousarray(maxA, dtype=np.int32),
                              np.ascontiguousarray(maxB, dtype=np.int32), np.ascontiguousarray(eta, dtype=np.float64),
                              float(upperP), int(bool(optimise)), V, p, MLL, BLL))
    return p, MLL, BLL


def device_count():
    return load().dsm_device_count()


ASSIGN_MAX_G = 10    # DSM_ASSIGN_MAX_G: dsm_assign_tau evaluates all 4^G joint states of a position


def _assign_model(gamma, eta, S):
    gamma = np.ascontiguousarray(gamma, dtype=np.float64)
    eta = np.ascontiguousarray(eta, dtype=np.float64)
    if gamma.ndim != 2 or gamma.shape[0] != S or eta.shape != (4, 4):
        raise ValueError("assign_tau: gamma must be [S=%d, G] and eta [4, 4]; got %s, %s" % (S, gamma.shape, eta.shape))
    return gamma, eta


def _assign_out(N, G, seed):
    out = dict(map_state=np.zeros((N, G), dtype=np.uint8), conf=np.zeros(N), logz=np.zeros(N), marg=np.zeros((N, G, 4)))
    if seed is not None:
        out["draw_state"] = np.zeros((N, G), dtype=np.uint8)
    return out


def assign_tau(counts, gamma, eta, seed=None, device=0):
    """Exact joint assignment of the positions ``counts`` [N,S,4] under fitted gamma [S,G], eta [4,4] (dsm_assign_tau): a dict of
    map_state [N,G] uint8, conf [N], logz [N], marg [N,G,4] and -- with a seed -- draw_state [N,G], one posterior draw per
    position keyed by (seed, position).  G <= ASSIGN_MAX_G."""
    x = np.ascontiguousarray(counts, dtype=np.int64)
    if x.ndim != 3 or x.shape[2] != 4:
        raise ValueError("assign_tau: counts must be [N,S,4]")
    N, S = x.shape[0], x.shape[1]
    gamma, eta = _assign_model(gamma, eta, S)
    G = gamma.shape[1]
    out = _assign_out(N, G, seed)
    check(load().dsm_assign_tau(int(device), x, N, S, G, gamma, eta, int(seed or 0) & 0xFFFFFFFFFFFFFFFF, _ptr(out["map_state"]),
                                _ptr(out["conf"]), _ptr(out["logz"]), _ptr(out["marg"]), _ptr(out.get("draw_state"))))
    return out


def assign_debug_set_chunk(positions=0):
    """test hook: positions per launch of assign_tau / Context.assign_tau (0 = the default bound); results do not depend on it"""
    check(load().dsm_assign_debug_set_chunk(int(positions)))


def pred_debug_set_chunk(positions=0):
    """test hook: positions per chunk of Context.trace_predictive (0 = the library's own choice); results do not depend on it"""
    check(load().dsm_pred_debug_set_chunk(int(positions)))


def pred_debug_set_parts(parts=0):
    """test hook: the parts a launch of Context.trace_predictive cuts its iterations into across workgroups (0 = the library's own
    choice); results do not depend on it"""
    check(load().dsm_pred_debug_set_parts(int(parts)))


SAMPLED_KEPT, SAMPLED_BURN = 100, 20    # conventions of `desman-assign --sampled`, not tuned
SAMPLED_PAIRS = 5                       # a bare `--pairs`: a pair pass after every fifth sweep -- a convention too, not tuned
SAMPLED_OPTIONAL = ("map_ll", "conf", "spread", "draw_state")


def _assign_sampled_out(N, G, want):
    """the output arrays of the sampled call; ``want`` names the optional ones (None: all of them)"""
    want = SAMPLED_OPTIONAL if want is None else tuple(want)
    bad = [k for k in want if k not in SAMPLED_OPTIONAL]
    if bad:
        raise ValueError("assign_tau_sampled: unknown optional output %r" % bad[0])
    out = dict(map_state=np.zeros((N, G), dtype=np.uint8), marg=np.zeros((N, G, 4)))
    for k in want:
        out[k] = np.zeros((N, G), dtype=np.uint8) if k == "draw_state" else np.zeros(N)
    return out


def _sweeps(burn, kept, pair_every=0):
    burn, kept, pair_every = int(burn), int(kept), int(pair_every)
    if not all(-2 ** 31 <= v < 2 ** 31 for v in (burn, kept, pair_every)):
        raise ValueError("assign_tau_sampled: burn / kept / pair_every outside the int range")
    return burn, kept, pair_every


def assign_tau_sampled(counts, gamma, eta, seed=0, burn=SAMPLED_BURN, kept=SAMPLED_KEPT, want=None, device=0, pair_every=0):
    """Sampled joint assignment of the positions ``counts`` [N,S,4] under fitted gamma [S,G], eta [4,4] (dsm_assign_tau_sampled;
    G <= 32): four private Gibbs chains per position, ``burn`` + ``kept`` sweeps each.  A dict of map_state [N,G] uint8, marg
    [N,G,4] and the optional outputs named by ``want`` (default all): map_ll [N], conf [N], spread [N], draw_state [N,G].
    ``pair_every`` = E > 0: every E-th sweep is followed by a pass of joint moves of two haplotypes, and the polish climbs over pairs
    as well (dsm_assign_tau_sampled_pairs); 0: single-site moves only."""
    x = np.ascontiguousarray(counts, dtype=np.int64)
    if x.ndim != 3 or x.shape[2] != 4:
        raise ValueError("assign_tau_sampled: counts must be [N,S,4]")
    N, S = x.shape[0], x.shape[1]
    gamma, eta = _assign_model(gamma, eta, S)
    G = gamma.shape[1]
    burn, kept, pair_every = _sweeps(burn, kept, pair_every)
    out = _assign_sampled_out(N, G, want)
    check(load().dsm_assign_tau_sampled_pairs(int(device), x, N, S, G, gamma, eta, int(seed) & 0xFFFFFFFFFFFFFFFF, burn, kept, pair_every,
                                              _ptr(out["map_state"]), _ptr(out.get("map_ll")), _ptr(out.get("conf")), _ptr(out["marg"]),
                                              _ptr(out.get("spread")), _ptr(out.get("draw_state"))))
    return out


def assign_sampled_debug_set_chunk(positions=0):
    """test hook: positions per launch of assign_tau_sampled / Context.assign_tau_sampled (0 = the default bound)"""
    check(load().dsm_assign_sampled_debug_set_chunk(int(positions)))


def assign_sampled_debug_path(S, G):
    """test hook: the path a shape takes -- dict of inst, lpv, nsl, gamma_chunk, positions_per_workgroup; nothing is launched"""
    out = (C.c_int * 5)()
    check(load().dsm_assign_sampled_debug_path(int(S), int(G), out))
    return dict(zip(("inst", "lpv", "nsl", "gamma_chunk", "positions_per_workgroup"), [int(v) for v in out]))


def pairtau_debug_path(S, G):
    """test hook: (lanes per position, sample slots per lane) of the pair-pass kernel for S samples; nothing is launched"""
    out = (C.c_int * 2)()
    check(load().dsm_pairtau_debug_path(int(S), int(G), out))
    return int(out[0]), int(out[1])


def rbtau_debug_path(S, G):
    """test hook: (lanes per position, sample slots per lane) of the kernel of Context.trace_rb_marginals for S samples; nothing is
    launched"""
    out = (C.c_int * 2)()
    check(load().dsm_rbtau_debug_path(int(S), int(G), out))
    return int(out[0]), int(out[1])


def rbpair_debug_path(S, G):
    """test hook: (lanes per position, sample slots per lane) of the kernel of Context.trace_rb_pairs for S samples; nothing is
    launched"""
    out = (C.c_int * 2)()
    check(load().dsm_rbpair_debug_path(int(S), int(G), out))
    return int(out[0]), int(out[1])


def rbpair_debug_set_chunk(positions=0):
    """test hook: positions per launch of Context.trace_rb_pairs (0 = by the scratch bound); results do not depend on it"""
    check(load().dsm_rbpair_debug_set_chunk(int(positions)))


def diag_debug_set_parts(parts=0):
    """test hook: the parts Context.trace_batch_stats splits its batches into across workgroups (0 = the library's own choice);
    results do not depend on it"""
    check(load().dsm_diag_debug_set_parts(int(parts)))


def fit_debug_set_parts(parts=0):
    """test hook: the parts Context.trace_fit_stats splits its iterations into across workgroups (0 = the library's own choice); the
    results agree to rounding between part counts and are the same bits for one part count"""
    check(load().dsm_fit_debug_set_parts(int(parts)))


def ppc_debug_set_parts(parts=0):
    """test hook: the parts a launch of Context.trace_ppc splits its iterations into across workgroups (0 = the library's own choice);
    no result depends on it"""
    check(load().dsm_ppc_debug_set_parts(int(parts)))


def ppc_debug_set_chunk(iterations=0, replicates=0):
    """test hook: the iterations and replicates per launch of Context.trace_ppc (0 = by the library's scratch bound); no result depends
    on them"""
    check(load().dsm_ppc_debug_set_chunk(int(iterations), int(replicates)))


FIT_MAX_ITER, FIT_TOL = 20000, 1.0e-9    # defaults of fit_gamma: plain EM is slow near the boundary


def _fit_tau(tau, V):
    """tau as [V,G] int64 digits, from digits or from the one-hot form [V,G,4]"""
    t = np.asarray(tau)
    if t.ndim == 3 and t.shape[2] == 4:
        t = np.argmax(t, axis=2)
    t = np.ascontiguousarray(t, dtype=np.int64)
    if t.ndim != 2 or t.shape[0] != V:
        raise ValueError("fit_gamma: tau must be [V=%d, G] digits or [V, G, 4] one-hot; got %s" % (V, np.shape(tau)))
    return t


def _fit_eta(eta):
    eta = np.ascontiguousarray(eta, dtype=np.float64)
    if eta.shape != (4, 4):
        raise ValueError("fit_gamma: eta must be [4, 4]; got %s" % (eta.shape,))
    return eta


def _fit_out(S, G, presence):
    out = dict(gamma=np.zeros((S, G)), loglik=np.zeros(S), deviance=np.zeros(S), iters=np.zeros(S, dtype=np.int32),
               converged=np.zeros(S, dtype=np.int32))
    if presence:
        out["lr_absent"] = np.zeros((S, G))
    return out


def fit_gamma(counts, tau, eta, max_iter=FIT_MAX_ITER, tol=FIT_TOL, presence=False, device=0):
    """Maximum-likelihood abundances of the haplotypes ``tau`` ([V,G] digits or [V,G,4] one-hot) in the samples of ``counts`` [V,S,4]
    with tau and eta [4,4] held fixed (dsm_fit_gamma): a dict of gamma [S,G], loglik [S], deviance [S], iters [S], converged [S] and --
    with ``presence`` -- lr_absent [S,G], the likelihood-ratio statistic of "haplotype g is absent from sample s"."""
    x = np.ascontiguousarray(counts, dtype=np.int64)
    if x.ndim != 3 or x.shape[2] != 4:
        raise ValueError("fit_gamma: counts must be [V,S,4]")
    V, S = x.shape[0], x.shape[1]
    t, eta = _fit_tau(tau, V), _fit_eta(eta)
    G = t.shape[1]
    out = _fit_out(S, G, presence)
    check(load().dsm_fit_gamma(int(device), x, V, S, G, t, eta, int(max_iter), float(tol), int(bool(presence)), _ptr(out["gamma"]),
                               _ptr(out["loglik"]), _ptr(out["deviance"]), _ptr(out["iters"]), _ptr(out["converged"]),
                               _ptr(out.get("lr_absent"))))
    return out


def abund_debug_set_chunk(samples=0):
    """test hook: samples per launch of fit_gamma / fit_gamma_interval and their Context forms (0 = the default bound); results do
    not depend on it"""
    check(load().dsm_abund_debug_set_chunk(int(samples)))


FIT_CTOL = 1.0e-6                         # default bracket width at which an interval search stops


def chi2_quantile(level):
    """the chi-square (1 d.o.f.) quantile of a confidence level in (0, 1): the square of the normal quantile at (1 + level) / 2"""
    from statistics import NormalDist
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError("interval level must lie in (0, 1); got %r" % level)
    return NormalDist().inv_cdf(0.5 * (1.0 + level)) ** 2


def _interval_args(gamma_hat, S, G, level, q):
    g = np.ascontiguousarray(gamma_hat, dtype=np.float64)
    if g.shape != (S, G):
        raise ValueError("fit_gamma_interval: gamma_hat must be [S=%d, G=%d]; got %s" % (S, G, g.shape))
    out = dict(lo=np.zeros((S, G)), hi=np.zeros((S, G)), flags=np.zeros((S, G), dtype=np.int32))
    return g, float(chi2_quantile(level) if q is None else q), out


def fit_gamma_interval(counts, tau, eta, gamma_hat, level=0.95, q=None, max_iter=FIT_MAX_ITER, tol=FIT_TOL, ctol=FIT_CTOL, device=0):
    """Profile-likelihood intervals of the abundances ``gamma_hat`` [S,G] that fit_gamma returned for the same counts, tau and eta
    (dsm_fit_gamma_interval): a dict of lo [S,G], hi [S,G] and flags [S,G] (bit 1: lo is the boundary 0, 2: hi is the boundary 1, 4: an
    inner fit ended at max_iter, the interval is too narrow).  ``level`` is the confidence level; ``q`` overrides its chi-square quantile."""
    x = np.ascontiguousarray(counts, dtype=np.int64)
    if x.ndim != 3 or x.shape[2] != 4:
        raise ValueError("fit_gamma_interval: counts must be [V,S,4]")
    V, S = x.shape[0], x.shape[1]
    t, eta = _fit_tau(tau, V), _fit_eta(eta)
    G = t.shape[1]
    g, q, out = _interval_args(gamma_hat, S, G, level, q)
    check(load().dsm_fit_gamma_interval(int(device), x, V, S, G, t, eta, g, q, int(max_iter), float(tol), float(ctol), _ptr(out["lo"]),
                                        _ptr(out["hi"]), _ptr(out["flags"])))
    return out


def _fit_eta_out(S, G):
    out = dict(gamma=np.zeros((S, G)), eta=np.zeros((4, 4)), loglik=np.zeros(S), loglik0=np.zeros(S), deviance=np.zeros(S))
    scal = dict(iters=np.zeros(1, dtype=np.int32), converged=np.zeros(1, dtype=np.int32), dead_rows=np.zeros(1, dtype=np.int32),
                lr_eta=np.zeros(1))
    ptrs = [_ptr(out[k]) for k in ("gamma", "eta", "loglik", "loglik0", "deviance")] \
        + [_ptr(scal[k]) for k in ("iters", "converged", "dead_rows", "lr_eta")]
    return out, scal, ptrs


def _fit_eta_result(out, scal):
    out.update(iters=int(scal["iters"][0]), converged=int(scal["converged"][0]), dead_rows=int(scal["dead_rows"][0]),
               lr_eta=float(scal["lr_eta"][0]))
    return out


def fit_gamma_eta(counts, tau, eta0, max_iter=FIT_MAX_ITER, tol=FIT_TOL, device=0):
    """Abundances of the haplotypes ``tau`` in the samples of ``counts`` [V,S,4] AND one error matrix shared by these samples, fitted
    jointly by EM from the uniform rows and ``eta0`` with tau held fixed (dsm_fit_gamma_eta): a dict of gamma [S,G], eta [4,4], loglik
    [S], deviance [S], loglik0 [S] (the fit with eta held at eta0: fit_gamma's loglik) and the call's iters, converged, dead_rows (bit a:
    row a of eta had no mass in some step and kept its values) and lr_eta = 2 (sum loglik - sum loglik0) >= 0."""
    x = np.ascontiguousarray(counts, dtype=np.int64)
    if x.ndim != 3 or x.shape[2] != 4:
        raise ValueError("fit_gamma_eta: counts must be [V,S,4]")
    V, S = x.shape[0], x.shape[1]
    t, eta0 = _fit_tau(tau, V), _fit_eta(eta0)
    G = t.shape[1]
    out, scal, ptrs = _fit_eta_out(S, G)
    check(load().dsm_fit_gamma_eta(int(device), x, V, S, G, t, eta0, int(max_iter), float(tol), *ptrs))
    return _fit_eta_result(out, scal)


def abund_debug_set_eta_batch(steps=0):
    """test hook: EM steps of fit_gamma_eta enqueued between two reads of the device's stop word (0 = the default); results do not
    depend on it"""
    check(load().dsm_abund_debug_set_eta_batch(int(steps)))


def abund_debug_set_eta_stage_max(nbytes=0):
    """test hook: the bound of fit_gamma_eta's sample-major copy of the counts in bytes (0 = the default, 1 GiB)"""
    check(load().dsm_abund_debug_set_eta_stage_max(int(nbytes)))


def _ptr(a):
    return None if a is None else a.ctypes.data


class Context:
    """A device-resident chain context (dsm_ctx)."""

    def __init__(self, device=0):
        self._h = _vp()
        self.lib = load()
        check(self.lib.dsm_ctx_create(C.byref(self._h), int(device)))
        self.V = self.S = self.G = 0
        self.nG = 0
        self.n_trace = 0

    def close(self):
        if self._h:
            self.lib.dsm_ctx_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.lib.dsm_ctx_sync(self._h))

    # ---- data / state
    def set_counts(self, variants):
        v = np.ascontiguousarray(variants, dtype=np.int64)
        if v.ndim != 3 or v.shape[2] != 4:
            raise ValueError("variants must be [V,S,4]")
        # re-uploading is skipped when the very same tensor is already resident (Init_NMFT and HaploSNP_Sampler of
        # one run share a context): same shape and same 128-bit digest of the bytes
        token = (v.shape, _digest(v))
        if getattr(self, "_counts_token", None) == token:
            return
        self._counts_token = None                        # a failed upload leaves no tensor resident
        check(self.lib.dsm_ctx_set_counts(self._h, v, v.shape[0], v.shape[1]))
        self.V, self.S = v.shape[0], v.shape[1]
        self.G = 0
        self._counts_token = token

    def set_state(self, tau, gamma, eta):
        tau = np.ascontiguousarray(tau, dtype=np.int64)
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        eta = np.ascontiguousarray(eta, dtype=np.float64)
        if tau.shape != (self.V, gamma.shape[1], 4) or gamma.shape[0] != self.S or eta.shape != (4, 4):
            raise ValueError("state shapes do not match the count tensor")
        check(self.lib.dsm_ctx_set_state(self._h, tau, gamma, eta, gamma.shape[1]))
        self.G = gamma.shape[1]

    def get_state(self):
        tau = np.empty((self.V, self.G, 4), dtype=np.int64)
        gamma = np.empty((self.S, self.G))
        eta = np.empty((4, 4))
        check(self.lib.dsm_ctx_get_state(self._h, _ptr(tau), _ptr(gamma), _ptr(eta)))
        return tau, gamma, eta

    def set_gamma_eta(self, gamma=None, eta=None):
        g = None if gamma is None else np.ascontiguousarray(gamma, dtype=np.float64)
        e = None if eta is None else np.ascontiguousarray(eta, dtype=np.float64)
        check(self.lib.dsm_ctx_set_gamma_eta(self._h, _ptr(g), _ptr(e)))

    def set_priors(self, alpha=0.1, delta=0.1, epsilon=1e-6):
        check(self.lib.dsm_ctx_set_priors(self._h, alpha, delta, epsilon))

    def seed(self, mt_seed, ctr_seed=None):
        if ctr_seed is None:
            ctr_seed = (int(mt_seed) * 0x9E3779B97F4A7C15 + 0x243F6A8885A308D3) & 0xFFFFFFFFFFFFFFFF
        check(self.lib.dsm_ctx_seed(self._h, int(mt_seed) & 0xFFFFFFFFFFFFFFFF, int(ctr_seed)))

    def get_mt_state(self):
        st = np.empty(625, dtype=np.uint32)
        check(self.lib.dsm_ctx_get_mt_state(self._h, st))
        return st

    # ---- checkpoint / resume (the reference's own hook is dead code)
    def checkpoint(self):
        """everything that places the chain: state, MT19937 stream, counter-stream key and iteration counter (a dict of arrays:
        np.savez(path, **ctx.checkpoint()) writes it).  Counts, priors and the tau RNG mode are the caller's to keep."""
        tau, gamma, eta = self.get_state()
        key, it = self.counters()
        try:
            mt = self.get_mt_state()
        except DesmanHipError:                                   # never seeded: counter-based runs
            mt = np.zeros(0, dtype=np.uint32)
        return dict(tau=tau, gamma=gamma, eta=eta, mt_state=mt, ctr_seed=np.uint64(key), iter_ctr=np.uint32(it), screen=self.screen_state())

    def counters(self):
        """(key of the counter-based streams, iterations drawn so far) -- needs no resident state"""
        key, it = C.c_uint64(0), C.c_uint32(0)
        check(self.lib.dsm_ctx_get_counters(self._h, C.byref(key), C.byref(it)))
        return int(key.value), int(it.value)

    def screen_state(self):
        """the tau sweep's screening state: sweeps still to run without the fp32 screening pass, per launch parity"""
        out = np.zeros(2, dtype=np.uint32)
        check(self.lib.dsm_ctx_get_screen_state(self._h, out))
        return out

    def set_screen_state(self, words):
        check(self.lib.dsm_ctx_set_screen_state(self._h, np.ascontiguousarray(words, dtype=np.uint32)))

    def restore(self, ck):
        """put a chain saved by checkpoint() into this context (counts set already): it continues bit for bit"""
        self.set_state(np.ascontiguousarray(ck["tau"], dtype=np.int64), np.ascontiguousarray(ck["gamma"], dtype=np.float64),
                       np.ascontiguousarray(ck["eta"], dtype=np.float64))
        mt = np.asarray(ck["mt_state"], dtype=np.uint32)
        if mt.size == 625:
            self.set_mt_state(np.ascontiguousarray(mt))
        check(self.lib.dsm_ctx_set_counters(self._h, int(ck["ctr_seed"]), int(ck["iter_ctr"])))
        # the screening decisions of the saved chain (older checkpoints have none: the screen starts switched on, as in a fresh chain)
        self.set_screen_state(ck["screen"] if "screen" in ck else np.zeros(2, dtype=np.uint32))

    def set_mt_state(self, st):
        check(self.lib.dsm_ctx_set_mt_state(self._h, np.ascontiguousarray(st, dtype=np.uint32)))

    def debug_mt_fill(self, n):
        out = np.empty(int(n), dtype=np.uint32)
        check(self.lib.dsm_ctx_debug_mt_fill(self._h, int(n), out))
        return out

    def set_tau_rng(self, mode):
        check(self.lib.dsm_ctx_set_tau_rng(self._h, int(mode)))

    def assign_tau(self, gamma, eta, seed=None):
        """assign_tau() of the module on the count tensor resident in this context (no second upload); the chain state is not touched"""
        gamma, eta = _assign_model(gamma, eta, self.S)
        G = gamma.shape[1]
        out = _assign_out(self.V, G, seed)
        check(self.lib.dsm_ctx_assign_tau(self._h, gamma, eta, G, int(seed or 0) & 0xFFFFFFFFFFFFFFFF, _ptr(out["map_state"]),
                                          _ptr(out["conf"]), _ptr(out["logz"]), _ptr(out["marg"]), _ptr(out.get("draw_state"))))
        return out

    def assign_tau_sampled(self, gamma, eta, seed=0, burn=SAMPLED_BURN, kept=SAMPLED_KEPT, want=None, pair_every=0):
        """assign_tau_sampled() of the module on the count tensor resident in this context; the chain state is not touched"""
        gamma, eta = _assign_model(gamma, eta, self.S)
        G = gamma.shape[1]
        burn, kept, pair_every = _sweeps(burn, kept, pair_every)
        out = _assign_sampled_out(self.V, G, want)
        check(self.lib.dsm_ctx_assign_tau_sampled_pairs(self._h, gamma, eta, G, int(seed) & 0xFFFFFFFFFFFFFFFF, burn, kept, pair_every,
                                                        _ptr(out["map_state"]), _ptr(out.get("map_ll")), _ptr(out.get("conf")),
                                                        _ptr(out["marg"]), _ptr(out.get("spread")), _ptr(out.get("draw_state"))))
        return out

    def fit_gamma(self, eta, tau=None, max_iter=FIT_MAX_ITER, tol=FIT_TOL, presence=False):
        """fit_gamma() of the module for the samples of the count tensor resident in this context (no second upload), with the given
        tau or -- tau=None -- the context's resident tau; the chain state is not touched"""
        eta = _fit_eta(eta)
        t = None if tau is None else _fit_tau(tau, self.V)
        G = self.G if t is None else t.shape[1]
        out = _fit_out(self.S, G, presence)
        check(self.lib.dsm_ctx_fit_gamma(self._h, G, _ptr(t), eta, int(max_iter), float(tol), int(bool(presence)), _ptr(out["gamma"]),
                                         _ptr(out["loglik"]), _ptr(out["deviance"]), _ptr(out["iters"]), _ptr(out["converged"]),
                                         _ptr(out.get("lr_absent"))))
        return out

    def fit_gamma_eta(self, eta0, tau=None, max_iter=FIT_MAX_ITER, tol=FIT_TOL):
        """fit_gamma_eta() of the module for the samples of the resident count tensor, with the given tau or the resident one"""
        eta0 = _fit_eta(eta0)
        t = None if tau is None else _fit_tau(tau, self.V)
        G = self.G if t is None else t.shape[1]
        out, scal, ptrs = _fit_eta_out(self.S, G)
        check(self.lib.dsm_ctx_fit_gamma_eta(self._h, G, _ptr(t), eta0, int(max_iter), float(tol), *ptrs))
        return _fit_eta_result(out, scal)

    def fit_gamma_interval(self, eta, gamma_hat, tau=None, level=0.95, q=None, max_iter=FIT_MAX_ITER, tol=FIT_TOL, ctol=FIT_CTOL):
        """fit_gamma_interval() of the module for the samples of the resident count tensor, with the given tau or the resident one"""
        eta = _fit_eta(eta)
        t = None if tau is None else _fit_tau(tau, self.V)
        G = self.G if t is None else t.shape[1]
        g, q, out = _interval_args(gamma_hat, self.S, G, level, q)
        check(self.lib.dsm_ctx_fit_gamma_interval(self._h, G, _ptr(t), eta, g, q, int(max_iter), float(tol), float(ctol), _ptr(out["lo"]),
                                                  _ptr(out["hi"]), _ptr(out["flags"])))
        return out

    # ---- single steps
    def sample_tau(self, want_logp=False):
        n = _i(0)
        logp = np.empty((self.V, self.G, 4)) if want_logp else None
        check(self.lib.dsm_ctx_sample_tau(self._h, C.byref(n), _ptr(logp)))
        return (n.value, logp) if want_logp else n.value

    def sample_stats(self, it):
        mu = np.zeros((self.S, self.G), dtype=np.uint64)
        E = np.zeros((4, 4), dtype=np.uint64)
        check(self.lib.dsm_ctx_sample_stats(self._h, int(it), mu, E))
        return mu, E

    def debug_log2f(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        check(self.lib.dsm_ctx_debug_log2f(self._h, x.ctypes.data, out.ctypes.data, x.size))
        return out

    def set_tau_neartie(self, mode=-1):
        """which instantiation of the Gibbs loop's tau sweep runs: -1 = the one with the near-tie screen when the chain holds a haplotype
        that is rare in every sample (decided at the start of each gibbs_update call), 0 = never, 1 = always; same draws either way"""
        check(self.lib.dsm_ctx_set_tau_neartie(self._h, int(mode)))

    def set_big_launch(self, mode=-1):
        """the launch of stats_big_kernel after stage 1 of the aggregated mu/E pass, where it is a choice (full chain, G < 10, spec 2 / 3):
        -1 = while stage 1 was last seen handing items over, 0 = never (the Dirichlet launch draws them), 1 = always; same draws either way"""
        check(self.lib.dsm_ctx_set_big_launch(self._h, int(mode)))

    def debug_big_lists(self):
        """(non-zero words among the deferred lists' counters -- 0 between passes --, the device's running count of lists found non-empty)"""
        a, b = _i(0), C.c_uint32(0)
        check(self.lib.dsm_ctx_debug_big_lists(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_tau_screen(self, on):
        """A/B switch: False = every step of the tau sweep in fp64 (same draws except in ~1e-13 near-ties)"""
        check(self.lib.dsm_ctx_set_tau_screen(self._h, 1 if on else 0))

    def tau_launch_info(self):
        """(workgroups a tau sweep launches, workgroups of that kernel resident on the device at once)"""
        a, b = _i(0), _i(0)
        check(self.lib.dsm_ctx_tau_launch_info(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_nmft_persist(self, mode=-1):
        """nmft_factorize as one persistent launch where the table fits: -1 / 1 = yes (default), 0 = the three-launch loop"""
        check(self.lib.dsm_ctx_set_nmft_persist(self._h, int(mode)))

    def set_nmft_fused(self, mode=-1):
        """gamma/control step of an NMFT update: -1 = by size, 0 = a launch of its own, 1 = one launch with the reduction, 3 = at the start of the update kernel (same results)"""
        check(self.lib.dsm_ctx_set_nmft_fused(self._h, int(mode)))

    def sweep_stats(self, reset=False):
        """(wavefront-steps of the tau sweeps so far, of which evaluated in fp64 because the screening pass
        could not decide them); reset=True also zeroes the totals"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.dsm_ctx_sweep_stats(self._h, C.byref(a), C.byref(b), 1 if reset else 0))
        return a.value, b.value

    def stats_spec(self):
        """2 / 3 = aggregated mu/E sampler (oracle/stats_agg.c: 2 = the default version, 3 = the table exp/log variant), 1 = per-read draws (orc_stats_counter)."""
        r = self.lib.dsm_ctx_stats_spec(self._h)
        if r < 0:
            check(r)
        return r

    def force_stats_spec(self, spec=0):
        """0 = shape rule, 1 = per-read draws everywhere, 2 (STATS_AGG) / 3 = that version of the aggregated sampler on small
        problems too (G <= 16), 4 = spec 2 over tau words (G <= 8; spec 2 where it does not apply)."""
        check(self.lib.dsm_ctx_force_stats_spec(self._h, int(spec)))

    def debug_stage1(self, it):
        nt = np.zeros((self.S, 1 << self.G), dtype=np.uint32)
        E = np.zeros((4, 4), dtype=np.uint64)
        check(self.lib.dsm_ctx_debug_stage1(self._h, int(it), nt.ctypes.data, E))
        return nt, E

    def debug_binom(self, kind, n, w, seed, nsamp, spec=STATS_AGG):
        w4 = np.zeros(4)
        w4[:len(w)] = w
        out = np.zeros((nsamp, 4) if kind == 2 else nsamp, dtype=np.uint32)
        check(self.lib.dsm_ctx_debug_binom(self._h, int(kind), int(n), w4, int(seed), int(nsamp), out.reshape(-1), int(spec)))
        return out

    def draw_gamma_eta(self, it, sum_mu, esum):
        g = np.empty((self.S, self.G)); e = np.empty((4, 4))
        check(self.lib.dsm_ctx_draw_gamma_eta(self._h, int(it), np.ascontiguousarray(sum_mu, dtype=np.uint64),
                                              np.ascontiguousarray(esum, dtype=np.uint64), g, e))
        return g, e

    def loglik(self):
        ll, lp = _d(0), _d(0)
        check(self.lib.dsm_ctx_loglik(self._h, C.byref(ll), C.byref(lp)))
        return ll.value, lp.value

    # ---- update loops
    def gibbs_update(self, n_iter):
        check(self.lib.dsm_ctx_gibbs_update(self._h, int(n_iter)))
        self.n_trace = int(n_iter)

    def gibbs_update_fixed_tau(self, n_iter, fix_eta=False, pool=-1):
        """n_iter iterations of the chain with tau held (include/desman_hip.h: dsm_ctx_gibbs_update_fixed_tau): results as after
        gibbs_update.  fix_eta: eta is held too.  pool: 0 = on the table as it is, 1 = on the counts pooled per distinct tau word,
        -1 = pooled where that makes the table smaller."""
        check(self.lib.dsm_ctx_gibbs_update_fixed_tau(self._h, int(n_iter), 1 if fix_eta else 0, int(pool)))
        self.n_trace = int(n_iter)

    def sample_tau_held(self, n_held):
        """one tau sweep over haplotypes 0 .. G - n_held - 1 of the resident state, the last n_held held (include/desman_hip.h:
        dsm_ctx_sample_tau_held); returns the number of changed (position, haplotype) pairs"""
        n = _i(0)
        check(self.lib.dsm_ctx_sample_tau_held(self._h, int(n_held), C.byref(n)))
        return n.value

    def set_pair_moves(self, every):
        """pair moves of gibbs_update (include/desman_hip.h: dsm_ctx_set_pair_moves): 0 = off, E > 0 = a pair pass after the sweep of
        every iteration whose counter satisfies (iter_ctr + 1) mod E == 0"""
        check(self.lib.dsm_ctx_set_pair_moves(self._h, int(every)))

    def get_pair_moves(self):
        e = _i(0)
        check(self.lib.dsm_ctx_get_pair_moves(self._h, C.byref(e)))
        return e.value

    def sample_tau_pairs(self, iteration):
        """one pair pass on the resident state with the resident gamma / eta, keyed by `iteration` (include/desman_hip.h:
        dsm_ctx_sample_tau_pairs); returns the number of changed haplotype digits"""
        n = _i(0)
        check(self.lib.dsm_ctx_sample_tau_pairs(self._h, int(iteration) & 0xFFFFFFFF, C.byref(n)))
        return n.value

    def gibbs_update_held_tau(self, n_iter, n_held, fix_eta=False):
        """n_iter Gibbs iterations with the last n_held haplotypes held (include/desman_hip.h: dsm_ctx_gibbs_update_held_tau): results
        as after gibbs_update.  fix_eta: eta is held too.  n_held = 0 is gibbs_update, n_held = G is gibbs_update_fixed_tau(pool=0)."""
        check(self.lib.dsm_ctx_gibbs_update_held_tau(self._h, int(n_iter), int(n_held), 1 if fix_eta else 0))
        self.n_trace = int(n_iter)

    def debug_fixtau_pool(self):
        """the pooled table of the resident state: dict of W, pooled [W,S,4] int32, words [W] uint64 ascending, row [V] int32"""
        w = _i(0)
        pooled = np.zeros((self.V, self.S, 4), dtype=np.int32)
        words = np.zeros(self.V, dtype=np.uint64)
        row = np.zeros(self.V, dtype=np.int32)
        check(self.lib.dsm_ctx_debug_fixtau_pool(self._h, C.byref(w), _ptr(pooled), _ptr(words), _ptr(row)))
        return dict(W=w.value, pooled=pooled[:w.value].copy(), words=words[:w.value].copy(), row=row)

    def debug_fixtau_sample_stats(self, it):
        """sample_stats(it) drawn on the pooled state of the resident one"""
        mu = np.zeros((self.S, self.G), dtype=np.uint64)
        E = np.zeros((4, 4), dtype=np.uint64)
        check(self.lib.dsm_ctx_debug_fixtau_sample_stats(self._h, int(it), mu, E))
        return mu, E

    def gibbs_update_sharded(self, n_iter, v_offset, v_total, exchange):
        """n_iter iterations of ONE chain sharded by positions (include/desman_hip.h: dsm_ctx_gibbs_update_sharded): this context
        holds positions v_offset .. v_offset + V of v_total.  ``exchange(tab_ptr, n_tab, vec_ptr, n_vec)`` is the caller's
        all-reduce (sum) of n_tab uint32 at device address tab_ptr (0 words: skip) and n_vec float64 at vec_ptr, in place; an
        exception raised inside it aborts the call and is re-raised here."""
        err = []

        def cb(user, tab, n_tab, vec, n_vec):
            try:
                exchange(tab or 0, int(n_tab), vec, int(n_vec))
                return 0
            except BaseException as e:                       # noqa: BLE001 -- must not propagate through the C frame
                err.append(e)
                return 1
        fn = EXCHANGE_FN(cb)
        rc = self.lib.dsm_ctx_gibbs_update_sharded(self._h, int(n_iter), int(v_offset), int(v_total), C.cast(fn, _vp), None)
        if err:
            raise err[0]
        check(rc)
        self.n_trace = int(n_iter)

    def gibbs_update_sharded_comm(self, n_iter, v_offset, v_total, comm):
        """the same with the exchange done by the library over its own RCCL communicator (desman_amd/comm.py: Comm): the two
        all-reduces of an iteration are enqueued on the chain's stream, no host synchronisation, no torch"""
        check(self.lib.dsm_ctx_gibbs_update_sharded_comm(self._h, int(n_iter), int(v_offset), int(v_total), comm._h))
        self.n_trace = int(n_iter)

    @staticmethod
    def batch_gibbs_update(ctxs, n_iter):
        """n_iter Gibbs iterations of every chain in ``ctxs`` (contexts of one shape on one device, at most 8), one launch
        per kernel of the iteration for all of them (include/desman_hip.h: dsm_batch_gibbs_update)."""
        ctxs = list(ctxs)
        arr = (_vp * len(ctxs))(*[c._h.value for c in ctxs])
        check(load().dsm_batch_gibbs_update(arr, len(ctxs), int(n_iter)))
        for c in ctxs:
            c.n_trace = int(n_iter)

    def update_tau(self, gamma_store, eta_store):
        g = np.ascontiguousarray(gamma_store, dtype=np.float64)
        e = np.ascontiguousarray(eta_store, dtype=np.float64)
        check(self.lib.dsm_ctx_update_tau(self._h, g.shape[0], g, e))
        self.n_trace = g.shape[0]

    def get_trace(self):
        n = self.n_trace
        ll = np.empty(n); lp = np.empty(n); nch = np.empty(n, dtype=np.int32)
        g = np.empty((n, self.S, self.G)); e = np.empty((n, 4, 4))
        check(self.lib.dsm_ctx_get_trace(self._h, _ptr(ll), _ptr(lp), _ptr(nch), _ptr(g), _ptr(e)))
        return dict(ll=ll, lp=lp, nchange=nch, gamma=g, eta=e)

    def get_star(self):
        tau = np.empty((self.V, self.G, 4), dtype=np.int64)
        g = np.empty((self.S, self.G)); e = np.empty((4, 4))
        lp, it = _d(0), _i(0)
        check(self.lib.dsm_ctx_get_star(self._h, _ptr(tau), _ptr(g), _ptr(e), C.byref(lp), C.byref(it)))
        return dict(tau=tau, gamma=g, eta=e, lp=lp.value, it=it.value)

    def get_tau_sum(self):
        out = np.empty((self.V, self.G, 4), dtype=np.int64)
        check(self.lib.dsm_ctx_get_tau_sum(self._h, out))
        return out

    def get_tau_at(self, it):
        out = np.empty((self.V, self.G, 4), dtype=np.int64)
        check(self.lib.dsm_ctx_get_tau_at(self._h, int(it), out))
        return out

    # ---- reductions of the resident traces (include/desman_hip.h: dsm_ctx_trace_snd and below; csrc/api_trace.hip)
    def _trace_n_it(self, it0, n_it):
        """n_it, or the iterations from it0 to the end of the trace"""
        return self.n_trace - int(it0) if n_it is None else int(n_it)

    def _trace_perm(self, who, perm, n_it=None):
        """perm as uint8 [n_it, G] labels (n_it None: any number of rows)"""
        p = np.ascontiguousarray(perm, dtype=np.uint8)
        fits = p.ndim == 2 and p.shape[1] == self.G and (n_it is None or p.shape[0] == max(n_it, 0))
        if not fits or not np.array_equal(p, np.asarray(perm)):
            raise ValueError("%s: perm must be [n_it%s, G=%d] labels 0..G-1" % (who, "" if n_it is None else "=%d" % n_it, self.G))
        return p

    @staticmethod
    def _trace_outputs(who, want, shapes, dtypes=None, strict=True):
        """the outputs of ``shapes`` (name -> shape, in the order of the C arguments) that ``want`` names as zeroed arrays, and one
        pointer per name of ``shapes`` (null: not fetched); strict: a name that ``shapes`` does not have is a ValueError"""
        bad = [k for k in want if k not in shapes]
        if bad and strict:
            raise ValueError("%s: unknown output %r (%s)" % (who, bad[0], ", ".join(shapes)))
        out = {k: np.zeros(shapes[k], dtype=(dtypes or {}).get(k, np.float64)) for k in shapes if k in want}
        return out, [_ptr(out.get(k)) for k in shapes]

    def trace_snd(self, mode=SND_STAR, ref=None, it0=0, n_it=None):
        """snd [n_it, G, Gr] int32: in how many positions haplotype g of stored iteration t differs from haplotype h of the reference --
        SND_STAR: the MAP record's tau; SND_SELF: the iteration itself; SND_GIVEN: ``ref`` ([V,Gr] digits or [V,Gr,4] one-hot)"""
        n_it = self._trace_n_it(it0, n_it)
        r, Gr = None, self.G
        if mode == SND_GIVEN:
            r = _fit_tau(ref, self.V)
            Gr = r.shape[1]
        out = np.zeros((max(n_it, 0), self.G, Gr), dtype=np.int32)
        check(self.lib.dsm_ctx_trace_snd(self._h, int(mode), _ptr(r), Gr if mode == SND_GIVEN else 0, int(it0), n_it, _ptr(out)))
        return out

    def get_tau_sum_perm(self, perm, it0=0):
        """get_tau_sum() over the iterations it0 .. it0 + len(perm) - 1 with iteration t's haplotype g counted as label perm[t, g]"""
        p = self._trace_perm("get_tau_sum_perm", perm)
        out = np.zeros((self.V, self.G, 4), dtype=np.int64)
        check(self.lib.dsm_ctx_get_tau_sum_perm(self._h, _ptr(p), int(it0), p.shape[0], _ptr(out)))
        return out

    def trace_batch_stats(self, batch_len, perm=None, it0=0, n_it=None, want=("sum", "first", "bsq", "flips")):
        """Batch sums of the tau trace for convergence diagnostics (include/desman_hip.h: dsm_ctx_trace_batch_stats;
        desman_amd/diagnose.py): with L = batch_len, B = 2 (n_it // (2 L)) and N = B L, over the LAST N of the iterations
        it0 .. it0 + n_it - 1 under the labels of ``perm`` ([n_it, G], rows counted from it0; None = identity) a dict of
        sum, first, bsq [V, G, 4] int64 and flips [V, G] int32 (those named in ``want``; the others are not fetched), B, N and L"""
        n_it = self._trace_n_it(it0, n_it)
        L = int(batch_len)
        p = perm if perm is None else self._trace_perm("trace_batch_stats", perm, n_it)
        vg4 = (self.V, self.G, 4)
        out, ptrs = self._trace_outputs("trace_batch_stats", want, dict(sum=vg4, first=vg4, bsq=vg4, flips=(self.V, self.G)),
                                        dict(sum=np.int64, first=np.int64, bsq=np.int64, flips=np.int32), strict=False)
        check(self.lib.dsm_ctx_trace_batch_stats(self._h, _ptr(p), int(it0), n_it, L, *ptrs))
        B = 2 * (n_it // (2 * L))
        out.update(B=B, N=B * L, L=L)
        return out

    def trace_fit_stats(self, it0=0, n_it=None, want=("sample", "position", "cell")):
        """Posterior predictive fit sums over the stored iterations it0 .. it0 + n_it - 1 (include/desman_hip.h:
        dsm_ctx_trace_fit_stats; desman_amd/check.py): a dict of sample [S, 4] and position [V, 4] -- the sums of (X, D, E, W) over the
        iterations and the other index -- and cell [V, S], the sum of X over the iterations; only those named in ``want`` are
        allocated and fetched.  n_it is in the dict."""
        n_it = self._trace_n_it(it0, n_it)
        out, ptrs = self._trace_outputs("trace_fit_stats", want, dict(sample=(self.S, 4), position=(self.V, 4), cell=(self.V, self.S)))
        check(self.lib.dsm_ctx_trace_fit_stats(self._h, int(it0), n_it, *ptrs))
        out["n_it"] = n_it
        return out

    def trace_rb_marginals(self, batch_len, perm=None, it0=0, n_it=None, want=("sum", "bsq")):
        """Rao-Blackwellised tau marginals of the positions of the fit (include/desman_hip.h: dsm_ctx_trace_rb_marginals;
        desman_amd/marginals.py): the full conditional q of every tau[v][g] under (tau_t, gamma_t, eta_t), over the LAST N = B L of the
        iterations it0 .. it0 + n_it - 1 (L = batch_len, B = 2 (n_it // (2 L))) under the labels of ``perm`` ([n_it, G], rows counted from
        it0; None = identity): a dict of sum and bsq [V, G, 4] float64 (those named in ``want``), dead, B, N and L"""
        n_it = self._trace_n_it(it0, n_it)
        L = int(batch_len)
        p = perm if perm is None else self._trace_perm("trace_rb_marginals", perm, n_it)
        vg4 = (self.V, self.G, 4)
        out, ptrs = self._trace_outputs("trace_rb_marginals", want, dict(sum=vg4, bsq=vg4))
        dead = C.c_longlong(0)
        check(self.lib.dsm_ctx_trace_rb_marginals(self._h, _ptr(p), int(it0), n_it, L, *ptrs, C.byref(dead)))
        B = 2 * (n_it // (2 * L)) if L >= 1 else 0
        out.update(dead=int(dead.value), B=B, N=B * L, L=L)
        return out

    def trace_rb_pairs(self, batch_len, perm=None, it0=0, n_it=None, stride=1, want=("joint", "same_batch")):
        """Rao-Blackwellised joint posterior of the bases of two haplotypes (include/desman_hip.h: dsm_ctx_trace_rb_pairs;
        desman_amd/marginals.py): the sixteen-state full conditional q of every (tau[v][g], tau[v][h]), g < h, under (tau_t, gamma_t,
        eta_t), over the iterations it0, it0 + stride, ... below it0 + n_it -- of these n_used the LAST N = B L (L = batch_len,
        B = 2 (n_used // (2 L))) -- under the labels of ``perm`` ([n_it, G], rows counted from it0; None = identity): a dict of joint
        [V, P, 4, 4] (the sum of q; [a, a'] = the bases of the lower and the higher label) and same_batch [B, P] float64 (those named in
        ``want``), pairs [P, 2] (the labels of every pair, lexicographic), dead, n_used, B, N and L"""
        n_it = self._trace_n_it(it0, n_it)
        L, stride = int(batch_len), int(stride)
        p = perm if perm is None else self._trace_perm("trace_rb_pairs", perm, n_it)
        n_used = -(-n_it // stride) if stride >= 1 and n_it > 0 else 0
        B = 2 * (n_used // (2 * L)) if L >= 1 else 0
        G = self.G
        P = G * (G - 1) // 2
        out, ptrs = self._trace_outputs("trace_rb_pairs", want, dict(joint=(self.V, P, 4, 4), same_batch=(B, P)))
        dead = C.c_longlong(0)
        check(self.lib.dsm_ctx_trace_rb_pairs(self._h, _ptr(p), int(it0), n_it, stride, L, *ptrs, C.byref(dead)))
        pairs = np.array([(g, h) for g in range(G) for h in range(g + 1, G)], dtype=np.int64).reshape(P, 2)
        out.update(pairs=pairs, dead=int(dead.value), n_used=n_used, B=B, N=B * L, L=L)
        return out

    def trace_predictive(self, counts=None, it0=0, n_it=None, stride=1, want=("lppd", "mean", "var")):
        """Position-marginal log predictive density over the stored iterations it0, it0 + stride, ... below it0 + n_it (include/
        desman_hip.h: dsm_ctx_trace_predictive; desman_amd/predictive.py): per position of ``counts`` [N, S, 4] -- None: the resident
        table -- logz[t] = ln of the sum over all 4^G haplotype states of exp L under (gamma_t, eta_t); a dict of lppd [N], mean [N],
        var [N] and, when named in ``want``, logz_it [n_used, N]; only those named are allocated and fetched.  n_used is in the dict.
        G <= ASSIGN_MAX_G."""
        n_it = self._trace_n_it(it0, n_it)
        stride = int(stride)
        x = None
        N = self.V
        if counts is not None:
            x = np.ascontiguousarray(counts, dtype=np.int64)
            if x.ndim != 3 or x.shape[1:] != (self.S, 4):
                raise ValueError("trace_predictive: counts must be [N, S=%d, 4]; got %s" % (self.S, x.shape))
            N = x.shape[0]
        n_used = -(-n_it // stride) if stride >= 1 and n_it > 0 else 0
        out, ptrs = self._trace_outputs("trace_predictive", want, dict(lppd=(N,), mean=(N,), var=(N,), logz_it=(n_used, N)))
        check(self.lib.dsm_ctx_trace_predictive(self._h, _ptr(x), N, int(it0), n_it, stride, *ptrs))
        out["n_used"] = n_used
        return out

    def trace_ppc(self, R, it0=0, n_it=None, stride=1, salt=0, want=("ge_sample", "ge_position", "rep_sample", "rep_position",
                                                                     "obs_sample", "obs_position")):
        """Posterior predictive p-values from R replicate tables per used iteration it0, it0 + stride, ... below it0 + n_it (include/
        desman_hip.h: dsm_ctx_trace_ppc; desman_amd/check.py): a dict of ge_sample [S] and ge_position [V] (int64: the (t, r) with
        T_rep >= T_obs), rep_sample [S, 2] and rep_position [V, 2] (the sums of T_rep and T_rep^2 over (t, r)), obs_sample [S] and
        obs_position [V] (the sum of T_obs over t); only those named in ``want`` are allocated and fetched.  n_used and R are in the
        dict; p = ge / (n_used R)."""
        n_it = self._trace_n_it(it0, n_it)
        stride, R = int(stride), int(R)
        out, ptrs = self._trace_outputs("trace_ppc", want, dict(ge_sample=(self.S,), ge_position=(self.V,), rep_sample=(self.S, 2),
                                                                rep_position=(self.V, 2), obs_sample=(self.S,), obs_position=(self.V,)),
                                        dict(ge_sample=np.int64, ge_position=np.int64))
        check(self.lib.dsm_ctx_trace_ppc(self._h, int(it0), n_it, stride, R, C.c_uint64(int(salt) & 0xFFFFFFFFFFFFFFFF), *ptrs))
        out["n_used"] = -(-n_it // stride) if stride >= 1 and n_it > 0 else 0
        out["R"] = R
        return out

    def ppc_debug_path(self, n_used=None, R=1):
        """test hook: what trace_ppc over n_used used iterations (default: the whole trace) and R replicates would launch: dict of nsl
        (the kernel's instantiation: sample slots per lane), lpv, gc, tiles, parts, ct and cr (iterations and replicates per launch) and
        C (cells of up to C reads are drawn read by read)"""
        out = (_i * 8)()
        check(self.lib.dsm_ppc_debug_path(self._h, int(self.n_trace if n_used is None else n_used), int(R), out))
        return dict(zip(("nsl", "lpv", "gc", "tiles", "parts", "ct", "cr", "C"), (int(x) for x in out)))

    def fit_debug_path(self, n_it=None):
        """test hook: what trace_fit_stats over n_it iterations (default: the whole trace) would launch: dict of nsl (the kernel's
        instantiation: sample slots per lane), lpv (lanes per position), gc (haplotypes per staged chunk of gamma), tiles and parts"""
        out = (_i * 5)()
        check(self.lib.dsm_fit_debug_path(self._h, int(self.n_trace if n_it is None else n_it), out))
        return dict(zip(("nsl", "lpv", "gc", "tiles", "parts"), (int(x) for x in out)))

    def debug_set_param_trace(self, gamma, eta):
        """test hook: installs gamma [n, S, G] and eta [n, 4, 4] as the first n rows of the gamma and eta traces (after
        debug_set_trace or an update)"""
        g = np.ascontiguousarray(gamma, dtype=np.float64)
        e = np.ascontiguousarray(eta, dtype=np.float64)
        if g.ndim != 3 or g.shape[1:] != (self.S, self.G) or e.shape != (g.shape[0], 4, 4):
            raise ValueError("debug_set_param_trace: gamma must be [n, S=%d, G=%d] and eta [n, 4, 4]" % (self.S, self.G))
        check(self.lib.dsm_ctx_debug_set_param_trace(self._h, _ptr(g), _ptr(e), g.shape[0]))

    def debug_set_trace(self, tau_digits):
        """test hook: installs tau_digits [n, V, G] (digits 0..3) as the tau trace of n iterations; slot 0 = the resident state"""
        t = np.ascontiguousarray(tau_digits, dtype=np.int64)
        if t.ndim != 3 or t.shape[1:] != (self.V, self.G):
            raise ValueError("debug_set_trace: tau_digits must be [n, V=%d, G=%d]" % (self.V, self.G))
        check(self.lib.dsm_ctx_debug_set_trace(self._h, _ptr(t), t.shape[0]))
        self.n_trace = t.shape[0]

    # ---- NMFT
    def nmft_set(self, tau, gamma):
        tau = np.ascontiguousarray(tau, dtype=np.float64)
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        G = gamma.shape[0]
        if tau.shape != (4 * self.V, G) or gamma.shape[1] != self.S:
            raise ValueError("NMFT factor shapes do not match the count tensor")
        check(self.lib.dsm_nmft_set(self._h, tau, gamma, G))
        self.nG = G

    def nmft_get(self):
        tau = np.empty((4 * self.V, self.nG)); gamma = np.empty((self.nG, self.S))
        check(self.lib.dsm_nmft_get(self._h, _ptr(tau), _ptr(gamma)))
        return tau, gamma

    def nmft_factorize(self, max_iter=5000, min_change=1e-5, fix_gamma=False):
        n = _i(0)
        tr = np.full(max_iter + 1, np.nan)
        check(self.lib.dsm_nmft_factorize(self._h, int(max_iter), float(min_change), int(bool(fix_gamma)),
                                          C.byref(n), _ptr(tr)))
        return n.value, tr[: n.value + 1]

    @staticmethod
    def batch_update_tau(ctxs, gamma_stores, eta_stores):
        """update_tau of every context in ``ctxs`` with shared launches (dsm_batch_update_tau); one (gamma_store, eta_store)
        pair of equal length per context"""
        ctxs = list(ctxs)
        gs = [np.ascontiguousarray(g, dtype=np.float64) for g in gamma_stores]
        es = [np.ascontiguousarray(e, dtype=np.float64) for e in eta_stores]
        n = gs[0].shape[0]
        if any(g.shape[0] != n for g in gs) or any(e.shape[0] != n for e in es):
            raise ValueError("batch_update_tau: traces of equal length expected")
        arr = (_vp * len(ctxs))(*[c._h.value for c in ctxs])
        gp = (_vp * len(ctxs))(*[g.ctypes.data for g in gs])
        ep = (_vp * len(ctxs))(*[e.ctypes.data for e in es])
        check(load().dsm_batch_update_tau(arr, len(ctxs), int(n), gp, ep))
        for c in ctxs:
            c.n_trace = int(n)

    @staticmethod
    def batch_nmft_factorize(ctxs, max_iter=5000, min_change=1e-5, fix_gamma=False):
        """nmft_factorize of every context in ``ctxs`` (one shape, one device, at most 8) with shared launches
        (include/desman_hip.h: dsm_batch_nmft_factorize) -> [(updates run, objective trace), ...]"""
        ctxs = list(ctxs)
        arr = (_vp * len(ctxs))(*[c._h.value for c in ctxs])
        n = (_i * len(ctxs))()
        tr = np.full((len(ctxs), max_iter + 1), np.nan)
        check(load().dsm_batch_nmft_factorize(arr, len(ctxs), int(max_iter), float(min_change), int(bool(fix_gamma)), n,
                                              tr.ctypes.data_as(_vp)))
        return [(int(n[k]), tr[k, : n[k] + 1].copy()) for k in range(len(ctxs))]

    def nmft_objective(self):
        d = _d(0)
        check(self.lib.dsm_nmft_objective(self._h, C.byref(d)))
        return d.value

    def nmft_debug_path(self, fix_gamma=False):
        """test hook: which kernels nmft_factorize(fix_gamma=...) takes for this context, nothing launched
        (include/desman_hip.h: dsm_nmft_debug_path) -> dict"""
        out = (_i * 8)()
        check(self.lib.dsm_nmft_debug_path(self._h, int(bool(fix_gamma)), out))
        fam, nt, kb, ncb, nwv, grid, lds, flags = (int(x) for x in out)
        return {"family": ("two-pass", "mfma", "split", "persist")[fam], "NT": nt, "KB": kb, "NCB": ncb, "NWV": nwv, "grid": grid,
                "lds": lds, "xpar": bool(flags & 1), "gstep": bool(flags & 2), "VT": (flags >> 8) & 255, "cus": flags >> 16}

    def nmft_get_tau(self):
        out = np.empty((self.V, self.nG, 4), dtype=np.int64)
        check(self.lib.dsm_nmft_get_tau(self._h, out))
        return out

    # ---- timing
    def set_timing(self, on):
        check(self.lib.dsm_ctx_set_timing(self._h, int(bool(on))))

    def get_timing(self):
        ms = np.zeros(len(K_NAMES)); n = np.zeros(len(K_NAMES), dtype=np.int64)
        check(self.lib.dsm_ctx_get_timing(self._h, _ptr(ms), _ptr(n)))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(K_NAMES)}


def kl_assign(cov, delta, eta, max_iter=10000, min_change=1.0e-4, device=0):
    """GeneAssign.KLAssign.factorize on the GPU: returns (eta [C,G], n_updates, divergence)."""
    cov = np.ascontiguousarray(cov, dtype=np.float64)
    delta = np.ascontiguousarray(delta, dtype=np.float64)
    eta = np.ascontiguousarray(eta, dtype=np.float64).copy()
    n, div = C.c_int(0), C.c_double(0.0)
    check(load().dsm_kl_assign(int(device), cov, delta, eta, cov.shape[0], cov.shape[1], delta.shape[1], int(max_iter),
                               float(min_change), C.byref(n), C.byref(div)))
    return eta, n.value, div.value


class Genes:
    """Device-resident accessory-gene sampler state (dsm_genes): all genes' variant rows in one tensor."""

    def __init__(self, device=0):
        self._h = _vp()
        check(load().dsm_genes_create(C.byref(self._h), int(device)))
        self.C = self.S = self.G = self.Vtot = 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            load().dsm_genes_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, variants, gene_off, cov):
        cov = np.ascontiguousarray(cov, dtype=np.float64)
        gene_off = np.ascontiguousarray(gene_off, dtype=np.int32)
        self.C, self.S = cov.shape
        self.Vtot = int(gene_off[-1])
        if self.Vtot:
            variants = np.ascontiguousarray(variants, dtype=np.int64)
            assert variants.shape == (self.Vtot, self.S, 4), variants.shape
        else:
            variants = None
        self.gene_off = gene_off
        check(load().dsm_genes_set_data(self._h, _ptr(variants), self.Vtot, self.S, self.C, gene_off, cov))

    def set_model(self, gamma, epsilon, delta_gs, max_eta, eta_log_prior, cov_const, mult_const):
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        self.G = gamma.shape[1]
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        check(load().dsm_genes_set_model(self._h, gamma, f(epsilon), f(delta_gs), self.G, int(max_eta), f(eta_log_prior),
                                         f(cov_const), f(mult_const)))

    def set_state(self, eta=None, tau=None):
        eta = None if eta is None else np.ascontiguousarray(eta, dtype=np.int32)
        tau = None if tau is None else np.ascontiguousarray(tau, dtype=np.int64)
        check(load().dsm_genes_set_state(self._h, _ptr(eta), _ptr(tau)))

    def get_state(self, want_tau=True):
        eta = np.empty((self.C, self.G), dtype=np.int32)
        tau = np.zeros((self.Vtot, self.G, 4), dtype=np.int64) if want_tau else None
        check(load().dsm_genes_get_state(self._h, _ptr(eta), _ptr(tau)))
        return eta, tau

    def seed(self, mt_seed, ctr_seed=0x13198A2E03707344):
        check(load().dsm_genes_seed(self._h, int(mt_seed), int(ctr_seed)))

    def set_gene_base(self, gene_base):
        check(load().dsm_genes_set_gene_base(self._h, int(gene_base)))

    def get_mt_state(self):
        st = np.empty(625, dtype=np.uint32)
        check(load().dsm_genes_get_mt_state(self._h, st))
        return st

    def set_mt_state(self, st):
        check(load().dsm_genes_set_mt_state(self._h, np.ascontiguousarray(st, dtype=np.uint32)))

    def _mask(self, eta_mask):
        return None if eta_mask is None else np.ascontiguousarray(eta_mask, dtype=np.int32)

    def nmft_tau(self, tau_init, eta_mask=None, max_iter=5000, min_change=1.0e-5):
        """tau_init [Vtot,4,G]; returns the per-gene update counts (-1 = gene skipped)."""
        tau_init = np.ascontiguousarray(tau_init, dtype=np.float64)
        n = np.empty(self.C, dtype=np.int32)
        m = self._mask(eta_mask)
        check(load().dsm_genes_nmft_tau(self._h, _ptr(m), tau_init, int(max_iter), float(min_change), _ptr(n)))
        return n

    def sweep_all(self, eta_mask=None, sweep=True, want_v_ll=False):
        nch = np.empty(self.C, dtype=np.int32)
        lv = np.empty(self.C)
        vll = np.empty(self.Vtot) if want_v_ll else None
        m = self._mask(eta_mask)
        check(load().dsm_genes_sweep_all(self._h, _ptr(m), int(sweep), _ptr(nch), _ptr(lv), _ptr(vll)))
        return nch, lv, vll

    def step_candidates(self, c, g):
        lv = np.empty(2)
        sw = np.empty(2, dtype=np.int32)
        check(load().dsm_genes_step_candidates(self._h, int(c), int(g), lv, _ptr(sw)))
        return lv, sw

    def step_choose(self, c, g, value):
        check(load().dsm_genes_step_choose(self._h, int(c), int(g), int(value)))

    def update(self, n_iter, reset_star=True, u_tau_ext=None, u_eta_ext=None):
        store = np.empty((n_iter, self.C, self.G), dtype=np.int32)
        trace = np.empty((n_iter, self.C))
        ut = None if u_tau_ext is None else np.ascontiguousarray(u_tau_ext, dtype=np.uint32)
        ue = None if u_eta_ext is None else np.ascontiguousarray(u_eta_ext, dtype=np.float64)
        check(load().dsm_genes_update(self._h, int(n_iter), int(bool(reset_star)), _ptr(store), _ptr(trace), _ptr(ut), _ptr(ue)))
        return store, trace

    def loglik(self):
        ll = np.empty(self.C)
        check(load().dsm_genes_loglik(self._h, _ptr(ll)))
        return ll

    def get_star(self):
        es = np.empty((self.C, self.G), dtype=np.int32)
        ls = np.empty(self.C)
        check(load().dsm_genes_get_star(self._h, _ptr(es), _ptr(ls)))
        return es, ls

    def set_star(self, eta_star, gene_llstar):
        check(load().dsm_genes_set_star(self._h, _ptr(np.ascontiguousarray(eta_star, dtype=np.int32)),
                                        _ptr(np.ascontiguousarray(gene_llstar, dtype=np.float64))))

    def debug_tile(self):
        """test hook: (lanes per variant row, samples per lane, lane groups per workgroup, dynamic LDS bytes) of a sweep launch"""
        lpv, nsl, gpb, lds = _i(0), _i(0), _i(0), C.c_size_t(0)
        check(load().dsm_genes_debug_tile(self._h, C.byref(lpv), C.byref(nsl), C.byref(gpb), C.byref(lds)))
        return lpv.value, nsl.value, gpb.value, lds.value
