"""Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 specification) in vectorised
numpy, and the tau sweep's counter-based uniforms built on it -- an implementation that shares no code with the kernels or with
oracle/desman_oracle.c: orc_philox4x32_10, against which tests/test_philox_cpu.py checks it.

Layout of the sweep's uniforms (kernels_gibbs.hip: tau_body): the step of haplotype g at global position v takes word 0
of Philox(counter = (lo32(i), hi32(i), it, 'TAUU'), key = (lo32(ctr_seed), hi32(ctr_seed))), i = v * G + g, as u32 / 2^32."""
import numpy as np

STREAM_TAUU = 0x54415555                      # 'TAUU' (dsm_device.h: DSM_STREAM_TAUU)
# the keys the chain tests run: both words non-zero and different (tells a dropped or swapped key word), a zero low word, and the small
# key of the older one-sweep check (tests/test_gpu_edges.py), whose high word is 0
CTR_SEEDS = (0x5EEDC0DE00000001, 0xABCDEF0100000000, 777)
_M32, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)     # the round multipliers
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)         # the Weyl increments of the key schedule


def philox4x32_10(ctr, key):
    """ctr [N,4], key [2] (one key for all counters) or [N,2] -> [N,4] uint32"""
    c = np.asarray(ctr, dtype=np.uint64).reshape(-1, 4) & _M32
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64).reshape(-1, 2) & _M32, (c.shape[0], 2))
    c0, c1, c2, c3 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    k0, k1 = k[:, 0], k[:, 1]
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2                         # 32 x 32 -> 64 bit products: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _W0) & _M32, (k1 + _W1) & _M32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def _uniforms(key, it, V, G, v_off=0):
    i = np.arange(V * G, dtype=np.uint64) + np.uint64(v_off * G)
    ctr = np.stack([i & _M32, i >> _S32, np.full_like(i, int(it)), np.full_like(i, STREAM_TAUU)], axis=1)
    return philox4x32_10(ctr, key)[:, 0].astype(np.float64) / 4294967296.0


def tau_uniforms(ctr_seed, it, V, G, v_off=0):
    """the V * G uniforms of the sweep with iteration counter ``it`` of a chain keyed ``ctr_seed``, in the (v, g) order
    cbind.sample_tau_u consumes; v_off = first global position of a shard"""
    return _uniforms([int(ctr_seed) & 0xFFFFFFFF, int(ctr_seed) >> 32], it, V, G, v_off)


def wrong_tau_uniforms(ctr_seed, it, V, G):
    """what three plausible mistakes would draw instead (name -> uniforms): the counter one ahead, the key's high word dropped, the
    key's words swapped.  A variant that is no mistake for this key (high word 0, or equal words) is left out."""
    lo, hi = int(ctr_seed) & 0xFFFFFFFF, int(ctr_seed) >> 32
    out = {"it + 1": _uniforms([lo, hi], (int(it) + 1) & 0xFFFFFFFF, V, G)}
    if hi != 0:
        out["high key word dropped"] = _uniforms([lo, 0], it, V, G)
    if hi != lo:
        out["key words swapped"] = _uniforms([hi, lo], it, V, G)
    return out
