// dsm_big_item.h -- one deferred stage-1 item (kernels_stats.hip: the lists stage 1 hands over), drawn by whoever consumes its list:
// stats_big_kernel (one lane per item of a list) or, where that launch was left out, the workgroup of the item's sample in the launch
// that runs stage 2 (dsm_stage2.h: s2_inline_items).  An item's stream is keyed by the item (cell, observed base, iteration), so who
// draws it does not change the draw; its reads are added to N[row(H, s)][s] here, the caller adds n[.] to its Esum accumulators.
#pragma once
#include "dsm_binom.h"

struct BigItemParams {
    const int32_t *cnt_vs;          // [V][S][4]
    const uint64_t *tau;            // [V]
    const double *gamma;            // [S][G] the abundances stage 1 ran with
    uint32_t *pat_x;                // spec 4: the pooled counts (consumed here, left zero), else null
    uint32_t *ntab;                 // [rep][2^G][ld]
    int rep, ld;
    int S, G, v_off, V_tot;
    uint32_t k0, k1, iter, hmul, swz;
};

// the sample of an item (list entry = cell * 4 + observed base, cell = s * V_tot + global position)
__device__ __forceinline__ int big_item_sample(const BigItemParams &p, unsigned long long item) { return (int)((uint32_t)(item >> 2) / (uint32_t)p.V_tot); }

// es: eta [4][4] (true, observed) in LDS; rcp / ltab: the samplers' tables in LDS (log table, then the exp table).  Returns the observed base.
template <int SPEC>
__device__ __forceinline__ int big_item_draw(const BigItemParams &p, unsigned long long item, unsigned copy, const double *es, const double *rcp,
                                             const double2 *ltab, uint32_t (&n)[4])
{
    const int S = p.S, G = p.G;
    const uint32_t cell = (uint32_t)(item >> 2);
    const int b = (int)(item & 3ull);
    const int s = (int)(cell / (uint32_t)p.V_tot), v = (int)(cell - (uint32_t)s * (uint32_t)p.V_tot) - p.v_off;
    const uint64_t t = p.tau[v];
    uint32_t xb;
    if (p.pat_x) { uint32_t *xw = p.pat_x + ((size_t)v * 4 + b) * S + s; xb = *xw; *xw = 0u; }     // spec 4: consumed here (see stats_agg_body)
    else xb = (uint32_t)p.cnt_vs[((size_t)v * S + s) * 4 + b];
    uint32_t H[4] = {0, 0, 0, 0};
    double Gam[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < G; ++g) {
        const int a = (int)((t >> (2 * g)) & 3);
        const double x = p.gamma[(size_t)s * G + g];
#pragma unroll
        for (int k = 0; k < 4; ++k) if (a == k) { H[k] |= 1u << g; Gam[k] = Gam[k] + x; }
    }
    double W[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) W[a] = es[a * 4 + b] * Gam[a];
    const double Wt = ((W[0] + W[1]) + W[2]) + W[3];
    if (!(Wt > 0.0)) {
#pragma unroll
        for (int a = 0; a < 4; ++a) W[a] = Gam[a];
    }
    uint32_t cbase[4];
    philox4x32_10(cell, 0u, p.iter, DSM_STREAM_STA1, p.k0, p.k1, cbase);
    Xo128 rng = item_seed<SPEC>(cbase, (uint32_t)b, p.k0, p.k1);
    bool defer = false;
    mult4<true, SPEC>(rng, xb, W, n, rcp, ltab, defer);
    uint32_t *const nt = p.ntab + (size_t)(copy % (unsigned)p.rep) * (((size_t)1 << G) * (size_t)p.ld);
#pragma unroll
    for (int a = 0; a < 4; ++a)
        if (n[a]) atomicAdd(nt + (size_t)((H[a] * p.hmul + ((uint32_t)s >> 4) * p.swz) & ((1u << G) - 1u)) * (size_t)p.ld + s, n[a]);
    return b;
}
