// kernels_heldtau.hip -- the gfx950 kernel of the partly held chain (api.hip: dsm_ctx_sample_tau_held, dsm_ctx_gibbs_update_held_tau;
// DESIGN.md sec. 8e).
//
//   held_sweep_kernel<LPV, NSL>   one tau sweep over the FREE haplotypes 0 .. F-1 of every position; the last G - F digits of a
//                                 packed word are only read
//
// The chain around it runs on the launchers of the Gibbs loop (kernels_stats.hip, kernels_gibbs.hip).
#include "dsm_sweep_tile.h"

struct HeldParams : SweepTileParams {
    const uint32_t *u_raw;     // MT19937 words, [V][F]; null -> Philox
    int F;                     // free haplotypes
};

// The frame of dsm_sweep_tile.h: one group of LPV lanes per position, NSL sample slots per lane (slot j of lane l = sample l + j LPV).
// Step g < F is the step of c_sample_tau.c:136-190 in plain fp64: the rest mixture is the h-ascending fma chain over ALL h != g --
// the links h < g (already re-drawn, final for this sweep) are carried from step to step, the links h > g, the held haplotypes among
// them, are re-done: the same operations in the same order as the chain from zero --, the four candidates are lane-partial sums
// (sweep_candidate) reduced over the group, and every lane of the group makes the same draw (sweep_draw).  No fp32 screening pass, no
// near-tie path, no re-use of the current candidate's value.  A held haplotype costs one link per free step and nothing else: no
// candidates, no reduction, no uniform.
// Uniforms: MT19937 word v F + g (a sweep consumes V F words, position-major, free haplotype ascending); Philox: the key of the full
// sweep's step (position v, haplotype g of G, iteration), tau_body in kernels_gibbs.hip.
template <int LPV, int NSL>
__global__ __launch_bounds__(256) void held_sweep_kernel(HeldParams p)
{
    constexpr int SP = LPV * NSL;
    constexpr int GPB = 256 / LPV;
    const int tid = threadIdx.x, G = p.G, S = p.S, F = p.F;
    const SweepTileLds lds = sweep_tile_stage<LPV, NSL>(p, 1.0);      // padded slot: abundance 1, count 0 (dsm_device.h: sweep_candidate)
    const double *gT = lds.gT, *eS = lds.eS;
    const double2 *ltab = lds.ltab;

    const int grp = tid / LPV, lig = tid % LPV;
    int nchg = 0;
    for (int v = (int)blockIdx.x * GPB + grp; v < p.V; v += (int)gridDim.x * GPB) {
        uint64_t t = p.tau[v];
        int4 c[NSL];
        sweep_tile_counts<LPV, NSL>(p, v, lig, c);
        double xf[NSL][4], pre[NSL][4];
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            xf[j][0] = (double)(float)c[j].x; xf[j][1] = (double)(float)c[j].y;      // c_sample_tau.c:164
            xf[j][2] = (double)(float)c[j].z; xf[j][3] = (double)(float)c[j].w;
#pragma unroll
            for (int b = 0; b < 4; ++b) pre[j][b] = 0.0;
        }
        for (int g = 0; g < F; ++g) {
            double gg[NSL], st[NSL][4];
#pragma unroll
            for (int j = 0; j < NSL; ++j) {
                gg[j] = gT[g * SP + lig + j * LPV];
#pragma unroll
                for (int b = 0; b < 4; ++b) st[j][b] = pre[j][b];
            }
#pragma unroll 2
            for (int h = g + 1; h < G; ++h) {
                const double *er = eS + (int)((t >> (2 * h)) & 3) * 4;
                const double e0 = er[0], e1 = er[1], e2 = er[2], e3 = er[3];
#pragma unroll
                for (int j = 0; j < NSL; ++j) {
                    const double gm = gT[h * SP + lig + j * LPV];
                    st[j][0] = fma(e0, gm, st[j][0]);
                    st[j][1] = fma(e1, gm, st[j][1]);
                    st[j][2] = fma(e2, gm, st[j][2]);
                    st[j][3] = fma(e3, gm, st[j][3]);
                }
            }
            double l[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) l[a] = sweep_candidate<NSL>(a, xf, st, gg, eS, ltab, lig, LPV, S);
            group_allreduce_sum4<LPV>(l[0], l[1], l[2], l[3]);
            uint32_t uw;
            if (p.u_raw) {
                uw = p.u_raw[(size_t)v * F + g];
            } else {
                uint32_t r[4];
                const size_t ug = (size_t)v * G + g;
                philox4x32_10((uint32_t)ug, (uint32_t)(ug >> 32), p.iter, DSM_STREAM_TAUU, p.k0, p.k1, r);
                uw = r[0];
            }
            const int told = (int)((t >> (2 * g)) & 3);
            const int tn = sweep_draw(l, uw);
            nchg += (lig == 0) & (tn != told);
            t = (t & ~(3ull << (2 * g))) | ((uint64_t)tn << (2 * g));
            const double *er = eS + tn * 4;                                     // link g of the chain, with the new base
            const double e0 = er[0], e1 = er[1], e2 = er[2], e3 = er[3];
#pragma unroll
            for (int j = 0; j < NSL; ++j) {
                pre[j][0] = fma(e0, gg[j], pre[j][0]);
                pre[j][1] = fma(e1, gg[j], pre[j][1]);
                pre[j][2] = fma(e2, gg[j], pre[j][2]);
                pre[j][3] = fma(e3, gg[j], pre[j][3]);
            }
        }
        if (lig == 0) p.tau[v] = t;
    }
    sweep_tile_nchange(p.nchange, nchg);
}

// One held sweep of the resident tau: haplotypes 0 .. G - n_held - 1 re-drawn with (gamma, eta), changed (v, g) pairs added to *c->nchange.
// u_raw: V (G - n_held) MT19937 words (ignored in Philox mode, where `iter` keys the draws).  0 < n_held < G: the ends are the callers'.
int k_held_sweep(dsm_ctx *c, int n_held, const double *gamma, const double *eta, uint32_t iter, const uint32_t *u_raw)
{
    KTimer tm(c, DSM_K_TAU);
    const int S = c->S, G = c->G, V = c->V;
    if (n_held < 1 || n_held >= G) { dsm_set_error("held sweep: n_held = %d outside 1..%d", n_held, G - 1); return DSM_ERR_ARG; }
    HeldParams p;
    p.cnt_vs = c->cnt_vs; p.tau = c->tau; p.gamma = gamma; p.eta = eta;
    p.u_raw = c->tau_rng == DSM_RNG_MT19937 ? u_raw : nullptr;
    if (c->tau_rng == DSM_RNG_MT19937 && !u_raw) { dsm_set_error("held sweep: no MT19937 words"); return DSM_ERR_STATE; }
    p.log_tab = c->log_tab; p.nchange = c->nchange;
    p.V = V; p.S = S; p.G = G; p.F = G - n_held;
    p.k0 = (uint32_t)c->ctr_seed; p.k1 = (uint32_t)(c->ctr_seed >> 32); p.iter = iter;
    return sweep_tile_dispatch(p, "", "held sweep", [&](auto L, auto N, int grid, size_t sh) {
        return sweep_tile_launch<held_sweep_kernel<L.value, N.value>>(c, p, grid, sh);
    });
}
