// kernels_pairtau.hip -- the pair pass of the main Gibbs chain (api.hip: dsm_ctx_sample_tau_pairs, dsm_ctx_set_pair_moves; DESIGN.md
// sec. 8i).
//
//   pair_sweep_kernel<LPV, NSL>   one pass over the pairs (g, h), g < h, of every position of the resident tau, in lexicographic order:
//                                 a block-Gibbs step that redraws both digits from their joint sixteen-state conditional
//
// The arithmetic is that of the pair step of dsm_assign_tau_sampled_pairs (the header comment of kernels_assign_sampled.hip):
//     m_a[s]    = sum_{k != g, h; a_k = a} gamma[s][k]                      (k in order)
//     rest[s][b]= ((m_0 eta[0][b] + m_1 eta[1][b]) + m_2 eta[2][b]) + m_3 eta[3][b]
//     L_k       = sum_{s,b: x > 0} x[s][b] ln((rest[s][b] + eta[a][b] gamma[s][g]) + eta[a'][b] gamma[s][h]),  k = 4 a + a'
//     q_k       = exp(L_k - max) / (e_0 + e_1 + ... + e_15, in this order);  all sixteen -inf: the pair stays
//     new pair  = inverse CDF over ascending k (the last edge forced),
//     u         = word 0 / 2^32 of Philox4x32-10(key = the chain's counter seed (lo32, hi32); counter = (lo32 j, hi32 j, iteration
//                 counter, DSM_STREAM_TPAR)),  j = position G^2 + g G + h
// The uniforms are Philox words in every tau RNG mode: the MT19937 stream of the single-site sweep is never touched.
#include "dsm_sweep_tile.h"

// The frame of dsm_sweep_tile.h: one group of LPV lanes per position, gamma transposed ([g][slot]; a padded slot holds abundance 0 under
// count 0: its mixture value is 0, never positive-normal, and an unseen cell adds nothing -- dsm_pair_candidates_row), eta and the
// logarithm's table in LDS.  A step forms the sixteen totals four at a time (one a, four a') from the m of the step; each row meets
// over the lane group by the DPP butterfly (no barrier: a group never spans wavefronts), so every lane of the group holds the same
// sixteen values, makes the same draw (dsm_pair_draw16), and lane 0 writes the word once per position.
template <int LPV, int NSL>
__global__ __launch_bounds__(256) void pair_sweep_kernel(SweepTileParams p)      // the pass needs no parameter of its own
{
    constexpr int SP = LPV * NSL;
    constexpr int GPB = 256 / LPV;
    const int tid = threadIdx.x, G = p.G;
    const SweepTileLds lds = sweep_tile_stage<LPV, NSL>(p, 0.0);
    const double *gT = lds.gT, *eS = lds.eS;
    const double2 *ltab = lds.ltab;

    const int grp = tid / LPV, lig = tid % LPV;
    const double NINF = -INFINITY;
    int nchg = 0;
    for (int v = (int)blockIdx.x * GPB + grp; v < p.V; v += (int)gridDim.x * GPB) {
        uint64_t t = p.tau[v];
        int4 c[NSL];
        sweep_tile_counts<LPV, NSL>(p, v, lig, c);
        double x[NSL][4];
#pragma unroll
        for (int j = 0; j < NSL; ++j) { x[j][0] = (double)c[j].x; x[j][1] = (double)c[j].y; x[j][2] = (double)c[j].z; x[j][3] = (double)c[j].w; }
        const unsigned long long jbase = (unsigned long long)v * (unsigned long long)G * (unsigned long long)G;
        for (int g = 0; g < G; ++g)
            for (int h = g + 1; h < G; ++h) {
                double m0[NSL], m1[NSL], m2[NSL], m3[NSL], gg[NSL], gh[NSL];
#pragma unroll
                for (int j = 0; j < NSL; ++j) { m0[j] = 0.0; m1[j] = 0.0; m2[j] = 0.0; m3[j] = 0.0; gg[j] = 0.0; gh[j] = 0.0; }
                for (int k = 0; k < G; ++k) {
                    const bool isg = k == g, ish = k == h;
                    const int d = (isg || ish) ? 4 : (int)(t >> (2 * k)) & 3;
#pragma unroll
                    for (int j = 0; j < NSL; ++j) {
                        const double ga = gT[k * SP + lig + j * LPV];
                        m0[j] += d == 0 ? ga : 0.0;
                        m1[j] += d == 1 ? ga : 0.0;
                        m2[j] += d == 2 ? ga : 0.0;
                        m3[j] += d == 3 ? ga : 0.0;
                        gg[j] = isg ? ga : gg[j];
                        gh[j] = ish ? ga : gh[j];
                    }
                }
                // the sixteen totals, kept in registers: row a is placed by selects, not by an indexed store
                double L[16], mx = NINF;
#pragma unroll
                for (int k = 0; k < 16; ++k) L[k] = 0.0;
#pragma unroll 1
                for (int a = 0; a < 4; ++a) {                           // four candidates at a time: the register budget of a single-site step
                    double R[4];
                    dsm_pair_candidates_row<NSL>(x, m0, m1, m2, m3, gg, gh, eS, ltab, a, R);
                    group_allreduce_sum4<LPV>(R[0], R[1], R[2], R[3]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) mx = R[i] > mx ? R[i] : mx;
                    dsm_put_row(L, a, R);
                }
                if (mx == NINF) continue;                               // group-uniform: the pair stays, its uniform is spent unseen
                const unsigned long long jj = jbase + (unsigned long long)(g * G + h);
                uint32_t w[4];
                philox4x32_10((uint32_t)jj, (uint32_t)(jj >> 32), p.iter, DSM_STREAM_TPAR, p.k0, p.k1, w);
                const double u = (double)w[0] * 2.3283064365386963e-10;
                const int kn = dsm_pair_draw16<false>(L, mx, u);
                const int ng = kn >> 2, nh = kn & 3;
                const int og = (int)(t >> (2 * g)) & 3, oh = (int)(t >> (2 * h)) & 3;
                nchg += (lig == 0) ? (int)(ng != og) + (int)(nh != oh) : 0;
                t = (t & ~((3ull << (2 * g)) | (3ull << (2 * h)))) | ((uint64_t)ng << (2 * g)) | ((uint64_t)nh << (2 * h));
            }
        if (lig == 0) p.tau[v] = t;
    }
    sweep_tile_nchange(p.nchange, nchg);
}

// test hook: the (LPV, NSL) of the instantiation k_pair_sweep launches for S samples (the sweep's own tiling: tau_shape)
extern "C" int dsm_pairtau_debug_path(int S, int G, int out[2])
{
    if (!out) { dsm_set_error("pairtau_debug_path: null pointer"); return DSM_ERR_ARG; }
    if (S < 1 || G < 1) { dsm_set_error("pairtau_debug_path: S=%d, G=%d", S, G); return DSM_ERR_ARG; }
    if (G > DSM_MAX_G) { dsm_set_error("pairtau_debug_path: G=%d exceeds DSM_MAX_G=%d", G, DSM_MAX_G); return DSM_ERR_UNSUPPORTED; }
    int LPV, NSL;
    { const int rc = tau_shape(S, &LPV, &NSL); if (rc != DSM_OK) return rc; }
    out[0] = LPV; out[1] = NSL;
    return DSM_OK;
}

// One pair pass over the resident tau with (gamma, eta), keyed by `iter`; the changed digits are added to *c->nchange.  G < 2: no pair.
int k_pair_sweep(dsm_ctx *c, const double *gamma, const double *eta, uint32_t iter)
{
    const int S = c->S, G = c->G, V = c->V;
    if (G < 2 || V < 1) return DSM_OK;
    KTimer tm(c, DSM_K_TAU);
    SweepTileParams p;
    p.cnt_vs = c->cnt_vs; p.tau = c->tau; p.gamma = gamma; p.eta = eta;
    p.log_tab = c->log_tab; p.nchange = c->nchange;
    p.V = V; p.S = S; p.G = G;
    p.k0 = (uint32_t)c->ctr_seed; p.k1 = (uint32_t)(c->ctr_seed >> 32); p.iter = iter;
    return sweep_tile_dispatch(p, "pair pass: ", "pair pass", [&](auto L, auto N, int grid, size_t sh) {
        return sweep_tile_launch<pair_sweep_kernel<L.value, N.value>>(c, p, grid, sh);
    });
}
