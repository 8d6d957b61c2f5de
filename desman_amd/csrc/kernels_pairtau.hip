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
#include <math.h>

#include <algorithm>

#include "dsm_device.h"
#include "dsm_host.h"
#include "log_table.h"

struct PairParams {
    const int32_t *cnt_vs;     // [V][S][4]
    uint64_t *tau;             // [V] packed, 2 bits per haplotype
    const double *gamma, *eta; // [S][G], [4][4]
    const double *log_tab;     // [256][2]
    int *nchange;
    int V, S, G;
    uint32_t k0, k1, iter;
};

// One group of LPV lanes per position, NSL sample slots per lane (slot j of lane l = sample l + j LPV; kernels_gibbs.hip: tau_shape),
// gamma transposed ([g][slot]; a padded slot holds abundance 0 under count 0: its mixture value is 0, never positive-normal, and an
// unseen cell adds nothing -- dsm_pair_candidates_row), eta and the logarithm's table in LDS.  A step forms the sixteen totals four at a
// time (one a, four a') from the m of the step; each row meets over the lane group by the DPP butterfly (no barrier: a group never
// spans wavefronts), so every lane of the group holds the same sixteen values, makes the same draw, and lane 0 writes the word once
// per position.  Nothing between two positions of the grid-stride loop is shared, and the loop has no barrier: groups of one wavefront
// may leave it at different times.
template <int LPV, int NSL>
__global__ __launch_bounds__(256) void pair_sweep_kernel(PairParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem_p[];
    constexpr int SP = LPV * NSL;
    constexpr int GPB = 256 / LPV;
    const int tid = threadIdx.x, G = p.G, S = p.S;
    double *gT = reinterpret_cast<double *>(smem_p);                 // [G][SP]
    double *eS = gT + (size_t)G * SP;                                  // [16]
    double2 *ltab = reinterpret_cast<double2 *>(eS + 16);             // [256] log table
    __shared__ int redi[4];
    if (tid < DSM_LOG_TAB_N) ltab[tid] = reinterpret_cast<const double2 *>(p.log_tab)[tid];
    for (int i = tid; i < G * SP; i += 256) {
        const int g = i / SP, s = i % SP;
        gT[i] = (s < S) ? p.gamma[(size_t)s * G + g] : 0.0;
    }
    if (tid < 16) eS[tid] = p.eta[tid];
    __syncthreads();

    const int grp = tid / LPV, lig = tid % LPV;
    const double NINF = -INFINITY;
    int nchg = 0;
    for (int v = (int)blockIdx.x * GPB + grp; v < p.V; v += (int)gridDim.x * GPB) {
        uint64_t t = p.tau[v];
        double x[NSL][4];
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            const int s = lig + j * LPV;
            int4 c = make_int4(0, 0, 0, 0);
            if (s < S) c = reinterpret_cast<const int4 *>(p.cnt_vs)[(size_t)v * S + s];
            x[j][0] = (double)c.x; x[j][1] = (double)c.y; x[j][2] = (double)c.z; x[j][3] = (double)c.w;
        }
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
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const bool here = a == k;
                        L[4 * k] = here ? R[0] : L[4 * k]; L[4 * k + 1] = here ? R[1] : L[4 * k + 1];
                        L[4 * k + 2] = here ? R[2] : L[4 * k + 2]; L[4 * k + 3] = here ? R[3] : L[4 * k + 3];
                    }
                }
                if (mx == NINF) continue;                               // group-uniform: the pair stays, its uniform is spent unseen
                const unsigned long long jj = jbase + (unsigned long long)(g * G + h);
                uint32_t w[4];
                philox4x32_10((uint32_t)jj, (uint32_t)(jj >> 32), p.iter, DSM_STREAM_TPAR, p.k0, p.k1, w);
                const double u = (double)w[0] * 2.3283064365386963e-10;
                double sum = 0.0;
#pragma unroll
                for (int k = 0; k < 16; ++k) { L[k] = L[k] == NINF ? 0.0 : exp(L[k] - mx); sum += L[k]; }     // e_k, added in ascending k
                double cdf = 0.0;
                int kn = 15;                                            // the last edge is forced
                bool found = false;
#pragma unroll
                for (int k = 0; k < 15; ++k) {
                    cdf += L[k] / sum;
                    if (!found && u < cdf) { kn = k; found = true; }
                }
                const int ng = kn >> 2, nh = kn & 3;
                const int og = (int)(t >> (2 * g)) & 3, oh = (int)(t >> (2 * h)) & 3;
                nchg += (lig == 0) ? (int)(ng != og) + (int)(nh != oh) : 0;
                t = (t & ~((3ull << (2 * g)) | (3ull << (2 * h)))) | ((uint64_t)ng << (2 * g)) | ((uint64_t)nh << (2 * h));
            }
        if (lig == 0) p.tau[v] = t;
    }
    const int wn = (int)group_allreduce_sum_u32<64>((unsigned)nchg);
    if ((tid & 63) == 0) redi[tid >> 6] = wn;
    __syncthreads();
    if (tid == 0) {
        const int tot = redi[0] + redi[1] + redi[2] + redi[3];
        if (tot) atomicAdd(p.nchange, tot);
    }
}

static size_t pair_lds_bytes(int G, int LPV, int NSL) { return ((size_t)G * LPV * NSL + 16 + 2 * DSM_LOG_TAB_N) * sizeof(double); }

template <int LPV, int NSL>
static int launch_pair(dsm_ctx *c, const PairParams &p, int grid, size_t sh)
{
    static bool attr_set = false;                  // more than 64 KB of dynamic LDS has to be asked for, once per instantiation
    if (sh > 64 * 1024 && !attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&pair_sweep_kernel<LPV, NSL>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    hipLaunchKernelGGL((pair_sweep_kernel<LPV, NSL>), dim3(grid), dim3(256), sh, c->stream, p);
    return DSM_OK;
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
    int LPV, NSL;
    { const int rc = tau_shape(S, &LPV, &NSL); if (rc != DSM_OK) return rc; }
    const int gpb = 256 / LPV;
    const int grid = std::max(1, std::min((V + gpb - 1) / gpb, DSM_MAX_GRID));
    PairParams p;
    p.cnt_vs = c->cnt_vs; p.tau = c->tau; p.gamma = gamma; p.eta = eta;
    p.log_tab = c->log_tab; p.nchange = c->nchange;
    p.V = V; p.S = S; p.G = G;
    p.k0 = (uint32_t)c->ctr_seed; p.k1 = (uint32_t)(c->ctr_seed >> 32); p.iter = iter;
    const size_t sh = pair_lds_bytes(G, LPV, NSL);
    if (sh > 160 * 1024) { dsm_set_error("pair pass: gamma tile (%zu B) exceeds LDS", sh); return DSM_ERR_UNSUPPORTED; }
    int rc = DSM_ERR_UNSUPPORTED;
    // every (LPV, NSL) tau_shape returns
#define PAIR_CASE(L, N) if (LPV == L && NSL == N) rc = launch_pair<L, N>(c, p, grid, sh)
    PAIR_CASE(16, 1); PAIR_CASE(16, 2); PAIR_CASE(16, 3); PAIR_CASE(32, 2); PAIR_CASE(32, 3);
    PAIR_CASE(64, 2); PAIR_CASE(64, 3); PAIR_CASE(64, 4); PAIR_CASE(64, 6); PAIR_CASE(64, 8);
#undef PAIR_CASE
    if (rc != DSM_OK) { if (rc == DSM_ERR_UNSUPPORTED) dsm_set_error("pair pass: no kernel for %d lanes x %d samples", LPV, NSL); return rc; }
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}
