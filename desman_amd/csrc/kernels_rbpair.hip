// kernels_rbpair.hip -- the Rao-Blackwellised JOINT posterior of two haplotypes' bases from the resident traces (api_trace.hip:
// dsm_ctx_trace_rb_pairs; desman_amd/marginals.py).
//
//   rb_pair_kernel<LPV, NSL>   for every used stored iteration t, position v and pair g < h (lexicographic, the order of the pair pass)
//                              the sixteen-state full conditional of (tau_vg, tau_vh) given the rest of (tau_t, gamma_t, eta_t), added
//                              to the cells of the relabelled pair; no draw, tau is never modified, nothing of the chain written
//   rb_pair_fold_kernel        the per-position batch sums of P(same base) -> same_batch, positions ascending
//
// The arithmetic is that of pair_sweep_kernel (the header comment of kernels_pairtau.hip; tests/_tau_rb_pairs_ref.py restates it):
//     m_a[s]    = sum_{k != g, h; tau_t[v][k] = a} gamma_t[s][k]                  (k in order)
//     rest[s][b]= ((m_0 eta[0][b] + m_1 eta[1][b]) + m_2 eta[2][b]) + m_3 eta[3][b]
//     L_k       = sum_{s,b: x > 0} x[s][b] ln((rest[s][b] + eta[a][b] gamma[s][g]) + eta[a'][b] gamma[s][h]),  k = 4 a + a'
//     q_k       = exp(L_k - max) / (e_0 + e_1 + ... + e_15, in this order);  all sixteen -inf: the one-hot of the current pair, counted
//                 in `dead`
//     same      = ((q_0 + q_5) + q_10) + q_15
#include "dsm_sweep_tile.h"
#include "dsm_trace_host.h"

struct RbPairParams : SweepTileParams {   // gamma / eta: the rows of the first used iteration; tau, nchange and the Philox key are not used
    const uint64_t *trace;                // the packed tau of the first used iteration
    size_t trace_step;                    // words between two USED iterations' rows (0: one row for all, the fixed-tau chain)
    size_t par_step;                      // rows of the gamma / eta traces between two used iterations (the stride)
    const uint16_t *slot;                 // [n_it][P] (relabelled pair index << 1) | (1: the labels are in descending order, q is transposed)
    double *joint;                        // [nv][P][16] the chunk's running sums, or null
    double *same;                         // [B][nv][P] per batch and position the running sum of `same`, or null
    unsigned long long *dead;             // (position, pair, iteration)s whose sixteen totals were all -inf
    int v0, nv;                           // the chunk: positions v0 .. v0 + nv - 1
    int n_it, L, P;                       // used iterations (a multiple of L), batch length, pairs
};

// The frame of dsm_sweep_tile.h around a loop over the used iterations, as rb_tau_kernel has it: the tables of iteration t are staged
// behind a barrier, then every group walks its positions of the chunk and their pairs as pair_sweep_kernel does, from the unchanged
// word of tau_t.  After the butterfly every lane of the group holds the same sixteen totals and forms the same sixteen q.  Lane k < 16
// owns accumulator k of the group's position: it takes q_k -- q_{4 a' + a} where the relabelling puts the pair in descending order --
// and adds it to joint[v][slot][k] by a plain read-modify-write of global memory (the sixteen lanes touch one 128-byte line), iteration
// 0 storing without the read.  A cell is owned by the same thread in every iteration (the position's group does not change within a
// launch, a row of `slot` is a bijection of the pairs), so its sum is the t-ascending one whatever the grid.  Lane 0 does the same for
// same[batch][v][slot], the first iteration of a batch storing without the read.
template <int LPV, int NSL>
__global__ __launch_bounds__(256) void rb_pair_kernel(RbPairParams p)
{
    static_assert(LPV >= 16, "lane k < 16 of a group owns accumulator k");
    constexpr int SP = LPV * NSL;
    constexpr int GPB = 256 / LPV;
    const int tid = threadIdx.x, G = p.G, P = p.P;
    const int grp = tid / LPV, lig = tid % LPV;
    const double NINF = -INFINITY;
    const size_t sg = (size_t)p.S * G;
    const int tk = ((lig & 3) << 2) | ((lig >> 2) & 3);             // the transposed index of accumulator lig (lig < 16)
    unsigned long long ndead = 0;
    int inb = 0, batch = 0;                                         // iterations of the running batch already added; its number
    for (int t = 0; t < p.n_it; ++t) {
        if (t) __syncthreads();
        SweepTileParams pt = p;
        pt.gamma = p.gamma + (size_t)t * p.par_step * sg;
        pt.eta = p.eta + (size_t)t * p.par_step * 16;
        const SweepTileLds lds = sweep_tile_stage<LPV, NSL>(pt, 0.0);
        const double *gT = lds.gT, *eS = lds.eS;
        const double2 *ltab = lds.ltab;
        const uint64_t *tw = p.trace + (size_t)t * p.trace_step;
        const uint16_t *sl = p.slot + (size_t)t * P;
        for (int i = (int)blockIdx.x * GPB + grp; i < p.nv; i += (int)gridDim.x * GPB) {
            const int v = p.v0 + i;
            const uint64_t tv = tw[v];
            int4 c[NSL];
            sweep_tile_counts<LPV, NSL>(p, v, lig, c);
            double x[NSL][4];
#pragma unroll
            for (int j = 0; j < NSL; ++j) { x[j][0] = (double)c[j].x; x[j][1] = (double)c[j].y; x[j][2] = (double)c[j].z; x[j][3] = (double)c[j].w; }
            double *jrow = p.joint ? p.joint + (size_t)i * P * 16 : nullptr;
            double *srow = p.same ? p.same + ((size_t)batch * p.nv + i) * P : nullptr;
            int pi = 0;
            for (int g = 0; g < G; ++g)
                for (int h = g + 1; h < G; ++h, ++pi) {
                    double m0[NSL], m1[NSL], m2[NSL], m3[NSL], gg[NSL], gh[NSL];
#pragma unroll
                    for (int j = 0; j < NSL; ++j) { m0[j] = 0.0; m1[j] = 0.0; m2[j] = 0.0; m3[j] = 0.0; gg[j] = 0.0; gh[j] = 0.0; }
                    for (int k = 0; k < G; ++k) {
                        const bool isg = k == g, ish = k == h;
                        const int d = (isg || ish) ? 4 : (int)(tv >> (2 * k)) & 3;
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
                    double Lk[16], mx = NINF;
#pragma unroll
                    for (int k = 0; k < 16; ++k) Lk[k] = 0.0;
#pragma unroll 1
                    for (int a = 0; a < 4; ++a) {                       // four candidates at a time, as the pair pass
                        double R[4];
                        dsm_pair_candidates_row<NSL>(x, m0, m1, m2, m3, gg, gh, eS, ltab, a, R);
                        group_allreduce_sum4<LPV>(R[0], R[1], R[2], R[3]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) mx = R[r] > mx ? R[r] : mx;
                        dsm_put_row(Lk, a, R);
                    }
                    double q[16];
                    if (mx == NINF) {                                   // group-uniform: no live state, the current pair stands
                        const int cur = (((int)(tv >> (2 * g)) & 3) << 2) | ((int)(tv >> (2 * h)) & 3);
#pragma unroll
                        for (int k = 0; k < 16; ++k) q[k] = k == cur ? 1.0 : 0.0;
                        ndead += lig == 0 ? 1u : 0u;
                    } else {
                        double tot = 0.0;
#pragma unroll
                        for (int k = 0; k < 16; ++k) { q[k] = Lk[k] == NINF ? 0.0 : exp(Lk[k] - mx); tot += q[k]; }
#pragma unroll
                        for (int k = 0; k < 16; ++k) q[k] = q[k] / tot;
                    }
                    const unsigned ps = sl[pi];
                    const int slot = (int)(ps >> 1);
                    if (jrow && lig < 16) {
                        const int src = (ps & 1u) ? tk : lig;
                        double mine = q[0];
#pragma unroll
                        for (int k = 1; k < 16; ++k) mine = src == k ? q[k] : mine;
                        double *cell = jrow + (size_t)slot * 16 + lig;
                        *cell = t ? *cell + mine : mine;
                    }
                    if (srow && lig == 0) {
                        const double s = ((q[0] + q[5]) + q[10]) + q[15];
                        double *cell = srow + slot;
                        *cell = inb ? *cell + s : s;
                    }
                }
        }
        if (inb == p.L - 1) { inb = 0; ++batch; } else ++inb;
    }
    if (ndead) atomicAdd(p.dead, ndead);                            // an integer count: its order does not matter
}

// same_batch[b][p] += the chunk's same[b][i][p], i ascending: one thread per (b, p).  The chunks come in position order, so every cell is
// the sum over ALL positions in ascending order from 0, however the positions were cut into chunks and whatever grid walked them.
__global__ __launch_bounds__(256) void rb_pair_fold_kernel(const double *__restrict__ same, double *__restrict__ out, int B, int nv, int P)
{
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (idx >= B * P) return;
    const int b = idx / P, pp = idx % P;
    const double *src = same + (size_t)b * nv * P + pp;
    double acc = out[idx];
    for (int i = 0; i < nv; ++i) acc += src[(size_t)i * P];
    out[idx] = acc;
}

static int g_rbpair_chunk = 0;       // dsm_rbpair_debug_set_chunk: positions per launch (0 = by the scratch bound)

extern "C" int dsm_rbpair_debug_set_chunk(int positions) { return dsm_set_knob(&g_rbpair_chunk, positions, "rbpair", "chunk"); }

// test hook: the (LPV, NSL) of the instantiation k_rb_pairs launches for S samples (the sweep's own tiling: tau_shape)
extern "C" int dsm_rbpair_debug_path(int S, int G, int out[2])
{
    if (!out) { dsm_set_error("rbpair_debug_path: null pointer"); return DSM_ERR_ARG; }
    if (S < 1 || G < 1) { dsm_set_error("rbpair_debug_path: S=%d, G=%d", S, G); return DSM_ERR_ARG; }
    if (G > DSM_MAX_G) { dsm_set_error("rbpair_debug_path: G=%d exceeds DSM_MAX_G=%d", G, DSM_MAX_G); return DSM_ERR_UNSUPPORTED; }
    int LPV, NSL;
    { const int rc = tau_shape(S, &LPV, &NSL); if (rc != DSM_OK) return rc; }
    out[0] = LPV; out[1] = NSL;
    return DSM_OK;
}

// positions per launch: the two scratch buffers together, nv P (16 [joint wanted] + B [same wanted]) doubles, stay within
// DSM_RBPAIR_SCRATCH_BYTES -- but a launch has at least one position
int rb_pairs_chunk(int V, int G, int B, bool want_joint, bool want_same)
{
    if (g_rbpair_chunk > 0) return std::min(g_rbpair_chunk, V);
    const size_t P = (size_t)G * (G - 1) / 2;
    const size_t per = P * sizeof(double) * ((want_joint ? 16 : 0) + (want_same ? (size_t)B : 0));
    if (per == 0) return V;
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)V, (size_t)DSM_RBPAIR_SCRATCH_BYTES / per));
}

// The pair conditionals of the chunk v0 .. v0 + nv - 1 over n_it >= 1 used iterations in batches of L (n_it a multiple of L), one launch
// and, with d_same, the fold: tr = the rows of the first used iteration, `stride` trace iterations between two used ones; d_slot
// [n_it][P]; d_joint [nv][P][16] and d_same [B][nv][P] scratch (either may be null), d_same_batch [B][P] zeroed by the caller before the
// first chunk, *d_dead zeroed by the caller.
int k_rb_pairs(dsm_ctx *c, const TraceView &tr, int stride, const uint16_t *d_slot, int n_it, int L, int v0, int nv, double *d_joint,
               double *d_same, double *d_same_batch, unsigned long long *d_dead)
{
    RbPairParams p;
    p.cnt_vs = c->cnt_vs; p.tau = nullptr; p.gamma = tr.gamma; p.eta = tr.eta;
    p.log_tab = c->log_tab; p.nchange = nullptr;
    p.V = nv; p.S = c->S; p.G = c->G;                               // (V sizes the grid: the chunk's positions)
    p.k0 = 0; p.k1 = 0; p.iter = 0;
    p.trace = tr.tau; p.trace_step = tr.tau_stride * (size_t)stride; p.par_step = (size_t)stride; p.slot = d_slot;
    p.joint = d_joint; p.same = d_same; p.dead = d_dead;
    p.v0 = v0; p.nv = nv; p.n_it = n_it; p.L = L; p.P = c->G * (c->G - 1) / 2;
    DSM_TRY(sweep_tile_dispatch(p, "rb pairs: ", "rb pairs", [&](auto LL, auto N, int grid, size_t sh) {
        return sweep_tile_launch<rb_pair_kernel<LL.value, N.value>>(c, p, grid, sh);
    }));
    if (d_same) {
        const int B = n_it / L, cells = B * p.P;
        hipLaunchKernelGGL(rb_pair_fold_kernel, dim3((cells + 255) / 256), dim3(256), 0, c->stream, d_same, d_same_batch, B, nv, p.P);
        HIP_TRY(hipGetLastError());
    }
    return DSM_OK;
}
