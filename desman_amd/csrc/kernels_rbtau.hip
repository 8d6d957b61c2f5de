// kernels_rbtau.hip -- the Rao-Blackwellised tau posterior of the positions of the fit from the resident traces (api_trace.hip:
// dsm_ctx_trace_rb_marginals; desman_amd/marginals.py).
//
//   rb_tau_kernel<LPV, NSL>   for every stored iteration t, position v and haplotype g the full conditional of tau_vg given the rest of
//                             (tau_t, gamma_t, eta_t), added to the cell of the label perm[t][g]; no draw, nothing of the chain written
//
// The arithmetic (tests/_tau_rb_ref.py restates it in numpy):
//     rest[s][b] = fma chain from 0 over h != g, h ascending, of eta_t[tau_t[v][h]][b] * gamma_t[s][h]
//     L_a        = sum_{s,b: x > 0} x[v][s][b] ln(rest[s][b] + eta_t[a][b] gamma_t[s][g]),  x exact in fp64; p = 0 under a count: -inf
//     q_a        = exp(L_a - max) / (((e_0 + e_1) + e_2) + e_3);  all four -inf: the one-hot of tau_t[v][g], counted in `dead`
// No random number is drawn anywhere.
#include "dsm_sweep_tile.h"
#include "dsm_trace_host.h"

struct RbParams : SweepTileParams {       // gamma / eta: the rows of the first used iteration; tau and nchange are not used
    const uint64_t *trace;                // the packed tau of the first used iteration
    size_t trace_stride;                  // words between two iterations' rows (0: one row for all, the fixed-tau chain)
    const uint8_t *perm;                  // [n_it][G] the label of haplotype g in iteration t
    double *bs, *sum, *bsq;               // [V][G][4] the running batch's sum; sum of the batch sums; sum of their squares
    unsigned long long *dead;             // cell-iterations whose four totals were all -inf
    int n_it, L;                          // used iterations (a multiple of L), batch length
};

// the four lane-partial totals of a step: dsm_pair_candidates_row's rule for a cell -- a count of 0 adds 0 whatever the mixture value
// (a padded slot holds abundance 0 under count 0), 0 under a positive count is -inf through libm's log
template <int NSL>
__device__ __forceinline__ void rb_candidates(const int4 (&c)[NSL], const double (&st)[NSL][4], const double (&gg)[NSL],
                                              const double *__restrict__ eS, const double2 *__restrict__ ltab, double (&L)[4])
{
    L[0] = 0.0; L[1] = 0.0; L[2] = 0.0; L[3] = 0.0;
#pragma unroll
    for (int j = 0; j < NSL; ++j) {
        const int xi[4] = {c[j].x, c[j].y, c[j].z, c[j].w};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            // (the empty asm keeps the conversion HERE: hoisted out of the haplotype loop, the counts would live as doubles across it)
            int xb = xi[b];
            asm volatile("" : "+v"(xb));
            const bool seen = xb > 0;
            const double x = (double)xb;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const double pr = st[j][b] + eS[a * 4 + b] * gg[j];
                double lg = 0.0;
                if (__builtin_expect(dsm_log_ok(pr), 1)) lg = dsm_log_core(pr, ltab);
                else if (seen) lg = dsm_log_slow(pr);
                L[a] += seen ? x * lg : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);                      // one cell's four logarithms at a time
        }
    }
}

// The frame of dsm_sweep_tile.h around a loop over the stored iterations: the tables of iteration t are staged behind a barrier (every
// group is done with those of t - 1), then every group walks its positions as the sweeps do.  The links h < g of the rest mixture are
// carried from step to step with the CURRENT bases, as held_sweep_kernel carries the re-drawn ones: the same operations in the same
// order as the chain from zero.  Lane 0 of a group owns the accumulators of its position: plain read-modify-write of global memory in
// t order, loaded at the start of the step and stored at its end -- per cell (v, label) the batch sum is the t-ascending sum from 0 over
// the batch's iterations, and at the batch's last iteration (every label occurs once in a perm row) it is added to `sum` and its square
// to `bsq`, batches ascending.  Nothing depends on the grid.
template <int LPV, int NSL>
__global__ __launch_bounds__(256) void rb_tau_kernel(RbParams p)
{
    constexpr int SP = LPV * NSL;
    constexpr int GPB = 256 / LPV;
    const int tid = threadIdx.x, G = p.G;
    const int grp = tid / LPV, lig = tid % LPV;
    const bool owner = lig == 0;
    const double NINF = -INFINITY;
    const size_t sg = (size_t)p.S * G;
    unsigned long long ndead = 0;
    int inb = 0;                                                    // iterations of the running batch already added
    for (int t = 0; t < p.n_it; ++t) {
        if (t) __syncthreads();
        SweepTileParams pt = p;
        pt.gamma = p.gamma + (size_t)t * sg;
        pt.eta = p.eta + (size_t)t * 16;
        const SweepTileLds lds = sweep_tile_stage<LPV, NSL>(pt, 0.0);
        const double *gT = lds.gT, *eS = lds.eS;
        const double2 *ltab = lds.ltab;
        const bool first = inb == 0, last = inb == p.L - 1;
        const uint8_t *pr = p.perm + (size_t)t * G;
        const uint64_t *tw = p.trace + (size_t)t * p.trace_stride;
        for (int v = (int)blockIdx.x * GPB + grp; v < p.V; v += (int)gridDim.x * GPB) {
            const uint64_t tv = tw[v];
            int4 c[NSL];
            sweep_tile_counts<LPV, NSL>(p, v, lig, c);
            double pre[NSL][4];
#pragma unroll
            for (int j = 0; j < NSL; ++j)
#pragma unroll
                for (int b = 0; b < 4; ++b) pre[j][b] = 0.0;
            for (int g = 0; g < G; ++g) {
                const size_t cell = ((size_t)v * G + pr[g]) * 4;
                double2 a01 = make_double2(0.0, 0.0), a23 = make_double2(0.0, 0.0);
                if (owner && !first) {
                    a01 = *reinterpret_cast<const double2 *>(p.bs + cell);
                    a23 = *reinterpret_cast<const double2 *>(p.bs + cell + 2);
                }
                double gg[NSL], st[NSL][4];
#pragma unroll
                for (int j = 0; j < NSL; ++j) {
                    gg[j] = gT[g * SP + lig + j * LPV];
#pragma unroll
                    for (int b = 0; b < 4; ++b) st[j][b] = pre[j][b];
                }
#pragma unroll 2
                for (int h = g + 1; h < G; ++h) {
                    const double *er = eS + (int)((tv >> (2 * h)) & 3) * 4;
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
                rb_candidates<NSL>(c, st, gg, eS, ltab, l);
                group_allreduce_sum4<LPV>(l[0], l[1], l[2], l[3]);
                const int cur = (int)((tv >> (2 * g)) & 3);
                double mx = l[0];
#pragma unroll
                for (int a = 1; a < 4; ++a) mx = l[a] > mx ? l[a] : mx;
                double q[4];
                if (mx == NINF) {                                   // group-uniform: the cell has no live base
#pragma unroll
                    for (int a = 0; a < 4; ++a) q[a] = a == cur ? 1.0 : 0.0;
                    ndead += owner ? 1u : 0u;
                } else {
                    double e[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) e[a] = l[a] == NINF ? 0.0 : exp(l[a] - mx);
                    const double tot = ((e[0] + e[1]) + e[2]) + e[3];
#pragma unroll
                    for (int a = 0; a < 4; ++a) q[a] = e[a] / tot;
                }
                const double *er = eS + cur * 4;                    // link g of the chain, with the current base
                const double e0 = er[0], e1 = er[1], e2 = er[2], e3 = er[3];
#pragma unroll
                for (int j = 0; j < NSL; ++j) {
                    pre[j][0] = fma(e0, gg[j], pre[j][0]);
                    pre[j][1] = fma(e1, gg[j], pre[j][1]);
                    pre[j][2] = fma(e2, gg[j], pre[j][2]);
                    pre[j][3] = fma(e3, gg[j], pre[j][3]);
                }
                if (owner) {
                    a01.x += q[0]; a01.y += q[1]; a23.x += q[2]; a23.y += q[3];
                    if (last) {
                        double2 s01 = *reinterpret_cast<const double2 *>(p.sum + cell), s23 = *reinterpret_cast<const double2 *>(p.sum + cell + 2);
                        double2 b01 = *reinterpret_cast<const double2 *>(p.bsq + cell), b23 = *reinterpret_cast<const double2 *>(p.bsq + cell + 2);
                        s01.x += a01.x; s01.y += a01.y; s23.x += a23.x; s23.y += a23.y;
                        b01.x += a01.x * a01.x; b01.y += a01.y * a01.y; b23.x += a23.x * a23.x; b23.y += a23.y * a23.y;
                        *reinterpret_cast<double2 *>(p.sum + cell) = s01; *reinterpret_cast<double2 *>(p.sum + cell + 2) = s23;
                        *reinterpret_cast<double2 *>(p.bsq + cell) = b01; *reinterpret_cast<double2 *>(p.bsq + cell + 2) = b23;
                    } else {
                        *reinterpret_cast<double2 *>(p.bs + cell) = a01;
                        *reinterpret_cast<double2 *>(p.bs + cell + 2) = a23;
                    }
                }
            }
        }
        inb = last ? 0 : inb + 1;
    }
    if (ndead) atomicAdd(p.dead, ndead);                            // an integer count: its order does not matter
}

// test hook: the (LPV, NSL) of the instantiation k_rb_tau launches for S samples (the sweep's own tiling: tau_shape)
extern "C" int dsm_rbtau_debug_path(int S, int G, int out[2])
{
    if (!out) { dsm_set_error("rbtau_debug_path: null pointer"); return DSM_ERR_ARG; }
    if (S < 1 || G < 1) { dsm_set_error("rbtau_debug_path: S=%d, G=%d", S, G); return DSM_ERR_ARG; }
    if (G > DSM_MAX_G) { dsm_set_error("rbtau_debug_path: G=%d exceeds DSM_MAX_G=%d", G, DSM_MAX_G); return DSM_ERR_UNSUPPORTED; }
    int LPV, NSL;
    { const int rc = tau_shape(S, &LPV, &NSL); if (rc != DSM_OK) return rc; }
    out[0] = LPV; out[1] = NSL;
    return DSM_OK;
}

// The conditionals of n_it >= 1 stored iterations in batches of L (n_it a multiple of L), one launch: tr = the rows of
// the first of them, d_perm [n_it][G]; d_sum, d_bsq and *d_dead zeroed by the caller, d_bs scratch of the same size as d_sum.
int k_rb_tau(dsm_ctx *c, const TraceView &tr, const uint8_t *d_perm, int n_it, int L, double *d_bs, double *d_sum, double *d_bsq,
             unsigned long long *d_dead)
{
    RbParams p;
    p.cnt_vs = c->cnt_vs; p.tau = nullptr; p.gamma = tr.gamma; p.eta = tr.eta;
    p.log_tab = c->log_tab; p.nchange = nullptr;
    p.V = c->V; p.S = c->S; p.G = c->G;
    p.k0 = 0; p.k1 = 0; p.iter = 0;
    p.trace = tr.tau; p.trace_stride = tr.tau_stride; p.perm = d_perm;
    p.bs = d_bs; p.sum = d_sum; p.bsq = d_bsq; p.dead = d_dead;
    p.n_it = n_it; p.L = L;
    return sweep_tile_dispatch(p, "rb marginals: ", "rb marginals", [&](auto LL, auto N, int grid, size_t sh) {
        return sweep_tile_launch<rb_tau_kernel<LL.value, N.value>>(c, p, grid, sh);
    });
}
