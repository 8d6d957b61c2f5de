// kernels_fit.hip -- gfx950 kernels for the posterior predictive fit of a chain per sample and per position, from the traces that stay
// resident after an update call (api_trace.hip: dsm_ctx_trace_fit_stats; desman_amd/check.py).
//
//   trace_fit_kernel<NSL>   per stored iteration t and cell (v, s) with counts n_b, N = sum_b n_b > 0, and the likelihood's own
//                           p_b = sum_g gamma_t[s][g] eta_t[tau_t[v][g]][b], k = #{b : p_b > 0}:
//                               X = sum_{b: p_b > 0} (n_b - N p_b)^2 / (N p_b)          (+inf where p_b = 0 < n_b)
//                               D = 2 sum_{b: n_b > 0} n_b ln(n_b / (N p_b))            (+inf there too)
//                               E = k - 1     W = 2 (k - 1) + (sum_{b: p_b > 0} 1 / p_b - (k^2 + 2 k - 2)) / N
//                           summed over a part of the iteration range in registers, then once over samples (per position) and over the
//                           positions of the workgroup (per sample)
//   fit_merge_*_kernel      the partial rows of the parts and workgroups, added in a fixed order
//
// Plain fp64, no floating-point atomics: for a given number of parts two launches give the same bits.  Every exclusion is a select,
// never a product with 0, so no operand can make a NaN and an infinite cell stays in its own sample's and position's sums.
#include <algorithm>
#include <math.h>

#include "dsm_trace_host.h"
#include "dsm_fit_cell.h"

#define FIT_BLOCKS 2048         // workgroups a launch aims at (256 compute units x 8)
#define FIT_LDS_GAMMA 4096      // doubles of LDS a chunk of gamma columns may take (32 KiB): the chunk is min(G, FIT_LDS_GAMMA / sample slots)

struct FitParams {
    const int32_t *cnt;         // [V][S][4]
    const uint64_t *trace;      // row of the first iteration
    size_t trace_stride;        // words between two iterations' rows (0: one row for all)
    const double *gamma, *eta;  // [n][S][G], [n][16] of the same iterations
    int n, V, S, G;
    int lpv_log2, gc;           // log2 of the lanes per position; haplotypes per staged chunk of gamma
    double *samp_part;          // [parts][tiles][S][4]
    double *pos_part;           // [parts][V][4]
    double *cell_part;          // [parts][V][S] or null
};

// The sweep's lane-group tiling (kernels_gibbs.hip: tau_shape), simplified: a group of LPV = 2^lpv_log2 lanes per position, NSL sample
// slots per lane (slot j of lane l = sample l + j LPV), 256 / LPV positions per workgroup, one workgroup per tile of positions and part
// of the iteration range (blockIdx.z; part z owns iterations z pi .. min(n, (z + 1) pi) - 1, pi = ceil(n / parts); an empty part writes
// zeros).  A thread keeps the four counts of its NSL cells and their running X, D, W (fp64) and E (an integer) in registers for the whole
// iteration loop.  Per iteration the position's trace word is one load (the lanes of a group ask for the same address), gamma_t is
// staged in LDS transposed -- [g][slot], so that the lanes of a group read consecutive doubles and the groups of a wavefront the same
// ones -- in chunks of gc haplotypes (one chunk unless S G > FIT_LDS_GAMMA), eta_t next to it.  The mixture over the four true bases
// m_a = sum_g gamma[s][g] [digit_g = a] is four named sums fed by compares against constants; then p_b = sum_a m_a eta[a][b].  The
// order of every sum is fixed and is that of check.cell_terms, so a cell's terms differ from the restatement's by the logarithm only.
// Lanes past S and positions past V hold zero counts: N = 0, nothing is added.
template <int NSL>
__global__ __launch_bounds__(256) void trace_fit_kernel(const FitParams p)
{
    extern __shared__ double lds[];
    const int LPV = 1 << p.lpv_log2, SP = LPV * NSL, PPB = 256 >> p.lpv_log2;
    const int tid = threadIdx.x, l = tid & (LPV - 1), grp = tid >> p.lpv_log2;
    const int V = p.V, S = p.S, G = p.G, gc = p.gc;
    const long long v = (long long)blockIdx.x * PPB + grp;
    const bool vin = v < V;
    double *const lgam = lds, *const leta = lds + (size_t)gc * SP;

    int c0[NSL], c1[NSL], c2[NSL], c3[NSL], aE[NSL];
    double aX[NSL], aD[NSL], aW[NSL];
#pragma unroll
    for (int j = 0; j < NSL; ++j) {
        const int s = l + j * LPV;
        int4 c = make_int4(0, 0, 0, 0);
        if (vin && s < S) c = *reinterpret_cast<const int4 *>(p.cnt + ((size_t)v * S + s) * 4);
        c0[j] = c.x; c1[j] = c.y; c2[j] = c.z; c3[j] = c.w;
        aX[j] = 0.0; aD[j] = 0.0; aW[j] = 0.0; aE[j] = 0;
    }

    const int parts = (int)gridDim.z, pi = (p.n + parts - 1) / parts;
    const int t0 = min(p.n, (int)blockIdx.z * pi), t1 = min(p.n, t0 + pi);
    const size_t sg = (size_t)S * G;
    for (int t = t0; t < t1; ++t) {
        const uint64_t word = vin ? p.trace[(size_t)t * p.trace_stride + (size_t)v] : 0ull;
        const double *gam_t = p.gamma + (size_t)t * sg;
        double m0[NSL], m1[NSL], m2[NSL], m3[NSL];
        fit_cell_mixture<NSL>(gam_t, p.eta + (size_t)t * 16, word, S, G, gc, p.lpv_log2, lgam, leta, m0, m1, m2, m3);      // (dsm_fit_cell.h)
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            const int Ni = c0[j] + c1[j] + c2[j] + c3[j];
            const double N = (double)Ni;
            double x = 0.0, dv = 0.0, rs = 0.0;
            int k = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double pb = fit_cell_p(m0[j], m1[j], m2[j], m3[j], leta, b);
                const int ni = b == 0 ? c0[j] : (b == 1 ? c1[j] : (b == 2 ? c2[j] : c3[j]));     // (b is a constant after unrolling)
                const double nb = (double)ni;
                const bool pos = pb > 0.0, seen = ni > 0;
                const double e = N * pb, dl = nb - e;
                x += pos ? dl * dl / e : (seen ? INFINITY : 0.0);
                dv += seen ? (pos ? nb * log(nb / e) : INFINITY) : 0.0;
                rs += pos ? 1.0 / pb : 0.0;
                k += pos ? 1 : 0;
            }
            const bool live = Ni > 0;
            const double w = 2.0 * (double)(k - 1) + (rs - (double)(k * k + 2 * k - 2)) / N;
            aX[j] += live ? x : 0.0;
            aD[j] += live ? 2.0 * dv : 0.0;
            aW[j] += live ? w : 0.0;
            aE[j] += live ? k - 1 : 0;
        }
    }

    // ---- per cell: the sum of X over the part
    if (p.cell_part && vin) {
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            const int s = l + j * LPV;
            if (s < S) p.cell_part[((size_t)blockIdx.z * V + (size_t)v) * S + s] = aX[j];
        }
    }
    // ---- per position: over the slots of the lane in order, then over the lanes of the group by halving (xor offsets below LPV stay
    // inside the group)
    {
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
#pragma unroll
        for (int j = 0; j < NSL; ++j) { q0 += aX[j]; q1 += aD[j]; q2 += (double)aE[j]; q3 += aW[j]; }
        for (int off = LPV >> 1; off > 0; off >>= 1) {
            q0 += __shfl_xor(q0, off); q1 += __shfl_xor(q1, off); q2 += __shfl_xor(q2, off); q3 += __shfl_xor(q3, off);
        }
        if (vin && l == 0) {
            double *o = p.pos_part + ((size_t)blockIdx.z * V + (size_t)v) * 4;
            o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3;
        }
    }
    // ---- per sample: over the position groups of the workgroup in order, one statistic at a time through LDS ([group][slot])
    double *const out = p.samp_part + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * (size_t)S * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NSL; ++j)
            lds[grp * SP + l + j * LPV] = q == 0 ? aX[j] : (q == 1 ? aD[j] : (q == 2 ? (double)aE[j] : aW[j]));
        __syncthreads();
        for (int s = tid; s < S; s += 256) {
            double a = 0.0;
            for (int r = 0; r < PPB; ++r) a += lds[r * SP + s];
            out[(size_t)s * 4 + q] = a;
        }
    }
}

// sample[s][q] = the sum of rows partial rows [rows][S][4]: one workgroup per sample; thread i adds rows i, i + 256, ... in order, then
// the 256 sums meet by halving in LDS -- a fixed order for a given number of rows
__global__ __launch_bounds__(256) void fit_merge_sample_kernel(const double *__restrict__ part, size_t rows, int S, double *__restrict__ sample)
{
    __shared__ double red[4][256];
    const int s = blockIdx.x, tid = threadIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (size_t r = tid; r < rows; r += 256) {
        const double *q = part + (r * S + s) * 4;
        a0 += q[0]; a1 += q[1]; a2 += q[2]; a3 += q[3];
    }
    red[0][tid] = a0; red[1][tid] = a1; red[2][tid] = a2; red[3][tid] = a3;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] += red[0][tid + off]; red[1][tid] += red[1][tid + off];
            red[2][tid] += red[2][tid + off]; red[3][tid] += red[3][tid + off];
        }
        __syncthreads();
    }
    if (tid < 4) sample[(size_t)s * 4 + tid] = red[tid][0];
}

// out[i] = sum over the parts z, in order, of part[z][i]
__global__ __launch_bounds__(256) void fit_merge_parts_kernel(const double *__restrict__ part, size_t len, int parts, double *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    double a = 0.0;
    for (int z = 0; z < parts; ++z) a += part[(size_t)z * len + i];
    out[i] = a;
}

static int g_fit_parts = 0;       // dsm_fit_debug_set_parts: iteration parts per launch (0 = by the grid the launch aims at)

extern "C" int dsm_fit_debug_set_parts(int parts)
{
    return dsm_set_knob(&g_fit_parts, parts, "fit", "parts");
}

// the tile, the gamma chunk and the grid of a launch over n_it iterations of this context's table; nothing is launched
int fit_plan(const dsm_ctx *c, int n_it, FitPlan *pl)
{
    const int S = c->S, G = c->G, V = c->V;
    if (S < 1 || S > DSM_MAX_S) { dsm_set_error("fit: S=%d outside 1..DSM_MAX_S=%d", S, DSM_MAX_S); return DSM_ERR_UNSUPPORTED; }
    if (G < 1 || G > DSM_MAX_G) { dsm_set_error("fit: G=%d outside 1..%d", G, DSM_MAX_G); return DSM_ERR_UNSUPPORTED; }
    int lg = 0;
    while (lg < 6 && (1 << lg) < S) ++lg;
    const int need = (S + 63) / 64;
    pl->lpv = 1 << lg;
    pl->nsl = need <= 1 ? 1 : (need <= 2 ? 2 : (need <= 4 ? 4 : 8));
    const int SP = pl->lpv * pl->nsl, ppb = 256 / pl->lpv;
    pl->gc = std::max(1, std::min(G, FIT_LDS_GAMMA / SP));
    pl->tiles = (V + ppb - 1) / ppb;
    int parts = g_fit_parts > 0 ? g_fit_parts : (int)std::min<long long>({(FIT_BLOCKS + pl->tiles - 1) / pl->tiles, ((long long)n_it + 31) / 32, 1024});
    pl->parts = std::max(1, std::min({parts, n_it, 65535}));     // gridDim.z; a part past the last iteration writes zeros
    return DSM_OK;
}

template <int NSL>
static void fit_launch(dsm_ctx *c, const FitPlan &pl, const FitParams &p)
{
    const int SP = pl.lpv * NSL;
    const size_t lds = std::max((size_t)pl.gc * SP + 16, (size_t)256 * NSL) * sizeof(double);
    hipLaunchKernelGGL((trace_fit_kernel<NSL>), dim3((unsigned)pl.tiles, 1, (unsigned)pl.parts), dim3(256), lds, c->stream, p);
}

// n_it >= 1 iterations; d_samp_part [parts][tiles][S][4], d_pos_part [parts][V][4], d_cell_part [parts][V][S] (with d_cell, else null)
// are scratch the caller sized by fit_plan; d_sample [S][4], d_position [V][4], d_cell [V][S] or null
int k_trace_fit_stats(dsm_ctx *c, const FitPlan &pl, const TraceView &tr, int n_it, double *d_samp_part, double *d_pos_part,
                      double *d_cell_part, double *d_sample, double *d_position, double *d_cell)
{
    FitParams p;
    p.cnt = c->cnt_vs; p.trace = tr.tau; p.trace_stride = tr.tau_stride; p.gamma = tr.gamma; p.eta = tr.eta;
    p.n = n_it; p.V = c->V; p.S = c->S; p.G = c->G; p.gc = pl.gc;
    p.lpv_log2 = 0;
    while ((1 << p.lpv_log2) < pl.lpv) ++p.lpv_log2;
    p.samp_part = d_samp_part; p.pos_part = d_pos_part; p.cell_part = d_cell ? d_cell_part : nullptr;
    switch (pl.nsl) {
    case 1: fit_launch<1>(c, pl, p); break;
    case 2: fit_launch<2>(c, pl, p); break;
    case 4: fit_launch<4>(c, pl, p); break;
    default: fit_launch<8>(c, pl, p); break;
    }
    HIP_TRY(hipGetLastError());
    const size_t V = (size_t)c->V, S = (size_t)c->S;
    hipLaunchKernelGGL(fit_merge_sample_kernel, dim3((unsigned)S), dim3(256), 0, c->stream, d_samp_part, (size_t)pl.parts * pl.tiles, (int)S,
                       d_sample);
    hipLaunchKernelGGL(fit_merge_parts_kernel, dim3((unsigned)((V * 4 + 255) / 256)), dim3(256), 0, c->stream, d_pos_part, V * 4, pl.parts,
                       d_position);
    if (d_cell)
        hipLaunchKernelGGL(fit_merge_parts_kernel, dim3((unsigned)((V * S + 255) / 256)), dim3(256), 0, c->stream, d_cell_part, V * S,
                           pl.parts, d_cell);
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}
