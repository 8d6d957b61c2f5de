// kernels_pred.hip -- position-marginal predictive density of a chain from its resident gamma and eta traces
// (dsm_ctx_trace_predictive; desman_amd/predictive.py).
//
// For a stored iteration t and a position with counts x[s][b], with L_t(state) exactly as kernels_assign.hip defines it under
// (gamma_t, eta_t):
//     logz[t][v] = ln sum over the 4^G joint states of exp L_t(state)
// -- the log predictive density of the whole position with its haplotype bases summed out, up to the constants the host adds (the
// multinomial coefficients and -G ln 4).  Then per position, over the used iterations in order:
//     lppd = ln mean_t exp logz     (max-shifted),     mean = mean_t logz,     var = sum_t (logz - mean)^2 / (n - 1)  (a second, centred pass)
//
// Shape of the work: assign_kernel's mapping without what a density does not need.
//   * pred_kernel: a workgroup is ONE wavefront for (position v, partial j, iteration part z); its lanes hold the 4^3 combinations of
//     the three least significant haplotypes, the outer haplotypes are a loop over blocks of 64 states, P = min(4^(G-3), 64) partials
//     of consecutive blocks per position (P depends on G only).  The log table and the position's list of non-zero cells are staged
//     in LDS ONCE; the wavefront then loops over the used iterations of its part and restages only eta_t and gamma_t (S (G + 1)
//     doubles).  Per state: 3 fma + one dsm_log + one fma per non-zero cell, as in assign_kernel and in the same order, then a
//     running (max, sum exp) -- no marginals, no arg-max, no draw.  One (max, sum) row per (t, v, j).
//   * pred_fold_kernel: one thread per (t, v) folds the P rows in index order -- assign_merge_kernel's arithmetic for logz -- into
//     the device matrix logz[t][v].
//   * pred_stats_kernel: one thread per position walks its logz column in iteration order, twice.
// No floating-point atomics; every (t, v, j) row is made by one wavefront from its own operands, so nothing depends on the position
// chunking, on the number of iteration parts or on scheduling.
//
// -inf (every state of (t, v) contradicted by exact zeros in eta_t / gamma_t): zero mass in lppd, mean = -inf, var = +inf; all
// iterations -inf: lppd = -inf.  Every exclusion is a select, so nothing is NaN.
#include <math.h>

#include <algorithm>
#include <vector>

#include "dsm_device.h"
#include "dsm_trace_host.h"
#include "log_table.h"

#define PRED_WAVES 4096                     // wavefronts a launch aims at (256 compute units x 16) before iterations are cut into parts
#define PRED_PART_BYTES ((size_t)64 << 20)  // bound of the (max, sum) rows of one launch
#define PRED_LOGZ_BYTES ((size_t)32 << 20)  // bound of the logz matrix of one position chunk (one position's column at the least)

struct PredParams {
    const int32_t *cnt;         // [n][S][4] the chunk's positions
    const double *gamma;        // trace row of used iteration 0 of this launch
    const double *eta;
    size_t step;                // trace rows between two used iterations (the stride)
    const double *log_tab;      // [256][2]
    int n, S, G, P, bpp;        // positions, partials per position, blocks per partial
    int nt, tpp;                // used iterations of this launch, iterations per part
    double *part;               // [nt][n][P][2]: max, sum exp(L - max)
};

static size_t pred_lds_bytes(int S, int G)
{
    const int GO = G > 3 ? G - 3 : 0, ROW = 4 + GO;
    return (size_t)DSM_LOG_TAB_N * 16 + 16 * 8 + (size_t)S * ROW * 8 + (size_t)S * 4 * 8 * 2 + (size_t)S * 4 * 2;
}

__global__ __launch_bounds__(64) void pred_kernel(const PredParams p)
{
    extern __shared__ double2 pred_smem[];
    const int S = p.S, G = p.G, GO = G > 3 ? G - 3 : 0, ROW = 4 + GO, lane = threadIdx.x;
    double2 *ltab = pred_smem;
    double *etaS = reinterpret_cast<double *>(ltab + DSM_LOG_TAB_N);     // [16]
    double *gS = etaS + 16;                   // [S][ROW]: inner slots 0..2 (haplotypes G-3..G-1; 0 where there is none), a pad, the outer haplotypes
    double *cx = gS + (size_t)S * ROW;        // counts of the listed cells, by observed base then sample
    double *base = cx + (size_t)S * 4;        // outer mixture of the listed cells for the running block
    uint16_t *cs = reinterpret_cast<uint16_t *>(base + (size_t)S * 4);   // sample of the listed cells

    const int v = blockIdx.x / p.P, j = blockIdx.x % p.P;
    const int t0 = min(p.nt, (int)blockIdx.y * p.tpp), t1 = min(p.nt, t0 + p.tpp);

    for (int i = lane; i < DSM_LOG_TAB_N; i += 64) ltab[i] = reinterpret_cast<const double2 *>(p.log_tab)[i];
    // the cell list: non-zero counts only, observed base by observed base; built once for all iterations
    int cstart[5];
    cstart[0] = 0;
    {
        int n = 0;
        const int32_t *row = p.cnt + (size_t)v * S * 4;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            for (int s0 = 0; s0 < S; s0 += 64) {
                const int s = s0 + lane;
                const int x = s < S ? row[s * 4 + b] : 0;
                const unsigned long long mk = __ballot(x > 0);
                if (x > 0) {
                    const int pos = n + __popcll(mk & ((1ull << lane) - 1ull));
                    cx[pos] = (double)x;
                    cs[pos] = (uint16_t)s;
                }
                n += __popcll(mk);
            }
            cstart[b + 1] = n;
        }
    }
    for (int i = lane; i < cstart[4]; i += 64) base[i] = 0.0;

    const bool lane_on = G >= 3 || lane < (1 << (2 * G));
    const double NINF = -INFINITY;
    const int o0 = j * p.bpp, o1 = o0 + p.bpp;
    const size_t sg = (size_t)S * G;

    for (int t = t0; t < t1; ++t) {
        const double *gam = p.gamma + (size_t)t * p.step * sg, *eta = p.eta + (size_t)t * p.step * 16;
        __syncthreads();                      // the readers of the previous iteration's tables are done
        if (lane < 16) etaS[lane] = eta[lane];
        for (int i = lane; i < S * ROW; i += 64) {
            const int s = i / ROW, k = i - s * ROW;
            const int g = k < 3 ? G - 3 + k : k - 4;
            gS[i] = (k != 3 && g >= 0) ? gam[(size_t)s * G + g] : 0.0;
        }
        __syncthreads();

        // this lane's inner digits and their eta rows
        double e[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int d = (lane >> (2 * (2 - k))) & 3;
#pragma unroll
            for (int b = 0; b < 4; ++b) e[k][b] = etaS[d * 4 + b];
        }

        double m = NINF, Wl = 0.0;
        for (int o = o0; o < o1; ++o) {
            if (GO > 0) {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    for (int i = cstart[b] + lane; i < cstart[b + 1]; i += 64) {
                        const double *gr = gS + (int)cs[i] * ROW + 4;
                        double acc = 0.0;
                        for (int g = 0; g < GO; ++g) acc = fma(gr[g], etaS[((o >> (2 * (GO - 1 - g))) & 3) * 4 + b], acc);
                        base[i] = acc;
                    }
                __syncthreads();
            }
            double L = 0.0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double e0 = e[0][b], e1 = e[1][b], e2 = e[2][b];
#pragma unroll 2
                for (int i = cstart[b]; i < cstart[b + 1]; ++i) {
                    const double *gr = gS + (int)cs[i] * ROW;
                    const double pr = fma(gr[0], e0, fma(gr[1], e1, fma(gr[2], e2, base[i])));
                    L = fma(cx[i], dsm_log(pr, ltab), L);
                }
            }
            if (!lane_on) L = NINF;
            if (GO > 0) __syncthreads();      // the next block rewrites `base`

            const double mB = wave_max_f64(L);
            if (mB > m) {                       // wave-uniform
                Wl *= (m == NINF) ? 0.0 : exp(m - mB);
                m = mB;
            }
            Wl += (L == NINF) ? 0.0 : exp(L - m);
        }
        const double Z = group_allreduce_sum<64>(Wl);
        if (lane == 0) {
            double *row = p.part + (((size_t)t * p.n + v) * p.P + j) * 2;
            row[0] = m; row[1] = Z;
        }
    }
}

// one thread per (t, v) of the launch: folds its P rows in index order into logz[t][v] (row stride n)
__global__ __launch_bounds__(256) void pred_fold_kernel(const double *__restrict__ part, size_t cells, int P, double *__restrict__ logz)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const double *rows = part + i * P * 2;
    const double NINF = -INFINITY;
    double M = NINF;
    for (int j = 0; j < P; ++j) M = fmax(M, rows[j * 2]);
    if (M == NINF) { logz[i] = NINF; return; }
    double Z = 0.0;
    for (int j = 0; j < P; ++j) {
        const double mj = rows[j * 2];
        if (mj == NINF) continue;
        const double f = (mj == M) ? 1.0 : exp(mj - M);
        Z = fma(rows[j * 2 + 1], f, Z);
    }
    logz[i] = M + log(Z);
}

// one thread per position: its logz column [nu] (row stride n) in iteration order -> lppd, mean, var
__global__ __launch_bounds__(256) void pred_stats_kernel(const double *__restrict__ logz, int n, int nu, double *__restrict__ lppd,
                                                         double *__restrict__ mean, double *__restrict__ var)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const double NINF = -INFINITY;
    double M = NINF, sum = 0.0;
    bool hole = false;
    for (int t = 0; t < nu; ++t) {
        const double z = logz[(size_t)t * n + v];
        M = fmax(M, z);
        hole = hole || z == NINF;
        sum += z == NINF ? 0.0 : z;
    }
    double w = 0.0;
    for (int t = 0; t < nu; ++t) {
        const double z = logz[(size_t)t * n + v];
        w += z == NINF ? 0.0 : exp(z - M);      // M is finite wherever some z is
    }
    lppd[v] = M == NINF ? NINF : M + log(w / (double)nu);
    const double mu = sum / (double)nu;
    double q = 0.0;
    for (int t = 0; t < nu; ++t) {
        const double d = hole ? 0.0 : logz[(size_t)t * n + v] - mu;
        q += d * d;
    }
    mean[v] = hole ? NINF : mu;
    var[v] = hole ? INFINITY : (nu > 1 ? q / (double)(nu - 1) : 0.0);
}

// ---------------------------------------------------------------- host side
static int g_pred_chunk = 0;        // dsm_pred_debug_set_chunk: positions per chunk (0 = by the scratch bounds)
static int g_pred_parts = 0;        // dsm_pred_debug_set_parts: iteration parts of a launch (0 = by the grid the launch aims at)

extern "C" int dsm_pred_debug_set_chunk(int positions)
{
    return dsm_set_knob(&g_pred_chunk, positions, "pred", "chunk");
}

extern "C" int dsm_pred_debug_set_parts(int parts)
{
    return dsm_set_knob(&g_pred_parts, parts, "pred", "parts");
}

extern "C" int dsm_ctx_trace_predictive(dsm_ctx *c, const int64_t *counts, int N, int it0, int n_it, int stride, double *lppd,
                                        double *mean, double *var, double *logz_it)
{
    DSM_TRY(trace_range(c, "trace_predictive", it0, n_it));
    BIND(c);                                           // everything below runs on c->stream
    if (stride < 1) { dsm_set_error("trace_predictive: stride %d", stride); return DSM_ERR_ARG; }
    const int S = c->S, G = c->G;
    if (G > DSM_ASSIGN_MAX_G) {
        dsm_set_error("trace_predictive: G=%d exceeds DSM_ASSIGN_MAX_G=%d (all 4^G joint states are evaluated)", G, DSM_ASSIGN_MAX_G);
        return DSM_ERR_UNSUPPORTED;
    }
    if (counts) {
        if (N < 0) { dsm_set_error("trace_predictive: N=%d", N); return DSM_ERR_ARG; }
        DSM_TRY(dsm_check_counts("trace_predictive", counts, (size_t)N, S));
    } else N = c->V;
    if (n_it == 0 || N == 0) return DSM_OK;

    const int nu = (n_it + stride - 1) / stride;
    const JointSplit js(G);
    const int P = js.P, bpp = js.bpp;
    const size_t lds = pred_lds_bytes(S, G);
    DSM_TRY(dsm_allow_lds(reinterpret_cast<const void *>(&pred_kernel), lds, "trace_predictive"));
    // positions per chunk: the logz matrix [nu][NC] stays below PRED_LOGZ_BYTES; iterations per launch: the rows [TC][NC][P][2] below
    // PRED_PART_BYTES -- one position's column and one iteration's rows at the least
    int NC = (int)std::max<size_t>(1, std::min<size_t>((size_t)1 << 16, PRED_LOGZ_BYTES / ((size_t)nu * sizeof(double))));
    if (g_pred_chunk > 0) NC = std::min(g_pred_chunk, 1 << 16);
    NC = std::min(NC, N);
    const int TC = (int)std::max<size_t>(1, std::min<size_t>((size_t)nu, PRED_PART_BYTES / ((size_t)NC * P * 2 * sizeof(double))));

    DevBuf<int32_t> d_x; DevBuf<double> d_part, d_logz, d_lppd, d_mean, d_var;
    if (counts) DSM_TRY(d_x.alloc((size_t)NC * S * 4));
    DSM_TRY(d_part.alloc((size_t)TC * NC * P * 2)); DSM_TRY(d_logz.alloc((size_t)nu * NC));
    DSM_TRY(d_lppd.alloc(NC)); DSM_TRY(d_mean.alloc(NC)); DSM_TRY(d_var.alloc(NC));
    std::vector<int32_t> x32;
    for (int n0 = 0; n0 < N; n0 += NC) {
        const int n = std::min(NC, N - n0);
        const int32_t *cnt = counts ? d_x.p : c->cnt_vs + (size_t)n0 * S * 4;
        if (counts) DSM_TRY(dsm_stage_counts(counts + (size_t)n0 * S * 4, (size_t)n * S * 4, d_x, x32, c->stream));
        for (int u0 = 0; u0 < nu; u0 += TC) {
            const int nt = std::min(TC, nu - u0);
            int parts = g_pred_parts > 0 ? g_pred_parts : (int)((PRED_WAVES + (long long)n * P - 1) / ((long long)n * P));
            parts = std::max(1, std::min({parts, nt, 65535}));
            const TraceView tr = trace_view(c, it0 + u0 * stride);
            PredParams q{cnt, tr.gamma, tr.eta, (size_t)stride, c->log_tab, n, S, G, P, bpp,
                         nt, (nt + parts - 1) / parts, d_part};
            hipLaunchKernelGGL(pred_kernel, dim3((unsigned)n * (unsigned)P, (unsigned)parts), dim3(64), lds, c->stream, q);
            HIP_TRY(hipGetLastError());
            const size_t cells = (size_t)nt * n;
            hipLaunchKernelGGL(pred_fold_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, d_part.p, cells, P,
                               d_logz.p + (size_t)u0 * n);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(pred_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_logz.p, n, nu, d_lppd.p,
                           d_mean.p, d_var.p);
        HIP_TRY(hipGetLastError());
        if (lppd) HIP_TRY(hipMemcpyAsync(lppd + n0, d_lppd, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (mean) HIP_TRY(hipMemcpyAsync(mean + n0, d_mean, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (var) HIP_TRY(hipMemcpyAsync(var + n0, d_var, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (logz_it)
            HIP_TRY(hipMemcpy2DAsync(logz_it + n0, (size_t)N * sizeof(double), d_logz, (size_t)n * sizeof(double), (size_t)n * sizeof(double),
                                     (size_t)nu, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return DSM_OK;
}
