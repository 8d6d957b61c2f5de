// kernels_assign.hip -- exact joint haplotype assignment of positions that were not in the fit
// (desman/HaploSNP_Sampler.py:233-261, assignTau; bin/desman:209-240).
//
// For one position with counts x[s][b], fitted gamma [S][G], eta [4][4] ([true][observed]) and a joint state
// t = (a_0 .. a_{G-1}), index idx(t) = sum_g a_g 4^(G-1-g) (haplotype 0 is the most significant digit):
//     p_t[s][b] = sum_g gamma[s][g] eta[a_g][b],   L(t) = sum_{s,b: x > 0} x[s][b] ln p_t[s][b],
//     post(t) = exp(L(t) - logZ),  logZ = ln sum_t exp L(t).
// All 4^G states are evaluated (DSM_ASSIGN_MAX_G = 10: about a million), everything in fp64, logarithms by dsm_log.
//
// Shape of the work:
//   * a workgroup is ONE wavefront; its 64 lanes hold the 4^3 combinations of the three least significant haplotypes ("inner"
//     digits), so the counts, gamma and the mixture of the outer haplotypes are wave-uniform: cells with a zero count are dropped
//     from the wavefront's cell list once (no divergence), and L(t) needs no cross-lane reduction.  G < 3: the missing inner
//     haplotypes carry gamma = 0 and lanes >= 4^G are switched off.
//   * the outer haplotypes are a loop over "blocks" o = 0 .. 4^(G-3) - 1 of 64 states; the outer mixture sum_{g outer} gamma eta of
//     the listed cells is rebuilt per block with the lanes over the cells ((G - 3) fma per cell and block, against 64 x (3 fma + log)
//     for the states), so a state costs 3 fma + one logarithm + one fma per non-zero cell.
//   * one pass with a running (max, sum exp, argmax) and the 4 G marginal sums, rescaled when the maximum moves.
//   * the states of a position are cut into P = min(4^(G-3), 64) PARTIALS of consecutive blocks, one wavefront each, which leave
//     (max, sum, best L, best idx, marg[G][4]) in a scratch row; assign_merge_kernel folds the P rows of a position in index order.
//     P depends on G only and every sum runs in a fixed order: no float atomics, nothing depends on scheduling, on how the positions
//     are chunked or on which entry point was called.
//   * the optional draw inverts the CDF over idx order with one Philox uniform keyed by (seed, position): the merge kernel finds
//     the partial the uniform falls into, a second launch re-runs that partial only (1/P of the first pass) and scans for the state.
//
// A position whose every state has L = -inf (eta / gamma with exact zeros that contradict the counts): map_state = 0..0, conf = 0,
// logz = -inf, marg = 0, draw_state = 0..0.  Where x = 0 the cell is not evaluated at all, so 0 ln 0 never arises.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dsm_device.h"
#include "dsm_host.h"
#include "dsm_host_util.h"
#include "log_table.h"

#define DSM_STREAM_ASGN 0x4153474Eu   // 'ASGN'  the posterior draw of dsm_assign_tau

struct AssignParams {
    const int32_t *cnt;         // [N][S][4]
    const double *gamma;        // [S][G]
    const double *eta;          // [16]
    const double *log_tab;      // [256][2]
    int N, S, G, P, bpp;        // partials per position, blocks per partial
    double *part;               // [N][P][4 + 4 G]: max, sum exp(L - max), best L, best idx, marg [G][4] (scaled like the sum)
    const int *dj;              // draw: partial the uniform falls into (-1: no state has mass)
    const double *dr;           // draw: target inside that partial, in units of exp(-max of the partial)
    uint32_t *didx;             // draw: the state
};

static size_t assign_lds_bytes(int S, int G)
{
    const int GO = G > 3 ? G - 3 : 0, ROW = 4 + GO;
    return (size_t)DSM_LOG_TAB_N * 16 + 16 * 8 + (size_t)S * ROW * 8 + (size_t)S * 4 * 8 * 2 + 64 * 8 + (size_t)S * 4 * 2;
}

// MODE 0: one partial of one position -> its scratch row.  MODE 1: the draw inside partial dj[v].
template <int MODE>
__global__ __launch_bounds__(64) void assign_kernel(AssignParams p)
{
    extern __shared__ double2 assign_smem[];
    const int S = p.S, G = p.G, GO = G > 3 ? G - 3 : 0, ROW = 4 + GO, lane = threadIdx.x;
    double2 *ltab = assign_smem;
    double *etaS = reinterpret_cast<double *>(ltab + DSM_LOG_TAB_N);     // [16]
    double *gS = etaS + 16;                   // [S][ROW]: inner slots 0..2 (haplotypes G-3..G-1; 0 where there is none), a pad, the outer haplotypes 0..GO-1
    double *cx = gS + (size_t)S * ROW;        // counts of the listed cells, by observed base then sample
    double *base = cx + (size_t)S * 4;        // outer mixture of the listed cells for the running block
    double *wsc = base + (size_t)S * 4;       // [64] the weights of the block the draw falls into
    uint16_t *cs = reinterpret_cast<uint16_t *>(wsc + 64);   // sample of the listed cells

    int v, j;
    if (MODE == 0) { v = blockIdx.x / p.P; j = blockIdx.x % p.P; }
    else {
        v = blockIdx.x; j = p.dj[v];
        if (j < 0) { if (lane == 0) p.didx[v] = 0u; return; }
    }

    for (int i = lane; i < DSM_LOG_TAB_N; i += 64) ltab[i] = reinterpret_cast<const double2 *>(p.log_tab)[i];
    if (lane < 16) etaS[lane] = p.eta[lane];
    for (int i = lane; i < S * ROW; i += 64) {
        const int s = i / ROW, k = i - s * ROW;
        const int g = k < 3 ? G - 3 + k : k - 4;
        gS[i] = (k != 3 && g >= 0) ? p.gamma[(size_t)s * G + g] : 0.0;
    }
    // the cell list: non-zero counts only, observed base by observed base
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
    __syncthreads();

    // this lane's inner digits and their eta rows
    double e[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int d = (lane >> (2 * (2 - k))) & 3;
#pragma unroll
        for (int b = 0; b < 4; ++b) e[k][b] = etaS[d * 4 + b];
    }
    const bool lane_on = G >= 3 || lane < (1 << (2 * G));
    const double NINF = -INFINITY;

    double m = NINF, Wl = 0.0, oacc[4] = {0.0, 0.0, 0.0, 0.0}, bestL = NINF;
    uint32_t bestI = 0xffffffffu;
    double cum = 0.0, mj = 0.0, target = 0.0;
    uint32_t lastpos = 0u, found = 0xffffffffu;
    if (MODE == 1) { mj = p.part[((size_t)v * p.P + j) * (4 + 4 * G)]; target = p.dr[v]; }

    const int o0 = j * p.bpp, o1 = o0 + p.bpp;
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
        if (GO > 0) __syncthreads();          // the next block rewrites `base`

        if (MODE == 0) {
            const double mB = wave_max_f64(L);
            if (mB > m) {                       // wave-uniform
                const double sc = (m == NINF) ? 0.0 : exp(m - mB);
                Wl *= sc;
#pragma unroll
                for (int k = 0; k < 4; ++k) oacc[k] *= sc;
                m = mB;
            }
            const double w = (L == NINF) ? 0.0 : exp(L - m);
            Wl += w;
            if (GO > 0) {
                const double bs = group_allreduce_sum<64>(w);
                const int a = lane < GO ? (o >> (2 * (GO - 1 - lane))) & 3 : -1;       // lane g < GO keeps the sums of outer haplotype g
#pragma unroll
                for (int k = 0; k < 4; ++k) oacc[k] += (a == k) ? bs : 0.0;
            }
            if (L > bestL) { bestL = L; bestI = (uint32_t)o * 64u + (uint32_t)lane; }
        } else {
            const double w = (L == NINF) ? 0.0 : exp(L - mj);
            const double bs = group_allreduce_sum<64>(w);
            const unsigned long long mk = __ballot(w > 0.0);
            if (mk) lastpos = (uint32_t)o * 64u + (uint32_t)(63 - __clzll(mk));
            if (cum + bs >= target || o == o1 - 1) {      // wave-uniform
                wsc[lane] = w;
                __syncthreads();
                if (lane == 0) {
                    double c = cum;
                    for (int l = 0; l < 64; ++l) {
                        c += wsc[l];
                        if (wsc[l] > 0.0 && c >= target) { found = (uint32_t)o * 64u + (uint32_t)l; break; }
                    }
                    p.didx[v] = found != 0xffffffffu ? found : lastpos;      // rounding at the last edge: the last state with mass
                }
                return;
            }
            cum += bs;
        }
    }

    if (MODE == 0) {
        double *row = p.part + ((size_t)v * p.P + j) * (4 + 4 * G);
        const double Z = group_allreduce_sum<64>(Wl);
        // argmax: largest L, ties to the lowest index
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double oL = __shfl_xor(bestL, off, 64);
            const uint32_t oI = (uint32_t)__shfl_xor((int)bestI, off, 64);
            if (oL > bestL || (oL == bestL && oI < bestI)) { bestL = oL; bestI = oI; }
        }
        if (lane == 0) { row[0] = m; row[1] = Z; row[2] = bestL; row[3] = (double)bestI; }
        if (lane < GO) {
#pragma unroll
            for (int k = 0; k < 4; ++k) row[4 + lane * 4 + k] = oacc[k];
        }
        // inner haplotypes: sums of the lanes' totals by digit
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int g = G - 3 + k, d = (lane >> (2 * (2 - k))) & 3;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const double t = group_allreduce_sum<64>(d == a ? Wl : 0.0);
                if (lane == 0 && g >= 0) row[4 + g * 4 + a] = t;
            }
        }
    }
}

// one thread per position: folds its P partial rows in index order
__global__ __launch_bounds__(64) void assign_merge_kernel(const double *__restrict__ part, int N, int G, int P, unsigned long long seed,
                                                          unsigned long long pos0, int want_draw, uint32_t *__restrict__ map_idx,
                                                          double *__restrict__ conf, double *__restrict__ logz, double *__restrict__ marg,
                                                          int *__restrict__ dj, double *__restrict__ dr)
{
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= N) return;
    const int R = 4 + 4 * G;
    const double *rows = part + (size_t)v * P * R;
    const double NINF = -INFINITY;
    double M = NINF, bestL = NINF;
    uint32_t bestI = 0u;
    for (int j = 0; j < P; ++j) {
        const double *r = rows + (size_t)j * R;
        M = fmax(M, r[0]);
        if (r[2] > bestL) { bestL = r[2]; bestI = (uint32_t)r[3]; }     // rows are in index order: strict > keeps the lowest index
    }
    double *mg = marg + (size_t)v * 4 * G;
    if (M == NINF) {
        map_idx[v] = 0u; conf[v] = 0.0; logz[v] = NINF;
        for (int k = 0; k < 4 * G; ++k) mg[k] = 0.0;
        if (want_draw) { dj[v] = -1; dr[v] = 0.0; }
        return;
    }
    double Z = 0.0;
    for (int k = 0; k < 4 * G; ++k) mg[k] = 0.0;
    for (int j = 0; j < P; ++j) {
        const double *r = rows + (size_t)j * R;
        if (r[0] == NINF) continue;
        const double f = (r[0] == M) ? 1.0 : exp(r[0] - M);
        Z = fma(r[1], f, Z);
        for (int k = 0; k < 4 * G; ++k) mg[k] = fma(r[4 + k], f, mg[k]);
    }
    map_idx[v] = bestI;
    conf[v] = 1.0 / Z;                       // best L == M: exp(L_max - M) = 1
    logz[v] = M + log(Z);
    for (int k = 0; k < 4 * G; ++k) mg[k] /= Z;
    if (want_draw) {
        const unsigned long long pos = pos0 + (unsigned long long)v;
        uint32_t w[4];
        philox4x32_10((uint32_t)pos, (uint32_t)(pos >> 32), DSM_STREAM_ASGN, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        const double T = u01_open(w[0], w[1]) * Z;
        double c = 0.0, rr = 0.0;
        int js = -1, jl = -1;
        double cl = 0.0, fl = 1.0;
        for (int j = 0; j < P && js < 0; ++j) {
            const double *r = rows + (size_t)j * R;
            if (r[0] == NINF) continue;
            const double f = (r[0] == M) ? 1.0 : exp(r[0] - M);
            const double zj = r[1] * f;
            if (!(zj > 0.0)) continue;
            jl = j; cl = c; fl = f;
            if (c + zj >= T) { js = j; rr = (T - c) / f; }
            c += zj;
        }
        if (js < 0) { js = jl; rr = (T - cl) / fl; }                // rounding at the last edge: the last partial with mass
        dj[v] = js; dr[v] = rr;
    }
}

// ---------------------------------------------------------------- host side
static int g_assign_chunk = 0;      // dsm_assign_debug_set_chunk: positions per launch (0 = by the scratch bound)

extern "C" int dsm_assign_debug_set_chunk(int positions)
{
    return dsm_set_knob(&g_assign_chunk, positions, "assign", "chunk");
}

static int assign_check_model(int S, int G, const double *gamma, const double *eta)
{
    if (S < 1 || G < 1) { dsm_set_error("assign: S=%d, G=%d", S, G); return DSM_ERR_ARG; }
    if (S > DSM_MAX_S) { dsm_set_error("assign: S=%d exceeds DSM_MAX_S=%d", S, DSM_MAX_S); return DSM_ERR_UNSUPPORTED; }
    if (G > DSM_ASSIGN_MAX_G) {
        dsm_set_error("assign: G=%d exceeds DSM_ASSIGN_MAX_G=%d (all 4^G joint states are evaluated)", G, DSM_ASSIGN_MAX_G);
        return DSM_ERR_UNSUPPORTED;
    }
    DSM_TRY(dsm_check_gamma("assign", gamma, (size_t)S * G));
    return dsm_check_eta("assign", eta);
}

// d_cnt: the whole tensor on the device (context form), or null with h_cnt = the caller's int64 tensor (uploaded chunk by chunk)
static int assign_run(const int32_t *d_cnt, const int64_t *h_cnt, int N, int S, int G, const double *gamma, const double *eta,
                      uint64_t seed, uint8_t *map_state, double *conf, double *logz, double *marg, uint8_t *draw_state)
{
    const JointSplit js(G);
    const int P = js.P, bpp = js.bpp, R = 4 + 4 * G;
    // positions per launch: the scratch rows stay below 32 MB whatever N is
    int NC = (int)std::max<size_t>(1, std::min<size_t>((size_t)1 << 16, ((size_t)32 << 20) / ((size_t)P * R * sizeof(double))));
    if (g_assign_chunk > 0) NC = g_assign_chunk;
    NC = std::min(NC, N);
    const size_t lds = assign_lds_bytes(S, G);
    DSM_TRY(dsm_allow_lds(reinterpret_cast<const void *>(&assign_kernel<0>), lds, "assign"));
    DSM_TRY(dsm_allow_lds(reinterpret_cast<const void *>(&assign_kernel<1>), lds, "assign"));
    DevBuf<int32_t> d_x; DevBuf<double> d_gamma, d_eta, d_ltab, d_part, d_conf, d_logz, d_marg, d_dr;
    DevBuf<uint32_t> d_map, d_didx; DevBuf<int> d_dj;
    if (!d_cnt) DSM_TRY(d_x.alloc((size_t)NC * S * 4));
    DSM_TRY(d_gamma.alloc((size_t)S * G)); DSM_TRY(d_eta.alloc(16)); DSM_TRY(d_ltab.alloc(2 * DSM_LOG_TAB_N));
    DSM_TRY(d_part.alloc((size_t)NC * P * R)); DSM_TRY(d_conf.alloc(NC)); DSM_TRY(d_logz.alloc(NC)); DSM_TRY(d_marg.alloc((size_t)NC * 4 * G));
    DSM_TRY(d_map.alloc(NC)); DSM_TRY(d_dj.alloc(NC)); DSM_TRY(d_dr.alloc(NC)); DSM_TRY(d_didx.alloc(NC));
    HIP_TRY(hipMemcpy(d_gamma, gamma, (size_t)S * G * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_eta, eta, 16 * sizeof(double), hipMemcpyHostToDevice));
    DSM_TRY(dsm_upload_log_table(d_ltab));
    std::vector<int32_t> x32;
    std::vector<uint32_t> idx((size_t)NC);
    auto unpack = [&](uint8_t *dst, int n0, int n) {
        for (int i = 0; i < n; ++i)
            for (int g = 0; g < G; ++g) dst[(size_t)(n0 + i) * G + g] = (uint8_t)((idx[i] >> (2 * (G - 1 - g))) & 3u);
    };
    for (int n0 = 0; n0 < N; n0 += NC) {
        const int n = std::min(NC, N - n0);
        const int32_t *cnt = d_cnt ? d_cnt + (size_t)n0 * S * 4 : d_x.p;
        if (!d_cnt) DSM_TRY(dsm_stage_counts(h_cnt + (size_t)n0 * S * 4, (size_t)n * S * 4, d_x, x32, nullptr));
        AssignParams q{cnt, d_gamma, d_eta, d_ltab, n, S, G, P, bpp, d_part, d_dj, d_dr, d_didx};
        hipLaunchKernelGGL(assign_kernel<0>, dim3((unsigned)n * (unsigned)P), dim3(64), lds, 0, q);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(assign_merge_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, d_part.p, n, G, P, (unsigned long long)seed,
                           (unsigned long long)n0, draw_state ? 1 : 0, d_map.p, d_conf.p, d_logz.p, d_marg.p, d_dj.p, d_dr.p);
        HIP_TRY(hipGetLastError());
        if (draw_state) {
            hipLaunchKernelGGL(assign_kernel<1>, dim3((unsigned)n), dim3(64), lds, 0, q);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpy(idx.data(), d_map, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        unpack(map_state, n0, n);
        HIP_TRY(hipMemcpy(conf + n0, d_conf, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(logz + n0, d_logz, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(marg + (size_t)n0 * 4 * G, d_marg, (size_t)n * 4 * G * sizeof(double), hipMemcpyDeviceToHost));
        if (draw_state) {
            HIP_TRY(hipMemcpy(idx.data(), d_didx, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            unpack(draw_state, n0, n);
        }
    }
    return DSM_OK;
}

extern "C" int dsm_assign_tau(int device, const int64_t *counts, int N, int S, int G, const double *gamma, const double *eta,
                              uint64_t seed, uint8_t *map_state, double *conf, double *logz, double *marg, uint8_t *draw_state)
{
    if (N < 0 || !gamma || !eta || (N > 0 && (!counts || !map_state || !conf || !logz || !marg))) {
        dsm_set_error("assign_tau: bad arguments");
        return DSM_ERR_ARG;
    }
    DSM_TRY(assign_check_model(S, G, gamma, eta));
    DSM_TRY(dsm_check_counts("assign_tau", counts, (size_t)N, S));
    if (N == 0) return DSM_OK;
    DSM_TRY(dsm_bind_device(device));
    return assign_run(nullptr, counts, N, S, G, gamma, eta, seed, map_state, conf, logz, marg, draw_state);
}

extern "C" int dsm_ctx_assign_tau(dsm_ctx *c, const double *gamma, const double *eta, int G, uint64_t seed, uint8_t *map_state,
                                  double *conf, double *logz, double *marg, uint8_t *draw_state)
{
    DSM_TRY(dsm_ctx_enter(c, true));
    if (!gamma || !eta || !map_state || !conf || !logz || !marg) { dsm_set_error("ctx_assign_tau: null pointer"); return DSM_ERR_ARG; }
    DSM_TRY(assign_check_model(c->S, G, gamma, eta));
    return assign_run(c->cnt_vs, nullptr, c->V, c->S, G, gamma, eta, seed, map_state, conf, logz, marg, draw_state);
}
