// kernels_abund.hip -- abundances of fitted haplotypes in samples that were not in the fit.
//
// With tau [V][G] and eta [4][4] ([true][observed]) held fixed the samples are independent and the log-likelihood of one sample,
//     L(gamma) = sum_{v,b: x_vb > 0} x_vb ln p_vb,     p_vb = sum_g gamma_g eta[tau_vg][b],
// is concave in its gamma row.  One EM step from an interior point:
//     r_g = gamma_g sum_{v,b: x > 0} x_vb eta[tau_vg][b] / p_vb,     gamma'_g = r_g / N,     N = sum x,
// evaluated through the class sums  c_a = sum_{g: tau_vg = a} gamma_g  (p_vb = sum_a c_a eta[a][b]) and the class weights
// w_a = sum_b x_vb eta[a][b] / p_vb  (r_g = gamma_g sum_v w_{tau_vg}): 8 G + ~100 fp64 operations per position instead of 4 G per cell.
// A FIT is a (sample, mask) pair: the full fit (f = 0), or the fit with haplotype f - 1 excluded (gamma_g = 0 from the start,
// the start uniform over the others), whose maximum gives the likelihood-ratio statistic of "haplotype g is absent".
//
// Shape of the work:
//   * a workgroup is ONE sample and NW of its F = 1 (+ G) fits, one WAVEFRONT per fit (more fits than a workgroup may have wavefronts -- NWMAX = 12 up to
//     G = 8, 8 up to G = 16, 4 above, by the registers a lane needs --: the fits are cut into ceil(F / NWMAX) groups of equal size, blockIdx.y).  The 64 lanes of a fit stride over the positions; gamma and the G
//     accumulators of sum_v w_{tau_vg} live in registers (the kernel is instantiated for G padded to 4 / 8 / 16 / 32).
//   * the sample's counts (int32 x 4) and the packed tau words are staged in LDS in tiles of DSM_ABUND_TILE positions by the whole
//     workgroup, and every wavefront of the workgroup reads the tile from there: the 1 + G fits of a sample fetch its counts from
//     memory once per iteration and group, not 1 + G times.  V <= DSM_ABUND_TILE: the tile is loaded once and stays for all iterations.
//   * the whole EM loop runs in the kernel: the stop test max_g |gamma' - gamma| < tol is a wave-uniform value, a fit that is done
//     writes its results and idles through the barriers of the tiles until the workgroup's other fits are done too.
//   * every sum has one order: a lane adds its positions lane, lane + 64, ... in turn, the 64 lane totals meet in the xor butterfly.
//     Neither depends on the tile, on the other wavefronts of the workgroup or on which samples share a launch, so a sample's numbers
//     are the same bits with and without the presence fits, for any chunking and from both entry points.
//   * EM passes take no logarithm; one more pass at the end evaluates L at the gamma that is returned.
//
// Degenerate operands: N = 0 -> the start row, loglik 0, iters 0, converged 1.  A cell with x > 0 and p = 0 in any pass (exact zeros in
// eta that contradict the counts: at the uniform start already) -> gamma row 0, loglik -inf, converged 0.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dsm_device.h"
#include "dsm_host.h"
#include "dsm_host_util.h"
#include "log_table.h"

#define DSM_ABUND_TILE 2048          // positions per LDS tile: 32 KB of counts + 16 KB of tau words

struct AbundParams {
    const int32_t *cnt;         // [n][V][4] sample-major
    const uint64_t *tau;        // [V] packed, haplotype g at bits 2 g
    const double *eta;          // [16]
    const double *log_tab;      // [256][2]
    int V, G, F, NW, max_iter;
    double tol;
    double *gamma;              // [n][G] of the full fit
    double *ll;                 // [n][F]
    double *dev;                // [n]
    int32_t *iters, *conv;      // [n]
};

// this lane's rows of the staged tile.  KIND 0: N and the saturated log-likelihood; 1: one EM pass (acc_g += w of g's class; bad: a
// cell with reads and p = 0); 2: L at gam.  ETA (with KIND 1, the joint fit of gamma and eta below): m[4 a + b] += c_a q_b as well
template <int GP, int KIND, bool ETA>
__device__ __forceinline__ void abund_rows_impl(int n, int lane, const int4 *__restrict__ xS, const uint64_t *__restrict__ tS,
                                                const double *__restrict__ etaS, const double2 *__restrict__ ltab, const double (&gam)[GP],
                                                double (&acc)[GP], double &o0, double &o1, bool &bad, double *__restrict__ m)
{
    for (int i = lane; i < n; i += 64) {
        const int4 xi = xS[i];
        const int xv[4] = {xi.x, xi.y, xi.z, xi.w};
        if (KIND == 0) {
            const double nv = (double)xi.x + (double)xi.y + (double)xi.z + (double)xi.w;       // exact: below 2^33
            o0 += nv;                                                                          // exact below 2^53
            const double ln = dsm_log(nv, ltab);
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (xv[b] > 0) o1 = fma((double)xv[b], dsm_log((double)xv[b], ltab) - ln, o1);
            continue;
        }
        const uint64_t t = tS[i];
        double c[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int g = 0; g < GP; ++g) {
            const int d = (int)(t >> (2 * g)) & 3;
#pragma unroll
            for (int a = 0; a < 4; ++a) c[a] += (d == a) ? gam[g] : 0.0;
        }
        double q[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double pb = fma(c[3], etaS[12 + b], fma(c[2], etaS[8 + b], fma(c[1], etaS[4 + b], c[0] * etaS[b])));
            const double x = (double)xv[b];
            if (KIND == 1) {
                q[b] = 0.0;
                if (xv[b] > 0) {
                    if (!(pb > 0.0)) bad = true;
                    else q[b] = pb >= 0x1p-500 ? fdiv(x, pb) : x / pb;
                }
            } else if (xv[b] > 0) o0 = fma(x, dsm_log(pb, ltab), o0);
        }
        if (KIND == 1) {
            double w[4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
                w[a] = fma(q[3], etaS[a * 4 + 3], fma(q[2], etaS[a * 4 + 2], fma(q[1], etaS[a * 4 + 1], q[0] * etaS[a * 4])));
#pragma unroll
            for (int g = 0; g < GP; ++g) {
                const int d = (int)(t >> (2 * g)) & 3;
                acc[g] += d == 0 ? w[0] : d == 1 ? w[1] : d == 2 ? w[2] : w[3];
            }
            if (ETA) {
#pragma unroll
                for (int k = 0; k < 16; ++k) m[k] = fma(c[k >> 2], q[k & 3], m[k]);
            }
        }
    }
}

template <int GP, int KIND>
__device__ __forceinline__ void abund_rows(int n, int lane, const int4 *__restrict__ xS, const uint64_t *__restrict__ tS,
                                           const double *__restrict__ etaS, const double2 *__restrict__ ltab, const double (&gam)[GP],
                                           double (&acc)[GP], double &o0, double &o1, bool &bad)
{
    abund_rows_impl<GP, KIND, false>(n, lane, xS, tS, etaS, ltab, gam, acc, o0, o1, bad, nullptr);
}

template <int GP, int NWMAX>
__global__ __launch_bounds__(NWMAX * 64) void abund_kernel(AbundParams p)
{
    __shared__ int4 xS[DSM_ABUND_TILE];
    __shared__ uint64_t tS[DSM_ABUND_TILE];
    __shared__ double2 ltab[DSM_LOG_TAB_N];
    __shared__ double etaS[16];
    __shared__ int doneS[NWMAX];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nthr = blockDim.x, nw = nthr >> 6;
    const int V = p.V, G = p.G, s = blockIdx.x, f = blockIdx.y * p.NW + wave;
    const int4 *cnt4 = reinterpret_cast<const int4 *>(p.cnt) + (size_t)s * V;
    const bool resident = V <= DSM_ABUND_TILE;
    const double NINF = -INFINITY;

    for (int i = threadIdx.x; i < DSM_LOG_TAB_N; i += nthr) ltab[i] = reinterpret_cast<const double2 *>(p.log_tab)[i];
    if (threadIdx.x < 16) etaS[threadIdx.x] = p.eta[threadIdx.x];
    auto stage = [&](int t0) {
        __syncthreads();                                   // the previous tile has been read by every wavefront
        const int n = min(DSM_ABUND_TILE, V - t0);
        for (int i = threadIdx.x; i < n; i += nthr) { xS[i] = cnt4[t0 + i]; tS[i] = p.tau[t0 + i]; }
        __syncthreads();
    };

    bool done = f >= p.F;                                  // a wavefront without a fit only keeps the barriers
    const int Ga = f == 0 ? G : G - 1;                     // haplotypes of this fit (F > 1 only with G > 1)
    double gam[GP], acc[GP];
#pragma unroll
    for (int g = 0; g < GP; ++g) { gam[g] = (g < G && g != f - 1) ? 1.0 / (double)Ga : 0.0; acc[g] = 0.0; }
    int iters = 0, conv = 0;
    double ll = 0.0, N = 0.0, Lsat = 0.0;
    bool dead = false;

    // N and the saturated model
    {
        double o0 = 0.0, o1 = 0.0; bool bad = false;
        for (int t0 = 0; t0 < V; t0 += DSM_ABUND_TILE) {
            if (!resident || t0 == 0) stage(t0);
            if (!done) abund_rows<GP, 0>(min(DSM_ABUND_TILE, V - t0), lane, xS, tS, etaS, ltab, gam, acc, o0, o1, bad);
        }
        N = group_allreduce_sum<64>(o0);
        Lsat = group_allreduce_sum<64>(o1);
    }
    bool finish = !done && N == 0.0;                       // no reads: the start row, L = 0
    if (finish) conv = 1;

    for (;;) {
        if (finish) {
            if (lane == 0) {
                p.ll[(size_t)s * p.F + f] = dead ? NINF : ll;
                if (f == 0) {
                    p.dev[s] = dead ? INFINITY : 2.0 * (Lsat - ll);
                    p.iters[s] = iters; p.conv[s] = dead ? 0 : conv;
#pragma unroll
                    for (int g = 0; g < GP; ++g) if (g < G) p.gamma[(size_t)s * G + g] = dead ? 0.0 : gam[g];
                }
            }
            finish = false; done = true;
        }
        // the workgroup goes on until each of its fits is done
        if (lane == 0) doneS[wave] = done ? 1 : 0;
        __syncthreads();
        bool all = true;
        for (int w = 0; w < nw; ++w) all = all && doneS[w] != 0;
        if (all) break;
        __syncthreads();                                   // (V in one tile: no barrier below before doneS is written again)

        const bool last = iters == p.max_iter || conv;     // wave-uniform: the pass that evaluates L at the final gamma
        double o0 = 0.0, o1 = 0.0; bool bad = false;
#pragma unroll
        for (int g = 0; g < GP; ++g) acc[g] = 0.0;
        for (int t0 = 0; t0 < V; t0 += DSM_ABUND_TILE) {
            if (!resident) stage(t0);
            if (done) continue;
            const int n = min(DSM_ABUND_TILE, V - t0);
            if (last) abund_rows<GP, 2>(n, lane, xS, tS, etaS, ltab, gam, acc, o0, o1, bad);
            else abund_rows<GP, 1>(n, lane, xS, tS, etaS, ltab, gam, acc, o0, o1, bad);
        }
        if (done) continue;
        if (last) {
            ll = group_allreduce_sum<64>(o0);
            if (!(ll > NINF)) dead = true;                 // (max_iter = 0 on a table the start contradicts; NaN cannot arise: p >= 0)
            finish = true;
            continue;
        }
        if (__ballot(bad) != 0ull) { dead = true; finish = true; continue; }
        double delta = 0.0;
#pragma unroll
        for (int g = 0; g < GP; ++g) {
            const double tot = group_allreduce_sum<64>(acc[g]);
            const double gn = gam[g] > 0.0 ? gam[g] * tot / N : 0.0;
            delta = fmax(delta, fabs(gn - gam[g]));
            gam[g] = gn;
        }
        ++iters;
        if (p.tol > 0.0 && delta < p.tol) conv = 1;
    }
}

// the resident tensor [V][S][4] -> samples s0 .. s0 + n - 1 as [n][V][4]
__global__ __launch_bounds__(256) void abund_repack_kernel(const int4 *__restrict__ in, int4 *__restrict__ out, int V, int S, int s0)
{
    const int v = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (v < V) out[(size_t)i * V + v] = in[(size_t)v * S + s0 + i];
}

// ---------------------------------------------------------------- host side
static int g_abund_chunk = 0;      // dsm_abund_debug_set_chunk: samples per launch (0 = by the scratch bound)

extern "C" int dsm_abund_debug_set_chunk(int samples)
{
    return dsm_set_knob(&g_abund_chunk, samples, "abund", "chunk");
}

template <int GP, int NWMAX>
static void abund_launch(const AbundParams &q, int n, int groups)
{
    hipLaunchKernelGGL((abund_kernel<GP, NWMAX>), dim3((unsigned)n, (unsigned)groups), dim3((unsigned)q.NW * 64u), 0, 0, q);
}

static int abund_check_model(int V, int G, const double *eta, int max_iter, double tol)
{
    if (V < 1 || G < 1 || G > DSM_MAX_G) { dsm_set_error("fit_gamma: V=%d, G=%d (1 <= G <= DSM_MAX_G=%d)", V, G, DSM_MAX_G); return DSM_ERR_ARG; }
    if (max_iter < 0 || !(tol >= 0.0) || !std::isfinite(tol)) { dsm_set_error("fit_gamma: max_iter=%d, tol=%g", max_iter, tol); return DSM_ERR_ARG; }
    return dsm_check_eta("fit_gamma", eta);
}

// The tau of a call, host half (argument checks only: it runs before the device is touched).  tau digits [V][G] -> packed words,
// DSM_ERR_ARG on a digit outside 0..3; tau null -- the context form `who` on the resident state, which must have G haplotypes -- leaves
// `out` empty.
static int abund_tau_words(const char *who, const dsm_ctx *c, const int64_t *tau, int V, int G, std::vector<uint64_t> &out)
{
    if (!tau) {
        if (!c->have_state || c->G != G) { dsm_set_error("%s: no tau given and no resident state of G=%d haplotypes", who, G); return DSM_ERR_STATE; }
        return DSM_OK;
    }
    out.assign((size_t)V, 0ull);
    for (int v = 0; v < V; ++v) {
        uint64_t t = 0;
        for (int g = 0; g < G; ++g) {
            const int64_t d = tau[(size_t)v * G + g];
            if (d < 0 || d > 3) { dsm_set_error("fit_gamma: tau[%d][%d] = %lld is not a base 0..3", v, g, (long long)d); return DSM_ERR_ARG; }
            t |= (uint64_t)d << (2 * g);
        }
        out[(size_t)v] = t;
    }
    return DSM_OK;
}

// ... device half, once the device is current: the words of abund_tau_words uploaded into `own`, or the context's resident tau
static int abund_tau_on_device(const dsm_ctx *c, const std::vector<uint64_t> &words, DevBuf<uint64_t> &own, const uint64_t **d_tau)
{
    if (words.empty()) { *d_tau = c->tau; return DSM_OK; }
    DSM_TRY(own.alloc(words.size()));
    HIP_TRY(hipMemcpy(own, words.data(), words.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    *d_tau = own;
    return DSM_OK;
}

// samples s0 .. s0 + n - 1 sample-major in d_x: from the resident tensor d_cnt [V][S][4], or -- d_cnt null -- from the caller's int64 tensor
static int abund_stage_chunk(const int32_t *d_cnt, const int64_t *h_cnt, int V, int S, int s0, int n, int32_t *d_x, std::vector<int32_t> &x32)
{
    if (d_cnt) {
        hipLaunchKernelGGL(abund_repack_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)n), dim3(256), 0, 0,
                           reinterpret_cast<const int4 *>(d_cnt), reinterpret_cast<int4 *>(d_x), V, S, s0);
        HIP_TRY(hipGetLastError());
        return DSM_OK;
    }
    x32.resize((size_t)n * V * 4);
    for (int v = 0; v < V; ++v)
        for (int i = 0; i < n; ++i) {
            const int64_t *src = h_cnt + ((size_t)v * S + s0 + i) * 4;
            int32_t *dst = x32.data() + ((size_t)i * V + v) * 4;
            for (int b = 0; b < 4; ++b) dst[b] = (int32_t)src[b];
        }
    HIP_TRY(hipMemcpy(d_x, x32.data(), x32.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return DSM_OK;
}

// samples per launch: the sample-major copy of the counts stays below 64 MB (one sample's V x 16 B at the least)
static int abund_chunk(int V, int S)
{
    int NC = (int)std::max<size_t>(1, std::min<size_t>((size_t)1 << 15, ((size_t)64 << 20) / ((size_t)V * 16)));
    if (g_abund_chunk > 0) NC = g_abund_chunk;
    return std::min(NC, S);
}

// d_cnt: the resident tensor [V][S][4] (context form), or null with h_cnt = the caller's int64 tensor; d_tau: packed words on the device
static int abund_run(const int32_t *d_cnt, const int64_t *h_cnt, int V, int S, int G, const uint64_t *d_tau, const double *eta,
                     int max_iter, double tol, int presence, double *gamma, double *loglik, double *deviance, int32_t *iters,
                     int32_t *converged, double *lr_absent)
{
    const int F = (presence && G > 1) ? 1 + G : 1;
    const int GP = G <= 4 ? 4 : G <= 8 ? 8 : G <= 16 ? 16 : 32, NWMAX = GP <= 8 ? 12 : GP == 16 ? 8 : 4;      // wavefronts a workgroup may have, i.e. a budget of 168 / 256 / 512 vector registers per lane (used: DESIGN.md sec. 8b; no vector spills, no scratch)
    const int groups = (F + NWMAX - 1) / NWMAX, NW = (F + groups - 1) / groups;
    const int NC = abund_chunk(V, S);
    DevBuf<int32_t> d_x, d_iters, d_conv; DevBuf<double> d_eta, d_ltab, d_gamma, d_ll, d_dev;
    DSM_TRY(d_x.alloc((size_t)NC * V * 4)); DSM_TRY(d_eta.alloc(16)); DSM_TRY(d_ltab.alloc(2 * DSM_LOG_TAB_N));
    DSM_TRY(d_gamma.alloc((size_t)NC * G)); DSM_TRY(d_ll.alloc((size_t)NC * F)); DSM_TRY(d_dev.alloc(NC));
    DSM_TRY(d_iters.alloc(NC)); DSM_TRY(d_conv.alloc(NC));
    HIP_TRY(hipMemcpy(d_eta, eta, 16 * sizeof(double), hipMemcpyHostToDevice));
    DSM_TRY(dsm_upload_log_table(d_ltab));
    std::vector<int32_t> x32;
    std::vector<double> ll((size_t)NC * F);
    for (int s0 = 0; s0 < S; s0 += NC) {
        const int n = std::min(NC, S - s0);
        DSM_TRY(abund_stage_chunk(d_cnt, h_cnt, V, S, s0, n, d_x, x32));
        AbundParams q{d_x, d_tau, d_eta, d_ltab, V, G, F, NW, max_iter, tol, d_gamma, d_ll, d_dev, d_iters, d_conv};
        switch (GP) {
        case 4: abund_launch<4, 12>(q, n, groups); break;
        case 8: abund_launch<8, 12>(q, n, groups); break;
        case 16: abund_launch<16, 8>(q, n, groups); break;
        default: abund_launch<32, 4>(q, n, groups); break;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(gamma + (size_t)s0 * G, d_gamma, (size_t)n * G * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ll.data(), d_ll, (size_t)n * F * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(deviance + s0, d_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(iters + s0, d_iters, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(converged + s0, d_conv, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) {
            const double L = ll[(size_t)i * F];
            loglik[s0 + i] = L;
            if (!lr_absent) continue;
            for (int g = 0; g < G; ++g) {
                // G = 1: no haplotype is left, the restricted model gives the reads probability 0
                const double d = F > 1 ? 2.0 * (L - ll[(size_t)i * F + 1 + g]) : INFINITY;
                lr_absent[(size_t)(s0 + i) * G + g] = d < 0.0 ? 0.0 : d;       // (the restricted maximum cannot lie above: rounding only)
            }
        }
    }
    return DSM_OK;
}

extern "C" int dsm_fit_gamma(int device, const int64_t *counts, int V, int S, int G, const int64_t *tau, const double *eta,
                             int max_iter, double tol, int presence, double *gamma, double *loglik, double *deviance,
                             int32_t *iters, int32_t *converged, double *lr_absent)
{
    if (S < 0 || !tau || !eta || (S > 0 && (!counts || !gamma || !loglik || !deviance || !iters || !converged))) {
        dsm_set_error("fit_gamma: bad arguments");
        return DSM_ERR_ARG;
    }
    DSM_TRY(abund_check_model(V, G, eta, max_iter, tol));
    DSM_TRY(dsm_check_counts("fit_gamma", counts, (size_t)V, S));
    std::vector<uint64_t> words;
    DSM_TRY(abund_tau_words("fit_gamma", nullptr, tau, V, G, words));
    if (S == 0) return DSM_OK;
    DSM_TRY(dsm_bind_device(device));
    DevBuf<uint64_t> own;
    const uint64_t *d_tau = nullptr;
    DSM_TRY(abund_tau_on_device(nullptr, words, own, &d_tau));
    return abund_run(nullptr, counts, V, S, G, d_tau, eta, max_iter, tol, presence, gamma, loglik, deviance, iters, converged, lr_absent);
}

extern "C" int dsm_ctx_fit_gamma(dsm_ctx *c, int G, const int64_t *tau, const double *eta, int max_iter, double tol, int presence,
                                 double *gamma, double *loglik, double *deviance, int32_t *iters, int32_t *converged, double *lr_absent)
{
    DSM_TRY(dsm_ctx_enter(c, true));
    if (!eta || !gamma || !loglik || !deviance || !iters || !converged) { dsm_set_error("ctx_fit_gamma: null pointer"); return DSM_ERR_ARG; }
    DSM_TRY(abund_check_model(c->V, G, eta, max_iter, tol));
    std::vector<uint64_t> words;
    DSM_TRY(abund_tau_words("ctx_fit_gamma", c, tau, c->V, G, words));
    DevBuf<uint64_t> own;
    const uint64_t *d_tau = nullptr;
    DSM_TRY(abund_tau_on_device(c, words, own, &d_tau));
    return abund_run(c->cnt_vs, nullptr, c->V, c->S, G, d_tau, eta, max_iter, tol, presence, gamma, loglik, deviance,
                     iters, converged, lr_absent);
}

// ---------------------------------------------------------------- profile-likelihood intervals of the abundances
// For haplotype g the profile log-likelihood  l_g(c) = max { L(gamma) : gamma_g = c, gamma_h >= 0, sum gamma = 1 }  is concave in c; the
// interval is { c : 2 (L(gamma_hat) - l_g(c)) <= q }.  A SEARCH is a (haplotype, side) pair, k = 2 g + side (0: lower end, 1: upper end):
// a bisection on c whose every trial is an inner fit -- EM over the other haplotypes with gamma_g held at c,
//     r_h = gamma_h sum_v w_{tau_vh},     gamma'_h = (1 - c) r_h / sum_{h != g} r_h      (the sum in index order),
// stopped as the fit is, followed by one pass that evaluates L.  The exact rules (bracket, endpoint test, start of an inner fit, what
// counts as outside) are in include/desman_hip.h and restated in tests/_abund_interval_ref.py.
//
// Shape of the work: that of abund_kernel, with a search where it has a fit -- a workgroup is one sample and NW of its 2 G searches, one
// wavefront per search, which runs its whole bisection here (fit, evaluate, halve, refit); the tiles, their barriers and the order of
// every sum are the fit's (abund_rows<GP, 1> and <GP, 2> are called, not copied).  The number of passes a search needs is wave-uniform
// and differs between the searches of a workgroup: a search that is done idles through the tile barriers until the others are.
// The held haplotype takes part in every pass with gamma_g = c (the class sums need it) and is never updated: its accumulator is
// formed like the others and ignored.  The search state (c, the bracket, L(gamma_hat), counters) is wave-uniform.
struct AbundIvParams {
    const int32_t *cnt;         // [n][V][4] sample-major
    const uint64_t *tau;        // [V] packed
    const double *eta;          // [16]
    const double *log_tab;      // [256][2]
    const double *ghat;         // [n][G] the fitted rows
    int V, G, NW, max_iter;
    double tol, ctol, q;
    double *res;                // [n][2 G] the end that search k found
    int32_t *fl;                // [n][2 G] its flag bits
};

template <int GP, int NWMAX>
__global__ __launch_bounds__(NWMAX * 64) void abund_interval_kernel(AbundIvParams p)
{
    __shared__ int4 xS[DSM_ABUND_TILE];
    __shared__ uint64_t tS[DSM_ABUND_TILE];
    __shared__ double2 ltab[DSM_LOG_TAB_N];
    __shared__ double etaS[16];
    __shared__ int doneS[NWMAX];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nthr = blockDim.x, nw = nthr >> 6;
    const int V = p.V, G = p.G, s = blockIdx.x, k = blockIdx.y * p.NW + wave, g = k >> 1, side = k & 1;
    const int4 *cnt4 = reinterpret_cast<const int4 *>(p.cnt) + (size_t)s * V;
    const double *ghat = p.ghat + (size_t)s * G;
    const bool resident = V <= DSM_ABUND_TILE;
    const double NINF = -INFINITY;

    for (int i = threadIdx.x; i < DSM_LOG_TAB_N; i += nthr) ltab[i] = reinterpret_cast<const double2 *>(p.log_tab)[i];
    if (threadIdx.x < 16) etaS[threadIdx.x] = p.eta[threadIdx.x];
    auto stage = [&](int t0) {
        __syncthreads();                                   // the previous tile has been read by every wavefront
        const int n = min(DSM_ABUND_TILE, V - t0);
        for (int i = threadIdx.x; i < n; i += nthr) { xS[i] = cnt4[t0 + i]; tS[i] = p.tau[t0 + i]; }
        __syncthreads();
    };

    bool done = k >= 2 * G;                                // a wavefront without a search only keeps the barriers
    double gam[GP], acc[GP];
    double sumhat = 0.0;
#pragma unroll
    for (int h = 0; h < GP; ++h) { gam[h] = h < G ? ghat[h] : 0.0; acc[h] = 0.0; sumhat += gam[h]; }

    enum { M_LHAT, M_EM, M_EVAL };                          // the pass in flight: L(gamma_hat), an EM step, l at the end of an inner fit
    int mode = M_LHAT, iters = 0, conv = 0, flags = 0;
    double c = 0.0, b_in = 0.0, b_out = 0.0, Lhat = 0.0, result = 0.0, N = 0.0;
    bool endpoint = false, finish = false;

    {
        double o0 = 0.0, o1 = 0.0; bool bad = false;
        for (int t0 = 0; t0 < V; t0 += DSM_ABUND_TILE) {
            if (!resident || t0 == 0) stage(t0);
            if (!done) abund_rows<GP, 0>(min(DSM_ABUND_TILE, V - t0), lane, xS, tS, etaS, ltab, gam, acc, o0, o1, bad);
        }
        N = group_allreduce_sum<64>(o0);
    }
    if (!done) {
        if (!(sumhat > 0.0)) { result = NAN; finish = true; }                                      // a dead row of the fit
        else if (G == 1) { result = 1.0; flags = side ? 2 : 0; finish = true; }                    // nothing is free: [1, 1]
        else if (N == 0.0) { result = side ? 1.0 : 0.0; flags = side ? 2 : 1; finish = true; }     // no reads: [0, 1]
    }

    for (;;) {
        if (finish) {
            if (lane == 0) { p.res[(size_t)s * 2 * G + k] = result; p.fl[(size_t)s * 2 * G + k] = flags; }
            finish = false; done = true;
        }
        // the workgroup goes on until each of its searches is done
        if (lane == 0) doneS[wave] = done ? 1 : 0;
        __syncthreads();
        bool all = true;
        for (int w = 0; w < nw; ++w) all = all && doneS[w] != 0;
        if (all) break;
        __syncthreads();                                   // (V in one tile: no barrier below before doneS is written again)

        double o0 = 0.0, o1 = 0.0; bool bad = false;
#pragma unroll
        for (int h = 0; h < GP; ++h) acc[h] = 0.0;
        for (int t0 = 0; t0 < V; t0 += DSM_ABUND_TILE) {
            if (!resident) stage(t0);
            if (done) continue;
            const int n = min(DSM_ABUND_TILE, V - t0);
            if (mode == M_EM) abund_rows<GP, 1>(n, lane, xS, tS, etaS, ltab, gam, acc, o0, o1, bad);
            else abund_rows<GP, 2>(n, lane, xS, tS, etaS, ltab, gam, acc, o0, o1, bad);
        }
        if (done) continue;

        // everything below is wave-uniform
        bool decided = false, inside = false, start = false;
        if (mode == M_EM) {
            if (__ballot(bad) != 0ull) decided = true;     // a cell with reads and p = 0: this c is outside
            else {
                double R = 0.0;
#pragma unroll
                for (int h = 0; h < GP; ++h) {
                    acc[h] = gam[h] * group_allreduce_sum<64>(acc[h]);
                    R += h != g ? acc[h] : 0.0;
                }
                if (!(R > 0.0)) { conv = 1; mode = M_EVAL; }                    // the free haplotypes explain no read: nothing moves
                else {
                    const double omc = 1.0 - c;
                    double delta = 0.0;
#pragma unroll
                    for (int h = 0; h < GP; ++h) {
                        const double gn = h == g ? c : gam[h] > 0.0 ? omc * acc[h] / R : 0.0;      // gamma_g = c survives the step
                        delta = fmax(delta, fabs(gn - gam[h]));
                        gam[h] = gn;
                    }
                    ++iters;
                    if (p.tol > 0.0 && delta < p.tol) conv = 1;
                    if (conv || iters == p.max_iter) mode = M_EVAL;
                }
            }
        } else {
            const double ll = group_allreduce_sum<64>(o0);
            if (mode == M_LHAT) {
                Lhat = ll;
                double gg = 0.0;
#pragma unroll
                for (int h = 0; h < GP; ++h) gg = h == g ? gam[h] : gg;
                b_in = gg; b_out = side ? 1.0 : 0.0;
                if (!(Lhat > NINF)) { result = NAN; finish = true; }             // gamma_hat itself contradicts the counts
                else if (b_in == b_out) { result = b_out; flags = side ? 2 : 1; finish = true; }
                else { endpoint = true; c = b_out; start = true; }               // the far end of the bracket first
            } else {
                if (!conv) flags |= 4;
                decided = true;
                inside = 2.0 * (Lhat - ll) <= p.q;                               // (l = -inf: outside)
            }
        }
        if (decided) {
            if (endpoint) {
                endpoint = false;
                if (inside) { result = b_out; flags |= side ? 2 : 1; finish = true; }
            } else if (inside) b_in = c;
            else b_out = c;
            if (!finish) {
                const double m = 0.5 * (b_in + b_out);
                if (!(fabs(b_out - b_in) > p.ctol) || m == b_in || m == b_out) { result = b_in; finish = true; }
                else { c = m; start = true; }
            }
        }
        if (start) {
            // the inner fit at c starts from the free part of the previous one (of gamma_hat: the first; whenever that part is all 0)
            double F = 0.0;
#pragma unroll
            for (int h = 0; h < GP; ++h) F += h != g ? gam[h] : 0.0;
            if (!(F > 0.0)) {
                F = 0.0;
#pragma unroll
                for (int h = 0; h < GP; ++h) { gam[h] = h < G ? ghat[h] : 0.0; F += h != g ? gam[h] : 0.0; }
                if (!(F > 0.0)) {
#pragma unroll
                    for (int h = 0; h < GP; ++h) gam[h] = (h < G && h != g) ? 1.0 : 0.0;
                    F = (double)(G - 1);
                }
            }
            const double omc = 1.0 - c, u = 0.001 / (double)(G - 1);
#pragma unroll
            for (int h = 0; h < GP; ++h)
                gam[h] = h == g ? c : h >= G ? 0.0 : G == 2 ? omc : omc * (0.999 * (gam[h] / F) + u);
            const bool nofit = G == 2 || c == 1.0;                               // the free part is determined: one evaluation
            iters = 0; conv = nofit ? 1 : 0;
            mode = (nofit || p.max_iter == 0) ? M_EVAL : M_EM;
        }
    }
}

template <int GP, int NWMAX>
static void abund_interval_launch(const AbundIvParams &q, int n, int groups)
{
    hipLaunchKernelGGL((abund_interval_kernel<GP, NWMAX>), dim3((unsigned)n, (unsigned)groups), dim3((unsigned)q.NW * 64u), 0, 0, q);
}

static int abund_check_interval(int S, int G, const double *gamma_hat, double q, double ctol)
{
    if (!(q > 0.0) || !std::isfinite(q) || !(ctol > 0.0) || !(ctol < 1.0)) { dsm_set_error("fit_gamma_interval: q=%g, ctol=%g", q, ctol); return DSM_ERR_ARG; }
    for (int s = 0; s < S; ++s) {
        double sum = 0.0;
        for (int g = 0; g < G; ++g) {
            const double x = gamma_hat[(size_t)s * G + g];
            if (!(x >= 0.0) || !(x <= 1.0)) { dsm_set_error("fit_gamma_interval: gamma_hat[%d][%d] = %g is outside [0, 1]", s, g, x); return DSM_ERR_ARG; }
            sum += x;
        }
        if (sum != 0.0 && !(fabs(sum - 1.0) <= 1e-9)) { dsm_set_error("fit_gamma_interval: gamma_hat row %d sums to %.17g", s, sum); return DSM_ERR_ARG; }
    }
    return DSM_OK;
}

// as abund_run: d_cnt the resident tensor or null with h_cnt; d_tau the packed words on the device
static int abund_interval_run(const int32_t *d_cnt, const int64_t *h_cnt, int V, int S, int G, const uint64_t *d_tau, const double *eta,
                              const double *gamma_hat, double q, int max_iter, double tol, double ctol, double *lo, double *hi, int32_t *flags)
{
    const int K = 2 * G;
    const int GP = G <= 4 ? 4 : G <= 8 ? 8 : G <= 16 ? 16 : 32, NWMAX = GP == 4 ? 12 : GP <= 16 ? 8 : 4;      // a budget of 168 / 256 / 256 / 512 vector registers per lane (used: DESIGN.md sec. 8b; no scratch)
    const int groups = (K + NWMAX - 1) / NWMAX, NW = (K + groups - 1) / groups;
    const int NC = abund_chunk(V, S);
    DevBuf<int32_t> d_x, d_fl; DevBuf<double> d_eta, d_ltab, d_ghat, d_res;
    DSM_TRY(d_x.alloc((size_t)NC * V * 4)); DSM_TRY(d_eta.alloc(16)); DSM_TRY(d_ltab.alloc(2 * DSM_LOG_TAB_N));
    DSM_TRY(d_ghat.alloc((size_t)NC * G)); DSM_TRY(d_res.alloc((size_t)NC * K)); DSM_TRY(d_fl.alloc((size_t)NC * K));
    HIP_TRY(hipMemcpy(d_eta, eta, 16 * sizeof(double), hipMemcpyHostToDevice));
    DSM_TRY(dsm_upload_log_table(d_ltab));
    std::vector<int32_t> x32, fl((size_t)NC * K);
    std::vector<double> res((size_t)NC * K);
    for (int s0 = 0; s0 < S; s0 += NC) {
        const int n = std::min(NC, S - s0);
        DSM_TRY(abund_stage_chunk(d_cnt, h_cnt, V, S, s0, n, d_x, x32));
        HIP_TRY(hipMemcpy(d_ghat, gamma_hat + (size_t)s0 * G, (size_t)n * G * sizeof(double), hipMemcpyHostToDevice));
        AbundIvParams a{d_x, d_tau, d_eta, d_ltab, d_ghat, V, G, NW, max_iter, tol, ctol, q, d_res, d_fl};
        switch (GP) {
        case 4: abund_interval_launch<4, 12>(a, n, groups); break;
        case 8: abund_interval_launch<8, 8>(a, n, groups); break;
        case 16: abund_interval_launch<16, 8>(a, n, groups); break;
        default: abund_interval_launch<32, 4>(a, n, groups); break;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(res.data(), d_res, (size_t)n * K * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(fl.data(), d_fl, (size_t)n * K * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < (size_t)n * G; ++i) {
            lo[(size_t)s0 * G + i] = res[2 * i];
            hi[(size_t)s0 * G + i] = res[2 * i + 1];
            flags[(size_t)s0 * G + i] = fl[2 * i] | fl[2 * i + 1];
        }
    }
    return DSM_OK;
}

extern "C" int dsm_fit_gamma_interval(int device, const int64_t *counts, int V, int S, int G, const int64_t *tau, const double *eta,
                                      const double *gamma_hat, double q, int max_iter, double tol, double ctol, double *lo, double *hi,
                                      int32_t *flags)
{
    if (S < 0 || !tau || !eta || (S > 0 && (!counts || !gamma_hat || !lo || !hi || !flags))) {
        dsm_set_error("fit_gamma_interval: bad arguments");
        return DSM_ERR_ARG;
    }
    DSM_TRY(abund_check_model(V, G, eta, max_iter, tol));
    DSM_TRY(dsm_check_counts("fit_gamma", counts, (size_t)V, S));
    DSM_TRY(abund_check_interval(S, G, gamma_hat, q, ctol));
    std::vector<uint64_t> words;
    DSM_TRY(abund_tau_words("fit_gamma_interval", nullptr, tau, V, G, words));
    if (S == 0) return DSM_OK;
    DSM_TRY(dsm_bind_device(device));
    DevBuf<uint64_t> own;
    const uint64_t *d_tau = nullptr;
    DSM_TRY(abund_tau_on_device(nullptr, words, own, &d_tau));
    return abund_interval_run(nullptr, counts, V, S, G, d_tau, eta, gamma_hat, q, max_iter, tol, ctol, lo, hi, flags);
}

extern "C" int dsm_ctx_fit_gamma_interval(dsm_ctx *c, int G, const int64_t *tau, const double *eta, const double *gamma_hat, double q,
                                          int max_iter, double tol, double ctol, double *lo, double *hi, int32_t *flags)
{
    DSM_TRY(dsm_ctx_enter(c, true));
    if (!eta || !gamma_hat || !lo || !hi || !flags) { dsm_set_error("ctx_fit_gamma_interval: null pointer"); return DSM_ERR_ARG; }
    DSM_TRY(abund_check_model(c->V, G, eta, max_iter, tol));
    DSM_TRY(abund_check_interval(c->S, G, gamma_hat, q, ctol));
    std::vector<uint64_t> words;
    DSM_TRY(abund_tau_words("ctx_fit_gamma_interval", c, tau, c->V, G, words));
    DevBuf<uint64_t> own;
    const uint64_t *d_tau = nullptr;
    DSM_TRY(abund_tau_on_device(c, words, own, &d_tau));
    return abund_interval_run(c->cnt_vs, nullptr, c->V, c->S, G, d_tau, eta, gamma_hat, q, max_iter, tol, ctol, lo, hi, flags);
}

// ---------------------------------------------------------------- the error matrix of new samples, fitted with gamma
// tau fixed; gamma [S][G] and ONE eta [4][4] shared by the samples of the call maximise  L(gamma, eta) = sum_s sum_{v,b: x > 0} x ln p
// by plain EM.  One step, from one E-step at (gamma, eta):  q_svb = x / p,
//     gamma'_sg = gamma_sg / N_s sum_v w_{s,v,tau_vg}        (the fit's step),
//     M[a][b] = eta[a][b] sum_s sum_v c_sva q_svb,           eta'[a][b] = M[a][b] / sum_b M[a][b]   (a row of sum 0 keeps its values).
// The eta statistics couple the samples, so a step is a PAIR OF LAUNCHES on the stream and the loop is the host's:
//   * abund_eta_step_kernel: a workgroup is one sample.  There are no presence fits, so the NW wavefronts of the workgroup SHARE the
//     sample's positions: the workgroup stages the fit's LDS tiles, wavefront w takes the w-th contiguous slice of every tile (slices of
//     ceil(n / (64 NW)) 64 positions of a tile of n), its lanes stride over the slice with the fit's arithmetic (abund_rows_impl) and add
//     the 16 sums c_a q_b besides.  Lane totals meet in the xor butterfly, the wavefront totals in LDS, added in wavefront order by
//     wavefront 0.  NW depends on the G class alone (8 / 8 / 8 / 4), so every sum has one order for a given V.
//   * abund_eta_reduce_kernel: one wavefront adds the samples' 16 partial sums in sample order, forms eta', the step's delta and the
//     device-side stop word (converged, dead, or max_iter reached).  Both kernels return at once when stop is set, so the host may
//     enqueue steps in batches and read stop between batches: a step launched after stop changes nothing.
//   * abund_eta_eval_kernel: N and the saturated model before the first step, L at the returned (gamma, eta) after the last, in the
//     order of the fit's final pass (one wavefront per sample over the fit's tiles, abund_rows<GP, 2>).
// No atomics; no launch depends on another workgroup of the same launch.
enum { AE_STOP = 0, AE_ITERS, AE_CONV, AE_DEAD, AE_ROWS, AE_NCTRL = 8 };

struct AbundEtaParams {
    const int32_t *cnt;         // [S][V][4] sample-major, every sample of the call
    const uint64_t *tau;        // [V] packed
    const double *log_tab;      // [256][2]
    int V, G, S, max_iter;
    double tol;
    double *gamma;              // [S][G] the current rows, updated in place by the sample's workgroup
    double *eta;                // [16] the current matrix, updated by the reduce kernel
    double *N, *Lsat, *ll;      // [S]
    double *part;               // [S][16] sum_v c_a q_b of the step
    double *delta;              // [S] max_g |gamma' - gamma| of the step
    int32_t *bad;               // [S] a cell with reads and p = 0
    int32_t *ctrl;              // [AE_NCTRL]
};

template <int GP, int NW>
__global__ __launch_bounds__(NW * 64) void abund_eta_step_kernel(AbundEtaParams p)
{
    __shared__ int4 xS[DSM_ABUND_TILE];
    __shared__ uint64_t tS[DSM_ABUND_TILE];
    __shared__ double etaS[16];
    __shared__ double redS[NW][GP + 16];
    __shared__ int badS[NW];

    if (p.ctrl[AE_STOP] != 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nthr = NW * 64;
    const int V = p.V, G = p.G, s = blockIdx.x;
    const double N = p.N[s];
    if (N == 0.0) return;                                  // no reads: nothing for M (part, delta and bad stay 0), the row stays
    const int4 *cnt4 = reinterpret_cast<const int4 *>(p.cnt) + (size_t)s * V;
    double *grow = p.gamma + (size_t)s * G;

    if (threadIdx.x < 16) etaS[threadIdx.x] = p.eta[threadIdx.x];
    double gam[GP], acc[GP], m[16];
#pragma unroll
    for (int g = 0; g < GP; ++g) { gam[g] = g < G ? grow[g] : 0.0; acc[g] = 0.0; }
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = 0.0;
    double o0 = 0.0, o1 = 0.0; bool bad = false;

    for (int t0 = 0; t0 < V; t0 += DSM_ABUND_TILE) {
        __syncthreads();                                   // the previous tile has been read by every wavefront
        const int n = min(DSM_ABUND_TILE, V - t0);
        for (int i = threadIdx.x; i < n; i += nthr) { xS[i] = cnt4[t0 + i]; tS[i] = p.tau[t0 + i]; }
        __syncthreads();
        const int per = (n + nthr - 1) / nthr * 64, lo = min(n, wave * per), cnt = min(per, n - lo);
        abund_rows_impl<GP, 1, true>(cnt, lane, xS + lo, tS + lo, etaS, nullptr, gam, acc, o0, o1, bad, m);
    }
#pragma unroll
    for (int g = 0; g < GP; ++g) acc[g] = group_allreduce_sum<64>(acc[g]);
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = group_allreduce_sum<64>(m[k]);
    const bool wbad = __ballot(bad) != 0ull;
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < GP; ++g) redS[wave][g] = acc[g];
#pragma unroll
        for (int k = 0; k < 16; ++k) redS[wave][GP + k] = m[k];
        badS[wave] = wbad ? 1 : 0;
    }
    __syncthreads();                                       // (every wavefront has read its gamma row long before)
    if (wave != 0) return;
    bool anybad = false;
    for (int w = 0; w < NW; ++w) anybad = anybad || badS[w] != 0;
    if (anybad) { if (lane == 0) p.bad[s] = 1; return; }
    // lane j: entry j of the wavefront totals, added in wavefront order -- j < GP: haplotype j, GP <= j < GP + 16: c_a q_b
    double tot = 0.0, d = 0.0;
    if (lane < GP + 16) {
        tot = redS[0][lane];
        for (int w = 1; w < NW; ++w) tot += redS[w][lane];
    }
    if (lane < G) {
        const double g0 = grow[lane], gn = g0 > 0.0 ? g0 * tot / N : 0.0;
        d = fabs(gn - g0);
        grow[lane] = gn;
    }
    if (lane >= GP && lane < GP + 16) p.part[(size_t)s * 16 + (lane - GP)] = tot;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) d = fmax(d, __shfl_xor(d, off, 64));
    if (lane == 0) p.delta[s] = d;
}

__global__ __launch_bounds__(64) void abund_eta_reduce_kernel(AbundEtaParams p)
{
    if (p.ctrl[AE_STOP] != 0) return;
    const int lane = threadIdx.x, k = lane & 15, a = k >> 2, S = p.S;
    int bad = 0;
    double dg = 0.0;
    for (int s = lane; s < S; s += 64) { bad |= p.bad[s]; dg = fmax(dg, p.delta[s]); }
    if (__ballot(bad != 0) != 0ull) {                      // eta is shared: the whole call's fit is dead, nothing else is written
        if (lane == 0) { p.ctrl[AE_DEAD] = 1; p.ctrl[AE_STOP] = 1; }
        return;
    }
    double sum = 0.0;                                      // (lanes k, k + 16, k + 32, k + 48 hold the same entry)
    for (int s = 0; s < S; ++s) sum += p.part[(size_t)s * 16 + k];
    const double e0 = p.eta[k], M = e0 * sum;
    const double rs = ((__shfl(M, 4 * a, 64) + __shfl(M, 4 * a + 1, 64)) + __shfl(M, 4 * a + 2, 64)) + __shfl(M, 4 * a + 3, 64);
    const bool live = rs > 0.0;
    const double en = live ? M / rs : e0;                  // a dead row keeps its values
    double d = fmax(dg, fabs(en - e0));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) d = fmax(d, __shfl_xor(d, off, 64));
    const unsigned long long deadl = __ballot(!live);
    if (lane < 16) p.eta[k] = en;
    if (lane == 0) {
        int rows = 0;
        for (int r = 0; r < 4; ++r) rows |= (int)((deadl >> (4 * r)) & 1ull) << r;
        const int iters = p.ctrl[AE_ITERS] + 1;
        p.ctrl[AE_ITERS] = iters;
        p.ctrl[AE_ROWS] |= rows;
        if (p.tol > 0.0 && d < p.tol) { p.ctrl[AE_CONV] = 1; p.ctrl[AE_STOP] = 1; }
        if (iters >= p.max_iter) p.ctrl[AE_STOP] = 1;
    }
}

// MODE 0: N, the saturated model, the uniform start row and zeroed step outputs; MODE 1: L at (gamma, eta).  Wavefront 0 computes, in the
// order of abund_kernel's passes; the other wavefronts of the workgroup help to stage the tiles.
template <int GP, int MODE>
__global__ __launch_bounds__(256) void abund_eta_eval_kernel(AbundEtaParams p)
{
    __shared__ int4 xS[DSM_ABUND_TILE];
    __shared__ uint64_t tS[DSM_ABUND_TILE];
    __shared__ double2 ltab[DSM_LOG_TAB_N];
    __shared__ double etaS[16];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int V = p.V, G = p.G, s = blockIdx.x;
    const int4 *cnt4 = reinterpret_cast<const int4 *>(p.cnt) + (size_t)s * V;
    for (int i = threadIdx.x; i < DSM_LOG_TAB_N; i += 256) ltab[i] = reinterpret_cast<const double2 *>(p.log_tab)[i];
    if (threadIdx.x < 16) etaS[threadIdx.x] = p.eta[threadIdx.x];
    double gam[GP], acc[GP];
#pragma unroll
    for (int g = 0; g < GP; ++g) { gam[g] = (MODE == 1 && g < G) ? p.gamma[(size_t)s * G + g] : 0.0; acc[g] = 0.0; }
    double o0 = 0.0, o1 = 0.0; bool bad = false;
    for (int t0 = 0; t0 < V; t0 += DSM_ABUND_TILE) {
        __syncthreads();
        const int n = min(DSM_ABUND_TILE, V - t0);
        for (int i = threadIdx.x; i < n; i += 256) { xS[i] = cnt4[t0 + i]; tS[i] = p.tau[t0 + i]; }
        __syncthreads();
        if (wave == 0) abund_rows<GP, MODE == 0 ? 0 : 2>(n, lane, xS, tS, etaS, ltab, gam, acc, o0, o1, bad);
    }
    if (wave != 0) return;
    o0 = group_allreduce_sum<64>(o0);
    if (MODE == 0) {
        o1 = group_allreduce_sum<64>(o1);
        if (lane == 0) { p.N[s] = o0; p.Lsat[s] = o1; p.delta[s] = 0.0; p.bad[s] = 0; }
        if (lane < 16) p.part[(size_t)s * 16 + lane] = 0.0;
        if (lane < G) p.gamma[(size_t)s * G + lane] = 1.0 / (double)G;
    } else if (lane == 0) p.ll[s] = o0;
}

static int g_abund_eta_batch = 0;            // dsm_abund_debug_set_eta_batch: steps enqueued between two reads of the stop word (0 = the default)
static size_t g_abund_eta_stage_max = 0;     // dsm_abund_debug_set_eta_stage_max: bound of the sample-major copy in bytes (0 = 1 GiB)
#define DSM_ABUND_ETA_BATCH 32               // 64 launches of a few microseconds per host read; a finished call idles through at most 31 steps

extern "C" int dsm_abund_debug_set_eta_batch(int steps)
{
    return dsm_set_knob(&g_abund_eta_batch, steps, "abund", "eta batch");
}

extern "C" int dsm_abund_debug_set_eta_stage_max(long long bytes)
{
    if (bytes < 0) { dsm_set_error("abund: eta stage bound %lld", bytes); return DSM_ERR_ARG; }
    g_abund_eta_stage_max = (size_t)bytes;
    return DSM_OK;
}

static int abund_eta_check(int V, int S, const double *eta0)
{
    for (int a = 0; a < 4; ++a) {
        const double sum = ((eta0[4 * a] + eta0[4 * a + 1]) + eta0[4 * a + 2]) + eta0[4 * a + 3];
        if (!(fabs(sum - 1.0) <= 1e-9)) { dsm_set_error("fit_gamma_eta: row %d of eta0 sums to %.17g", a, sum); return DSM_ERR_ARG; }
    }
    // every step reads every sample: the whole sample-major copy is staged at once (checked before anything is allocated)
    const size_t bound = g_abund_eta_stage_max ? g_abund_eta_stage_max : (size_t)1 << 30;
    if ((size_t)V * (size_t)S * 16 > bound) {
        dsm_set_error("fit_gamma_eta: V=%d x S=%d needs a %zu B copy of the counts, above the bound of %zu B", V, S, (size_t)V * (size_t)S * 16, bound);
        return DSM_ERR_UNSUPPORTED;
    }
    return DSM_OK;
}

template <int GP, int NW>
static void abund_eta_launch_step(const AbundEtaParams &q)
{
    hipLaunchKernelGGL((abund_eta_step_kernel<GP, NW>), dim3((unsigned)q.S), dim3(NW * 64u), 0, 0, q);
    hipLaunchKernelGGL(abund_eta_reduce_kernel, dim3(1), dim3(64), 0, 0, q);
}

template <int MODE>
static void abund_eta_launch_eval(const AbundEtaParams &q, int GP)
{
    switch (GP) {
    case 4: hipLaunchKernelGGL((abund_eta_eval_kernel<4, MODE>), dim3((unsigned)q.S), dim3(256), 0, 0, q); break;
    case 8: hipLaunchKernelGGL((abund_eta_eval_kernel<8, MODE>), dim3((unsigned)q.S), dim3(256), 0, 0, q); break;
    case 16: hipLaunchKernelGGL((abund_eta_eval_kernel<16, MODE>), dim3((unsigned)q.S), dim3(256), 0, 0, q); break;
    default: hipLaunchKernelGGL((abund_eta_eval_kernel<32, MODE>), dim3((unsigned)q.S), dim3(256), 0, 0, q); break;
    }
}

// as abund_run: d_cnt the resident tensor or null with h_cnt; d_tau the packed words on the device.  The arguments have been checked.
static int abund_eta_run(const int32_t *d_cnt, const int64_t *h_cnt, int V, int S, int G, const uint64_t *d_tau, const double *eta0,
                         int max_iter, double tol, double *gamma, double *eta, double *loglik, double *loglik0, double *deviance,
                         int32_t *iters, int32_t *converged, int32_t *dead_rows, double *lr_eta)
{
    // the reference fit: eta held at eta0, the path of dsm_fit_gamma itself
    {
        std::vector<double> g0((size_t)S * G), dev0((size_t)S);
        std::vector<int32_t> it0((size_t)S), cv0((size_t)S);
        DSM_TRY(abund_run(d_cnt, h_cnt, V, S, G, d_tau, eta0, max_iter, tol, 0, g0.data(), loglik0, dev0.data(), it0.data(), cv0.data(), nullptr));
    }
    const int GP = G <= 4 ? 4 : G <= 8 ? 8 : G <= 16 ? 16 : 32;
    DevBuf<int32_t> d_x, d_bad, d_ctrl; DevBuf<double> d_eta, d_ltab, d_gamma, d_N, d_Lsat, d_ll, d_part, d_delta;
    DSM_TRY(d_x.alloc((size_t)S * V * 4)); DSM_TRY(d_bad.alloc(S)); DSM_TRY(d_ctrl.alloc(AE_NCTRL)); DSM_TRY(d_eta.alloc(16));
    DSM_TRY(d_ltab.alloc(2 * DSM_LOG_TAB_N)); DSM_TRY(d_gamma.alloc((size_t)S * G)); DSM_TRY(d_N.alloc(S)); DSM_TRY(d_Lsat.alloc(S));
    DSM_TRY(d_ll.alloc(S)); DSM_TRY(d_part.alloc((size_t)S * 16)); DSM_TRY(d_delta.alloc(S));
    HIP_TRY(hipMemcpy(d_eta, eta0, 16 * sizeof(double), hipMemcpyHostToDevice));
    DSM_TRY(dsm_upload_log_table(d_ltab));
    int32_t ctrl[AE_NCTRL] = {0};
    ctrl[AE_STOP] = max_iter == 0 ? 1 : 0;
    HIP_TRY(hipMemcpy(d_ctrl, ctrl, sizeof ctrl, hipMemcpyHostToDevice));
    std::vector<int32_t> x32;
    for (int s0 = 0; s0 < S; s0 += 1 << 15) {              // (the repack kernel's grid holds 65535 samples at the most)
        const int n = std::min(1 << 15, S - s0);
        DSM_TRY(abund_stage_chunk(d_cnt, h_cnt, V, S, s0, n, d_x.p + (size_t)s0 * V * 4, x32));
    }
    std::vector<int32_t>().swap(x32);
    AbundEtaParams q{d_x, d_tau, d_ltab, V, G, S, max_iter, tol, d_gamma, d_eta, d_N, d_Lsat, d_ll, d_part, d_delta, d_bad, d_ctrl};
    abund_eta_launch_eval<0>(q, GP);
    HIP_TRY(hipGetLastError());
    const int batch = g_abund_eta_batch > 0 ? g_abund_eta_batch : DSM_ABUND_ETA_BATCH;
    while (ctrl[AE_STOP] == 0) {
        for (int i = 0; i < batch; ++i)
            switch (GP) {                                  // wavefronts per workgroup by the registers a lane needs
            case 4: abund_eta_launch_step<4, 8>(q); break;
            case 8: abund_eta_launch_step<8, 8>(q); break;
            case 16: abund_eta_launch_step<16, 8>(q); break;
            default: abund_eta_launch_step<32, 4>(q); break;
            }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(ctrl, d_ctrl, sizeof ctrl, hipMemcpyDeviceToHost));
    }
    abund_eta_launch_eval<1>(q, GP);
    HIP_TRY(hipGetLastError());
    std::vector<double> Lsat((size_t)S);
    HIP_TRY(hipMemcpy(gamma, d_gamma, (size_t)S * G * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(eta, d_eta, 16 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(loglik, d_ll, (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(Lsat.data(), d_Lsat, (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    bool dead = ctrl[AE_DEAD] != 0;
    for (int s = 0; s < S; ++s) dead = dead || !(loglik[s] > -INFINITY);       // (the final pass: max_iter = 0 on a table eta0 contradicts)
    *iters = ctrl[AE_ITERS];
    *dead_rows = ctrl[AE_ROWS];
    if (dead) {
        for (size_t i = 0; i < (size_t)S * G; ++i) gamma[i] = 0.0;
        for (int s = 0; s < S; ++s) { loglik[s] = -INFINITY; deviance[s] = INFINITY; }
        memcpy(eta, eta0, 16 * sizeof(double));
        *converged = 0;
        *lr_eta = NAN;
        return DSM_OK;
    }
    *converged = ctrl[AE_CONV];
    double L = 0.0, L0 = 0.0;
    for (int s = 0; s < S; ++s) { deviance[s] = 2.0 * (Lsat[s] - loglik[s]); L += loglik[s]; L0 += loglik0[s]; }
    const double lr = 2.0 * (L - L0);
    *lr_eta = lr < 0.0 ? 0.0 : lr;                         // (eta0 is in the model: rounding, or a joint fit that max_iter ended early)
    return DSM_OK;
}

extern "C" int dsm_fit_gamma_eta(int device, const int64_t *counts, int V, int S, int G, const int64_t *tau, const double *eta0,
                                 int max_iter, double tol, double *gamma, double *eta, double *loglik, double *loglik0, double *deviance,
                                 int32_t *iters, int32_t *converged, int32_t *dead_rows, double *lr_eta)
{
    if (S < 1 || !counts || !tau || !eta0 || !gamma || !eta || !loglik || !loglik0 || !deviance || !iters || !converged || !dead_rows || !lr_eta) {
        dsm_set_error("fit_gamma_eta: bad arguments");
        return DSM_ERR_ARG;
    }
    DSM_TRY(abund_check_model(V, G, eta0, max_iter, tol));
    DSM_TRY(abund_eta_check(V, S, eta0));
    DSM_TRY(dsm_check_counts("fit_gamma", counts, (size_t)V, S));
    std::vector<uint64_t> words;
    DSM_TRY(abund_tau_words("fit_gamma_eta", nullptr, tau, V, G, words));
    DSM_TRY(dsm_bind_device(device));
    DevBuf<uint64_t> own;
    const uint64_t *d_tau = nullptr;
    DSM_TRY(abund_tau_on_device(nullptr, words, own, &d_tau));
    return abund_eta_run(nullptr, counts, V, S, G, d_tau, eta0, max_iter, tol, gamma, eta, loglik, loglik0, deviance, iters, converged,
                         dead_rows, lr_eta);
}

extern "C" int dsm_ctx_fit_gamma_eta(dsm_ctx *c, int G, const int64_t *tau, const double *eta0, int max_iter, double tol, double *gamma,
                                     double *eta, double *loglik, double *loglik0, double *deviance, int32_t *iters, int32_t *converged,
                                     int32_t *dead_rows, double *lr_eta)
{
    DSM_TRY(dsm_ctx_enter(c, true));
    if (!eta0 || !gamma || !eta || !loglik || !loglik0 || !deviance || !iters || !converged || !dead_rows || !lr_eta) {
        dsm_set_error("ctx_fit_gamma_eta: null pointer");
        return DSM_ERR_ARG;
    }
    DSM_TRY(abund_check_model(c->V, G, eta0, max_iter, tol));
    DSM_TRY(abund_eta_check(c->V, c->S, eta0));
    std::vector<uint64_t> words;
    DSM_TRY(abund_tau_words("ctx_fit_gamma_eta", c, tau, c->V, G, words));
    DevBuf<uint64_t> own;
    const uint64_t *d_tau = nullptr;
    DSM_TRY(abund_tau_on_device(c, words, own, &d_tau));
    return abund_eta_run(c->cnt_vs, nullptr, c->V, c->S, G, d_tau, eta0, max_iter, tol, gamma, eta, loglik, loglik0,
                         deviance, iters, converged, dead_rows, lr_eta);
}
