// kernels_ppc.hip -- gfx950 kernels for the posterior predictive p-values of a chain per sample and per position, from replicate tables
// drawn at the stored iterations (api_trace.hip: dsm_ctx_trace_ppc; desman_amd/check.py; the definition stands in
// include/desman_hip.h above the call).
//
//   trace_ppc_kernel<NSL>     per used iteration t of the launch: p_b (dsm_fit_cell.h, shared with trace_fit_kernel), X_obs and the
//                             read-by-read thresholds of every cell once; then per replicate r the cell's draw fused with X_rep, the
//                             position's T_rep over the lane group (compared with T_obs and accumulated in the kernel) and the tile's
//                             share of every sample's T_rep, written to [tile][t][r][s]
//   ppc_merge_tiles_kernel    the tiles' shares, added in ascending order
//   ppc_sample_acc_kernel     per sample: T_rep against T_obs(t), the counts and sums over (t, r) of the launch
//   ppc_pos_acc_kernel        per position: the iterations' sums, added in ascending order
//
// Plain fp64, no floating-point atomics (the counts of the positions are integer atomics).  Every exclusion is a select, never a product
// with 0.  Nothing of the chain is written.
#include <algorithm>
#include <math.h>

#include "dsm_trace_host.h"
#include "dsm_fit_cell.h"
#include "dsm_binom.h"

#define PPC_BLOCKS 2048                     // workgroups a launch aims at (256 compute units x 8)
#define PPC_LDS_GAMMA 4096                  // as FIT_LDS_GAMMA (kernels_fit.hip): fit_plan cuts gamma into chunks of that many doubles
#define PPC_CELL_WORDS 6                    // doubles of LDS per cell: p_0 .. p_3, then (th_0, th_1) and (th_2, N) as 32-bit words

struct PpcParams {
    const int32_t *cnt;         // [V][S][4]
    const uint64_t *trace;      // row of iteration it0
    size_t trace_stride;        // words between two iterations' rows (0: one row for all)
    const double *gamma, *eta;  // rows of iteration it0: [..][S][G], [..][16]
    const double *log_tab;
    int V, S, G;
    int lpv_log2, gc;           // log2 of the lanes per position; haplotypes per staged chunk of gamma
    int it0, stride;            // used iteration k is the stored iteration it0 + k stride
    int k0, nk;                 // the used iterations of this launch: k0 .. k0 + nk - 1
    int r0, nr, R;              // its replicates: r0 .. r0 + nr - 1 of R (nr < R: nk = 1)
    uint32_t key0, key1;
    double *samp_part;          // [tiles][nk][nr][S]  the tile's share of T_s^rep
    double *obs_part;           // [tiles][nk][S]      ... of T_s^obs
    double *pos_it;             // [nk][V][3]          sum_r T_v^rep, sum_r (T_v^rep)^2 (carried from launch to launch of one iteration), T_v^obs
    unsigned long long *ge_pos; // [V]
};

// Pearson's X of a cell with N > 0 reads against p, the formula of trace_fit_kernel term for term
__device__ __forceinline__ double ppc_pearson(int Ni, const double (&pb)[4], const uint32_t (&n)[4])
{
    const double N = (double)Ni;
    double x = 0.0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const double nb = (double)n[b];
        const bool pos = pb[b] > 0.0, seen = n[b] > 0u;
        const double e = N * pb[b], dl = nb - e;
        x += pos ? dl * dl / e : (seen ? INFINITY : 0.0);
    }
    return x;
}

// over the slots of a lane the caller has added in order; here over the lanes of the group by halving (xor offsets below LPV stay inside it)
__device__ __forceinline__ double ppc_group_sum(double q, int LPV)
{
    for (int off = LPV >> 1; off > 0; off >>= 1) q += __shfl_xor(q, off);
    return q;
}

// The tiling of trace_fit_kernel: LPV = 2^lpv_log2 lanes per position, NSL sample slots per lane (slot j of lane l = sample l + j LPV),
// 256 / LPV positions per workgroup, one workgroup per tile of positions and part of the launch's iterations (blockIdx.z; part z owns the
// iterations z pi .. min(nk, (z + 1) pi) - 1 of the launch, pi = ceil(nk / parts)).  LDS: the region gamma_t and eta_t are staged in, which
// the reductions over the positions of the tile reuse ([group][slot]); the logarithm's table and 1/k for the binomial sampler, staged once
// per workgroup; and PPC_CELL_WORDS doubles per cell ([slot][word][thread]: no bank conflicts), written once per iteration, from which
// the replicate loop -- one binomial site, `#pragma unroll 1` over the slots -- reads its cell.  A cell's registers in that loop are those
// of one cell whatever NSL is.
template <int NSL>
__global__ __launch_bounds__(256) void trace_ppc_kernel(const PpcParams p)
{
    extern __shared__ double lds[];
    const int LPV = 1 << p.lpv_log2, SP = LPV * NSL, PPB = 256 >> p.lpv_log2;
    const int tid = threadIdx.x, l = tid & (LPV - 1), grp = tid >> p.lpv_log2;
    const int V = p.V, S = p.S, G = p.G, gc = p.gc;
    const long long v = (long long)blockIdx.x * PPB + grp;
    const bool vin = v < V;
    const int a_len = (max(gc * SP + 16, 256 * NSL) + 1) & ~1;
    double *const lgam = lds, *const leta = lds + (size_t)gc * SP, *const red = lds;
    double2 *const ltab = reinterpret_cast<double2 *>(lds + a_len);                  // [DSM_LOG_TAB_N]
    double *const rcp = lds + a_len + 2 * DSM_LOG_TAB_N;                             // [DSM_RCP_TAB_N]
    double *const cell = rcp + DSM_RCP_TAB_N;                                        // [NSL][PPC_CELL_WORDS][256]

    if (tid < DSM_LOG_TAB_N) ltab[tid] = reinterpret_cast<const double2 *>(p.log_tab)[tid];
    for (int k = tid; k < DSM_RCP_TAB_N; k += 256) rcp[k] = k ? 1.0 / (double)k : 0.0;

    int c0[NSL], c1[NSL], c2[NSL], c3[NSL];
#pragma unroll
    for (int j = 0; j < NSL; ++j) {
        const int s = l + j * LPV;
        int4 c = make_int4(0, 0, 0, 0);
        if (vin && s < S) c = *reinterpret_cast<const int4 *>(p.cnt + ((size_t)v * S + s) * 4);
        c0[j] = c.x; c1[j] = c.y; c2[j] = c.z; c3[j] = c.w;
    }

    const int parts = (int)gridDim.z, pi = (p.nk + parts - 1) / parts;
    const int ka = min(p.nk, (int)blockIdx.z * pi), kb = min(p.nk, ka + pi);
    const size_t sg = (size_t)S * G;
    for (int kk = ka; kk < kb; ++kk) {
        const size_t tr = (size_t)(p.k0 + kk) * (size_t)p.stride;                    // rows past iteration it0
        const uint32_t t = (uint32_t)p.it0 + (uint32_t)tr;                           // the stored iteration's own number
        const uint64_t word = vin ? p.trace[tr * p.trace_stride + (size_t)v] : 0ull;
        double m0[NSL], m1[NSL], m2[NSL], m3[NSL];
        fit_cell_mixture<NSL>(p.gamma + tr * sg, p.eta + tr * 16, word, S, G, gc, p.lpv_log2, lgam, leta, m0, m1, m2, m3);

        // ---- per cell, once per iteration: p, X_obs, the thresholds of the read-by-read path
        double xo[NSL], qo = 0.0;
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            double pb[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) pb[b] = fit_cell_p(m0[j], m1[j], m2[j], m3[j], leta, b);
            const uint32_t n[4] = {(uint32_t)c0[j], (uint32_t)c1[j], (uint32_t)c2[j], (uint32_t)c3[j]};
            const int Ni = c0[j] + c1[j] + c2[j] + c3[j];
            const double x = ppc_pearson(Ni, pb, n);
            xo[j] = Ni > 0 ? x : 0.0;
            qo += xo[j];
            // draw_reads' rule (dsm_binom.h): running sums in ascending order, one scale, floor with saturation
            const double cum0 = 0.0 + pb[0], cum1 = cum0 + pb[1], cum2 = cum1 + pb[2], cum3 = cum2 + pb[3];
            const double scale = 4294967296.0 / cum3;
            const uint32_t th0 = cvt_sat_u32(cum0 * scale), th1 = cvt_sat_u32(cum1 * scale), th2 = cvt_sat_u32(cum2 * scale);
            double *cw = cell + (size_t)j * PPC_CELL_WORDS * 256 + tid;
            cw[0] = pb[0]; cw[256] = pb[1]; cw[512] = pb[2]; cw[768] = pb[3];
            cw[1024] = __hiloint2double((int)th1, (int)th0);
            cw[1280] = __hiloint2double(cum3 > 0.0 ? Ni : 0, (int)th2);              // a cell no base can be drawn for is skipped like an empty one
        }
        __syncthreads();                                                             // gamma and eta have been read by everyone
#pragma unroll
        for (int j = 0; j < NSL; ++j) red[grp * SP + l + j * LPV] = xo[j];
        __syncthreads();
        for (int s = tid; s < S; s += 256) {
            double a = 0.0;
            for (int g = 0; g < PPB; ++g) a += red[g * SP + s];
            p.obs_part[((size_t)blockIdx.x * p.nk + kk) * S + s] = a;
        }
        const double tobs = ppc_group_sum(qo, LPV);

        // ---- the replicates
        double sumT = 0.0, sumT2 = 0.0;
        unsigned long long ge = 0ull;
        double *const pit = p.pos_it + ((size_t)kk * V + (size_t)(vin ? v : 0)) * 3;
        if (p.r0 > 0 && vin && l == 0) { sumT = pit[0]; sumT2 = pit[1]; }
        for (int rr = 0; rr < p.nr; ++rr) {
            const uint32_t ctr = t * (uint32_t)DSM_PPC_MAX_R + (uint32_t)(p.r0 + rr);
            __syncthreads();                                                         // the readers of the previous reduction are done
            double qr = 0.0;
#pragma unroll 1
            for (int j = 0; j < NSL; ++j) {
                const double *cw = cell + (size_t)j * PPC_CELL_WORDS * 256 + tid;
                const double w4 = cw[1024], w5 = cw[1280];
                const int Ni = __double2hiint(w5);
                double xr = 0.0;
                if (Ni > 0) {
                    const double pb[4] = {cw[0], cw[256], cw[512], cw[768]};
                    const unsigned long long ci = (unsigned long long)v * (unsigned long long)S + (unsigned long long)(l + j * LPV);
                    Xo128 rng = xo_seed((uint32_t)ci, (uint32_t)(ci >> 32), ctr, DSM_STREAM_PPCR, p.key0, p.key1);
                    uint32_t n[4];
                    if (Ni <= DSM_PPC_READS) {
                        const uint32_t th0 = (uint32_t)__double2loint(w4), th1 = (uint32_t)__double2hiint(w4), th2 = (uint32_t)__double2loint(w5);
                        uint32_t k0 = 0, k1 = 0, k2 = 0;
                        for (int i = 0; i < Ni; ++i) {
                            const uint32_t w = rng.next();
                            k0 += w < th0 ? 1u : 0u; k1 += w < th1 ? 1u : 0u; k2 += w < th2 ? 1u : 0u;
                        }
                        // the last base with p > 0 takes the remainder: it and every base after it hold all N reads in the running counts
                        const int last = pb[3] > 0.0 ? 3 : (pb[2] > 0.0 ? 2 : (pb[1] > 0.0 ? 1 : 0));
                        k0 = last <= 0 ? (uint32_t)Ni : k0; k1 = last <= 1 ? (uint32_t)Ni : k1; k2 = last <= 2 ? (uint32_t)Ni : k2;
                        n[0] = k0; n[1] = k1 - k0; n[2] = k2 - k1; n[3] = (uint32_t)Ni - k2;
                    } else {
                        const double tail2 = pb[3], tail1 = pb[2] + tail2, tail0 = pb[1] + tail1;
                        uint32_t rem = (uint32_t)Ni, kq[3] = {0u, 0u, 0u};
                        bool defer = false;
#pragma unroll 1
                        for (int b = 0; b < 3; ++b) {                                // ONE binomial site (the sampler is a large piece of code)
                            const double wa = b == 0 ? pb[0] : (b == 1 ? pb[1] : pb[2]), wb = b == 0 ? tail0 : (b == 1 ? tail1 : tail2);
                            const uint32_t kx = binom<true, 2>(rng, rem, wa, wb, rcp, ltab, defer);    // wa = 0: 0; wb = 0: all that is left
                            kq[0] = b == 0 ? kx : kq[0]; kq[1] = b == 1 ? kx : kq[1]; kq[2] = b == 2 ? kx : kq[2];
                            rem -= kx;
                        }
                        n[0] = kq[0]; n[1] = kq[1]; n[2] = kq[2]; n[3] = rem;
                    }
                    xr = ppc_pearson(Ni, pb, n);
                }
                red[grp * SP + l + j * LPV] = xr;
                qr += xr;
            }
            __syncthreads();
            for (int s = tid; s < S; s += 256) {
                double a = 0.0;
                for (int g = 0; g < PPB; ++g) a += red[g * SP + s];
                p.samp_part[(((size_t)blockIdx.x * p.nk + kk) * p.nr + rr) * S + s] = a;
            }
            const double trep = ppc_group_sum(qr, LPV);
            ge += trep >= tobs ? 1ull : 0ull;
            sumT += trep;
            sumT2 += trep * trep;
        }
        if (vin && l == 0) {
            pit[0] = sumT; pit[1] = sumT2; pit[2] = tobs;
            if (ge) atomicAdd(p.ge_pos + v, ge);
        }
    }
}

// out[i] = sum over the tiles, in ascending order from 0, of part[tile][i]
__global__ __launch_bounds__(256) void ppc_merge_tiles_kernel(const double *__restrict__ part, size_t len, int tiles, double *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    double a = 0.0;
    for (int z = 0; z < tiles; ++z) a += part[(size_t)z * len + i];
    out[i] = a;
}

// One thread per sample: T_rep [nk][nr][S] against T_obs [nk][S]; the sums over r are nested inside the iteration (carried in `carry`
// [S][2] from launch to launch where one iteration's replicates take several launches), the iteration's sums join the totals with its last
// replicate
__global__ __launch_bounds__(256) void ppc_sample_acc_kernel(const double *__restrict__ trep, const double *__restrict__ tobs, int S, int nk,
                                                             int nr, int first, int last, double *carry, unsigned long long *ge,
                                                             double *rep, double *obs)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    unsigned long long n = ge[s];
    double r0 = rep[2 * s], r1 = rep[2 * s + 1], o = obs[s];
    for (int k = 0; k < nk; ++k) {
        const double to = tobs[(size_t)k * S + s];
        double a = first ? 0.0 : carry[2 * s], b = first ? 0.0 : carry[2 * s + 1];
        for (int r = 0; r < nr; ++r) {
            const double t = trep[((size_t)k * nr + r) * S + s];
            n += t >= to ? 1ull : 0ull;
            a += t;
            b += t * t;
        }
        if (last) { r0 += a; r1 += b; o += to; }
        else { carry[2 * s] = a; carry[2 * s + 1] = b; }
    }
    ge[s] = n; rep[2 * s] = r0; rep[2 * s + 1] = r1; obs[s] = o;
}

// One thread per position: the finished iterations of a launch, pos_it [nk][V][3], join the totals in ascending order
__global__ __launch_bounds__(256) void ppc_pos_acc_kernel(const double *__restrict__ pos_it, int V, int nk, double *rep, double *obs)
{
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= (size_t)V) return;
    double r0 = rep[2 * v], r1 = rep[2 * v + 1], o = obs[v];
    for (int k = 0; k < nk; ++k) {
        const double *q = pos_it + ((size_t)k * V + v) * 3;
        r0 += q[0]; r1 += q[1]; o += q[2];
    }
    rep[2 * v] = r0; rep[2 * v + 1] = r1; obs[v] = o;
}

static int g_ppc_parts = 0;       // dsm_ppc_debug_set_parts: iteration parts per launch (0 = by the grid the launch aims at)
static int g_ppc_ct = 0;          // dsm_ppc_debug_set_chunk: iterations / replicates per launch (0 = by the scratch bound)
static int g_ppc_cr = 0;

extern "C" int dsm_ppc_debug_set_parts(int parts)
{
    return dsm_set_knob(&g_ppc_parts, parts, "ppc", "parts");
}

extern "C" int dsm_ppc_debug_set_chunk(int iterations, int replicates)
{
    DSM_TRY(dsm_set_knob(&g_ppc_ct, iterations, "ppc", "iterations per launch"));
    return dsm_set_knob(&g_ppc_cr, replicates, "ppc", "replicates per launch");
}

static size_t ppc_lds_bytes(int nsl, int lpv, int gc)
{
    const size_t a_len = (std::max((size_t)gc * lpv * nsl + 16, (size_t)256 * nsl) + 1) & ~(size_t)1;
    return (a_len + 2 * DSM_LOG_TAB_N + DSM_RCP_TAB_N + (size_t)nsl * PPC_CELL_WORDS * 256) * sizeof(double);
}

// the tile and the gamma chunk (fit_plan's), the chunks and the grid of the launches over n_used iterations and R replicates; nothing is
// launched.  The per-tile sample sums of a launch, tiles x iterations x replicates x S doubles, stay within DSM_PPC_SCRATCH_MB: as many whole
// iterations as fit, or -- where one iteration alone does not -- one iteration and as many of its replicates as do.
int ppc_plan(const dsm_ctx *c, int n_used, int R, PpcPlan *pl)
{
    FitPlan fp;
    DSM_TRY(fit_plan(c, n_used, &fp));
    pl->nsl = fp.nsl; pl->lpv = fp.lpv; pl->gc = fp.gc; pl->tiles = fp.tiles;
    pl->lds = ppc_lds_bytes(fp.nsl, fp.lpv, fp.gc);
    const size_t bound = (size_t)DSM_PPC_SCRATCH_MB << 20, per_rep = (size_t)fp.tiles * c->S * sizeof(double);
    if (per_rep > bound) { dsm_set_error("ppc: V=%d positions are too many for the scratch bound of %d MiB", c->V, DSM_PPC_SCRATCH_MB); return DSM_ERR_UNSUPPORTED; }
    long long ct = (long long)(bound / (per_rep * R)), cr = R;
    if (ct < 1) { ct = 1; cr = (long long)(bound / per_rep); }
    if (g_ppc_ct > 0) ct = g_ppc_ct;
    if (g_ppc_cr > 0) cr = g_ppc_cr;
    pl->cr = (int)std::max(1LL, std::min<long long>(cr, R));
    pl->ct = pl->cr < R ? 1 : (int)std::max(1LL, std::min<long long>(ct, n_used));
    const int parts = g_ppc_parts > 0 ? g_ppc_parts : (PPC_BLOCKS + fp.tiles - 1) / fp.tiles;
    pl->parts = std::max(1, std::min({parts, pl->ct, 65535}));
    return DSM_OK;
}

template <int NSL>
static int ppc_launch(dsm_ctx *c, const PpcPlan &pl, int parts, const PpcParams &p)
{
    DSM_TRY(dsm_allow_lds(reinterpret_cast<const void *>(&trace_ppc_kernel<NSL>), pl.lds, "ppc"));
    hipLaunchKernelGGL((trace_ppc_kernel<NSL>), dim3((unsigned)pl.tiles, 1, (unsigned)parts), dim3(256), pl.lds, c->stream, p);
    return DSM_OK;
}

// n_used >= 1; the six outputs are device buffers, zero on entry
int k_trace_ppc(dsm_ctx *c, const PpcPlan &pl, const TraceView &tr, int it0, int stride, int n_used, int R, uint32_t key0, uint32_t key1,
                unsigned long long *d_ge_s, unsigned long long *d_ge_v, double *d_rep_s, double *d_rep_v, double *d_obs_s, double *d_obs_v)
{
    const size_t V = (size_t)c->V, S = (size_t)c->S;
    DevBuf<double> samp_part, obs_part, pos_it, trep, tobs, carry;
    DSM_TRY(samp_part.alloc((size_t)pl.tiles * pl.ct * pl.cr * S));
    DSM_TRY(obs_part.alloc((size_t)pl.tiles * pl.ct * S));
    DSM_TRY(pos_it.alloc((size_t)pl.ct * V * 3));
    DSM_TRY(trep.alloc((size_t)pl.ct * pl.cr * S));
    DSM_TRY(tobs.alloc((size_t)pl.ct * S));
    DSM_TRY(carry.alloc(S * 2));
    PpcParams p;
    p.cnt = c->cnt_vs; p.trace = tr.tau; p.trace_stride = tr.tau_stride; p.gamma = tr.gamma; p.eta = tr.eta; p.log_tab = c->log_tab;
    p.V = c->V; p.S = c->S; p.G = c->G; p.gc = pl.gc;
    p.lpv_log2 = 0;
    while ((1 << p.lpv_log2) < pl.lpv) ++p.lpv_log2;
    p.it0 = it0; p.stride = stride; p.R = R; p.key0 = key0; p.key1 = key1;
    p.samp_part = samp_part; p.obs_part = obs_part; p.pos_it = pos_it; p.ge_pos = d_ge_v;
    for (int k0 = 0; k0 < n_used; k0 += pl.ct) {
        p.k0 = k0; p.nk = std::min(pl.ct, n_used - k0);
        const int parts = std::min(pl.parts, p.nk);
        for (int r0 = 0; r0 < R; r0 += pl.cr) {
            p.r0 = r0; p.nr = std::min(pl.cr, R - r0);
            const int last = r0 + p.nr == R;
            switch (pl.nsl) {
            case 1: DSM_TRY(ppc_launch<1>(c, pl, parts, p)); break;
            case 2: DSM_TRY(ppc_launch<2>(c, pl, parts, p)); break;
            case 4: DSM_TRY(ppc_launch<4>(c, pl, parts, p)); break;
            default: DSM_TRY(ppc_launch<8>(c, pl, parts, p)); break;
            }
            HIP_TRY(hipGetLastError());
            const size_t nrep = (size_t)p.nk * p.nr * S, nobs = (size_t)p.nk * S;
            hipLaunchKernelGGL(ppc_merge_tiles_kernel, dim3((unsigned)((nrep + 255) / 256)), dim3(256), 0, c->stream, samp_part.p, nrep, pl.tiles,
                               trep.p);
            hipLaunchKernelGGL(ppc_merge_tiles_kernel, dim3((unsigned)((nobs + 255) / 256)), dim3(256), 0, c->stream, obs_part.p, nobs, pl.tiles,
                               tobs.p);
            hipLaunchKernelGGL(ppc_sample_acc_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, c->stream, trep.p, tobs.p, (int)S, p.nk, p.nr,
                               (int)(r0 == 0), last, carry.p, d_ge_s, d_rep_s, d_obs_s);
            if (last)
                hipLaunchKernelGGL(ppc_pos_acc_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, c->stream, pos_it.p, (int)V, p.nk, d_rep_v,
                                   d_obs_v);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));          // the scratch buffers are freed on return
    return DSM_OK;
}
