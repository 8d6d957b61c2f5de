// kernels_relabel.hip -- gfx950 kernels that reduce the resident tau trace (dsm_ctx::tau_trace, one packed word per position and stored
// iteration, 2 bits per haplotype) to what label-switch-aware summaries need (api_trace.hip: dsm_ctx_trace_snd, dsm_ctx_get_tau_sum_perm;
// desman_amd/relabel.py).
//
//   trace_snd_kernel      snd[t][g][h] = #{v : tau_t[v][g] != ref_t[v][h]}, ref = one fixed word table or tau_t itself
//   tau_sum_perm_kernel   tau_sum[v][perm_t[g]][a] += [tau_t[v][g] = a]
//
// Both read the trace once per pass over it, produce integers and add them with vector integer atomics: the results are the same bits
// for any grid and any order.
#include <algorithm>

#include "dsm_trace_host.h"

#define RL_HT 8                 // reference haplotypes per tile: their counts of one 64-position step live in scalar registers
#define RL_BLOCKS 2048          // workgroups a launch aims at (256 compute units x 8)

// One wavefront per 64 positions, its lanes over the positions: the trace word and the reference word are one coalesced 8 B load each.
// Lanes past V hold the word 0 on both sides, so they differ nowhere.  For a tile of RL_HT reference haplotypes the digits are taken out
// of the reference word once; then per haplotype g of the trace word one compare per pair, whose 64-bit lane mask (v_cmp -> SGPR pair)
// is counted by the scalar unit; the tile's counts are placed into lanes 0 .. RL_HT-1 (v_cndmask) and added to the workgroup's table
// in LDS with one ds_add.  Nothing diverges: the step loop is per wavefront, the haplotype loops are uniform.  The table goes to the
// output with global integer atomics at the end.  grid = (position chunks, iterations); trace_stride = 0: every iteration reads the
// same row (a fixed-tau trace).
__global__ __launch_bounds__(256) void trace_snd_kernel(const uint64_t *__restrict__ trace, size_t trace_stride,
                                                        const uint64_t *__restrict__ ref, int V, int G, int Gr, int *__restrict__ out)
{
    __shared__ int acc[DSM_MAX_G * DSM_MAX_G];
    const int npair = G * Gr;
    for (int i = threadIdx.x; i < npair; i += 256) acc[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t *tw = trace + (size_t)blockIdx.y * trace_stride;
    const int nstep = (V + 63) >> 6;
    for (int s = blockIdx.x * 4 + wave; s < nstep; s += gridDim.x * 4) {
        const int v = s * 64 + lane;
        uint64_t w = 0, r = 0;
        if (v < V) {
            w = tw[v];
            r = ref ? ref[v] : w;
        }
        for (int h0 = 0; h0 < Gr; h0 += RL_HT) {
            int dh[RL_HT];
#pragma unroll
            for (int j = 0; j < RL_HT; ++j) dh[j] = (int)(r >> (2 * min(h0 + j, DSM_MAX_G - 1))) & 3;     // (h >= Gr: counted, never added)
            for (int g = 0; g < G; ++g) {
                const int dg = (int)(w >> (2 * g)) & 3;
                int mine = 0;
#pragma unroll
                for (int j = 0; j < RL_HT; ++j) {
                    const int cnt = __popcll(__ballot(dg != dh[j]));
                    mine = lane == j ? cnt : mine;
                }
                if (lane < RL_HT && h0 + lane < Gr && mine) atomicAdd(&acc[g * Gr + h0 + lane], mine);
            }
        }
    }
    __syncthreads();
    int *o = out + (size_t)blockIdx.y * npair;
    for (int i = threadIdx.x; i < npair; i += 256) {
        const int a = acc[i];
        if (a) atomicAdd(o + i, a);
    }
}

// One thread per (position, output label); blockIdx.y = the output label, so the iteration's source haplotype inv[t][label] (the
// inverse of the caller's permutation, made by the host) is one uniform byte per iteration and the digit is one shift of the trace
// word.  Four named counters, compared against constants as tau_sum_kernel does: nothing is indexed at run time.  blockIdx.z splits
// the iterations; the parts meet in 64-bit integer atomics on the zeroed output.
__global__ __launch_bounds__(256) void tau_sum_perm_kernel(const uint64_t *__restrict__ trace, size_t trace_stride,
                                                           const uint8_t *__restrict__ inv, int n, int V, int G,
                                                           unsigned long long *__restrict__ out)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int label = blockIdx.y;
    if (v >= V) return;
    const int per = (n + (int)gridDim.z - 1) / (int)gridDim.z;
    const int t0 = (int)blockIdx.z * per, t1 = min(n, t0 + per);
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int t = t0; t < t1; ++t) {
        const int sh = 2 * (int)inv[(size_t)t * G + label];
        const int d = (int)(trace[(size_t)t * trace_stride + v] >> sh) & 3;
        c0 += (d == 0); c1 += (d == 1); c2 += (d == 2); c3 += (d == 3);
    }
    unsigned long long *p = out + ((size_t)v * G + label) * 4;
    if (c0) atomicAdd(p + 0, (unsigned long long)c0);
    if (c1) atomicAdd(p + 1, (unsigned long long)c1);
    if (c2) atomicAdd(p + 2, (unsigned long long)c2);
    if (c3) atomicAdd(p + 3, (unsigned long long)c3);
}

// d_out [n_it][G][Gr] int32, zeroed here.  ref = nullptr: every iteration against itself.
int k_trace_snd(dsm_ctx *c, const TraceView &tr, const uint64_t *ref, int Gr, int n_it, int *d_out)
{
    if (n_it < 1) return DSM_OK;
    const int V = c->V, G = c->G;
    const size_t npair = (size_t)G * Gr;
    HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)n_it * npair * sizeof(int), c->stream));
    const int nstep = (V + 63) / 64;
    for (int t0 = 0; t0 < n_it; t0 += 65535) {                     // gridDim.y
        const int nt = std::min(n_it - t0, 65535);
        const int gx = std::max(1, std::min((RL_BLOCKS + nt - 1) / nt, (nstep + 3) / 4));
        hipLaunchKernelGGL(trace_snd_kernel, dim3((unsigned)gx, (unsigned)nt), dim3(256), 0, c->stream, tr.tau + (size_t)t0 * tr.tau_stride,
                           tr.tau_stride, ref, V, G, Gr, d_out + (size_t)t0 * npair);
        HIP_TRY(hipGetLastError());
    }
    return DSM_OK;
}

// d_out [V][G][4] int64, zeroed here; d_inv [n][G]: inv[t][perm[t][g]] = g.
int k_tau_sum_perm(dsm_ctx *c, const TraceView &tr, const uint8_t *d_inv, int n, int64_t *d_out)
{
    const int V = c->V, G = c->G;
    HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)V * G * 4 * sizeof(int64_t), c->stream));
    if (n < 1) return DSM_OK;
    const int gx = (V + 255) / 256;
    const int gz = std::max(1, std::min({(RL_BLOCKS + gx * G - 1) / (gx * G), (n + 31) / 32, 1024}));
    hipLaunchKernelGGL(tau_sum_perm_kernel, dim3((unsigned)gx, (unsigned)G, (unsigned)gz), dim3(256), 0, c->stream, tr.tau, tr.tau_stride,
                       d_inv, n, V, G, reinterpret_cast<unsigned long long *>(d_out));
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}
