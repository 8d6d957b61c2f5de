// kernels_diag.hip -- gfx950 kernel that reduces the resident tau trace to what batch-means convergence diagnostics need, as exact
// integers (api_trace.hip: dsm_ctx_trace_batch_stats; desman_amd/diagnose.py).
//
//   trace_batch_stats_kernel   with x_t[v][l][a] = [the haplotype carrying label l in iteration t has base a at v], over B batches of
//                              L consecutive iterations:  sum = sum_t x_t,  first = the same over batches 0 .. B/2 - 1,
//                              bsq = sum_b (sum_{t in b} x_t)^2,  flips[v][l] = #{t > 0 : label l's base at v differs from that at t - 1}
//
// Integer arithmetic only; the parts of the iteration range meet in vector integer atomics on zeroed outputs: the results are the same
// bits for any grid and any split of the iterations.
#include <algorithm>

#include "dsm_trace_host.h"

#define DG_BLOCKS 2048          // workgroups a launch aims at (256 compute units x 8)

// The mapping of tau_sum_perm_kernel (kernels_relabel.hip): one thread per (position, output label), blockIdx.y = the label, so the
// iteration's source haplotype inv[t][label] is one uniform byte and the digit is one shift of the trace word.  Per thread: four
// counters of the running batch, four sums, four sums over the first half, four sums of squares, the previous digit and the flips --
// all named and compared against constants, nothing is indexed at run time.  blockIdx.z splits the BATCHES (never a batch): part z owns
// batches z * pb .. min(B, (z + 1) * pb) - 1 with pb = ceil(B / parts); a part past the last batch does nothing.  A part that does not
// begin the range fetches iteration t - 1 under that iteration's own inv row for its first flip; the first iteration of the range is
// compared with itself (no flip).  inv holds B * L rows; trace_stride = 0: every iteration reads the same row (a fixed-tau trace).
__global__ __launch_bounds__(256) void trace_batch_stats_kernel(const uint64_t *__restrict__ trace, size_t trace_stride,
                                                                const uint8_t *__restrict__ inv, int B, int L, int V, int G,
                                                                unsigned long long *__restrict__ sum, unsigned long long *__restrict__ first,
                                                                unsigned long long *__restrict__ bsq, int *__restrict__ flips)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int label = blockIdx.y;
    if (v >= V) return;
    const int pb = (B + (int)gridDim.z - 1) / (int)gridDim.z;
    const int b0 = (int)blockIdx.z * pb, b1 = min(B, b0 + pb);
    if (b0 >= b1) return;
    const int half = B >> 1;
    int t = b0 * L;
    const int tp = t > 0 ? t - 1 : 0;
    int prev = (int)(trace[(size_t)tp * trace_stride + v] >> (2 * (int)inv[(size_t)tp * G + label])) & 3;
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0, f0 = 0, f1 = 0, f2 = 0, f3 = 0, nf = 0;
    unsigned long long q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    for (int b = b0; b < b1; ++b) {
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        for (int i = 0; i < L; ++i, ++t) {
            const int sh = 2 * (int)inv[(size_t)t * G + label];
            const int d = (int)(trace[(size_t)t * trace_stride + v] >> sh) & 3;
            c0 += (d == 0); c1 += (d == 1); c2 += (d == 2); c3 += (d == 3);
            nf += (d != prev);
            prev = d;
        }
        s0 += c0; s1 += c1; s2 += c2; s3 += c3;
        q0 += (unsigned long long)c0 * (unsigned long long)c0; q1 += (unsigned long long)c1 * (unsigned long long)c1;
        q2 += (unsigned long long)c2 * (unsigned long long)c2; q3 += (unsigned long long)c3 * (unsigned long long)c3;
        if (b < half) { f0 += c0; f1 += c1; f2 += c2; f3 += c3; }
    }
    const size_t cell = (size_t)v * G + label;
    unsigned long long *ps = sum + cell * 4, *pf = first + cell * 4, *pq = bsq + cell * 4;
    if (s0) atomicAdd(ps + 0, (unsigned long long)s0);
    if (s1) atomicAdd(ps + 1, (unsigned long long)s1);
    if (s2) atomicAdd(ps + 2, (unsigned long long)s2);
    if (s3) atomicAdd(ps + 3, (unsigned long long)s3);
    if (f0) atomicAdd(pf + 0, (unsigned long long)f0);
    if (f1) atomicAdd(pf + 1, (unsigned long long)f1);
    if (f2) atomicAdd(pf + 2, (unsigned long long)f2);
    if (f3) atomicAdd(pf + 3, (unsigned long long)f3);
    if (q0) atomicAdd(pq + 0, q0);
    if (q1) atomicAdd(pq + 1, q1);
    if (q2) atomicAdd(pq + 2, q2);
    if (q3) atomicAdd(pq + 3, q3);
    if (nf) atomicAdd(flips + cell, nf);
}

static int g_diag_parts = 0;      // dsm_diag_debug_set_parts: iteration parts per launch (0 = by the grid the launch aims at)

extern "C" int dsm_diag_debug_set_parts(int parts)
{
    return dsm_set_knob(&g_diag_parts, parts, "diag", "parts");
}

// d_sum, d_first, d_bsq [V][G][4] int64 and d_flips [V][G] int32, zeroed here; d_inv [B * L][G]: inv[t][perm[t][g]] = g; B even
int k_trace_batch_stats(dsm_ctx *c, const TraceView &tr, const uint8_t *d_inv, int B, int L, int64_t *d_sum, int64_t *d_first,
                        int64_t *d_bsq, int32_t *d_flips)
{
    const int V = c->V, G = c->G;
    const size_t nt = (size_t)V * G * 4;
    HIP_TRY(hipMemsetAsync(d_sum, 0, nt * sizeof(int64_t), c->stream));
    HIP_TRY(hipMemsetAsync(d_first, 0, nt * sizeof(int64_t), c->stream));
    HIP_TRY(hipMemsetAsync(d_bsq, 0, nt * sizeof(int64_t), c->stream));
    HIP_TRY(hipMemsetAsync(d_flips, 0, (size_t)V * G * sizeof(int32_t), c->stream));
    if (B < 1) return DSM_OK;
    const int gx = (V + 255) / 256;
    const long long n = (long long)B * L;
    int gz = g_diag_parts > 0 ? g_diag_parts : (int)std::min<long long>({(DG_BLOCKS + gx * G - 1) / (gx * G), (n + 31) / 32, 1024});
    gz = std::max(1, std::min({gz, B, 65535}));                  // a part holds whole batches; gridDim.z
    hipLaunchKernelGGL(trace_batch_stats_kernel, dim3((unsigned)gx, (unsigned)G, (unsigned)gz), dim3(256), 0, c->stream, tr.tau,
                       tr.tau_stride, d_inv, B, L, V, G, reinterpret_cast<unsigned long long *>(d_sum),
                       reinterpret_cast<unsigned long long *>(d_first), reinterpret_cast<unsigned long long *>(d_bsq), d_flips);
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}
