// kernels_fixtau.hip -- gfx950 kernels of the fixed-tau chain (api.hip: dsm_ctx_gibbs_update_fixed_tau).
//
//   fixtau_pool_kernel       the counts of all positions that carry one packed tau word, added into that word's row
//   fixtau_fill_eta_kernel   fix_eta: every row of the eta trace = the held matrix
//   fixtau_add_const_kernel  the pooled chain's ll / lp -> the caller's table (the multinomial coefficients differ by a constant)
//
// The chain itself runs on the launchers of the Gibbs loop (kernels_stats.hip, kernels_gibbs.hip).
#include <algorithm>

#include "dsm_host.h"

// One thread per (position, sample): the 16 B slab of the cell is one coalesced int4 load, its non-zero counts go into the row of the
// position's word with vector integer atomics (global_atomic_add, no return value).  Integer sums: exact, and the same bits whatever
// order the atomics land in.  row[v] < W and pooled is [W][S][4] (api.hip: fixtau_words makes the map, fixtau_pool_counts the buffer);
// the host has checked that no sum passes INT32_MAX.
__global__ __launch_bounds__(256) void fixtau_pool_kernel(const int32_t *__restrict__ cnt_vs, const int32_t *__restrict__ row,
                                                          int32_t *__restrict__ pooled, int V, int S)
{
    const size_t n = (size_t)V * S;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int v = (int)(i / (size_t)S), s = (int)(i % (size_t)S);
        const int4 c = reinterpret_cast<const int4 *>(cnt_vs)[i];
        int32_t *dst = pooled + ((size_t)row[v] * S + s) * 4;
        if (c.x) atomicAdd(dst + 0, c.x);
        if (c.y) atomicAdd(dst + 1, c.y);
        if (c.z) atomicAdd(dst + 2, c.z);
        if (c.w) atomicAdd(dst + 3, c.w);
    }
}

__global__ __launch_bounds__(256) void fixtau_fill_eta_kernel(const double *__restrict__ eta, double *__restrict__ trace, int n)
{
    const size_t tot = (size_t)n * 16;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (size_t)gridDim.x * 256) trace[i] = eta[i & 15];
}

__global__ __launch_bounds__(256) void fixtau_add_const_kernel(double *__restrict__ ll, double *__restrict__ lp, int n,
                                                               double *__restrict__ star, double *__restrict__ scalars, double K)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) { ll[i] += K; lp[i] += K; }
    if (blockIdx.x == 0 && threadIdx.x == 0) { star[0] += K; scalars[0] += K; scalars[1] += K; }
}

int k_fixtau_pool(dsm_ctx *c, const int32_t *d_row, int32_t *d_pooled)
{
    const size_t n = (size_t)c->V * c->S;
    const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(fixtau_pool_kernel, dim3(grid), dim3(256), 0, c->stream, c->cnt_vs, d_row, d_pooled, c->V, c->S);
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}

int k_fixtau_fill_eta(dsm_ctx *c, const double *eta, double *eta_trace, int n)
{
    if (n < 1) return DSM_OK;
    const int grid = (int)std::min<size_t>(((size_t)n * 16 + 255) / 256, 1024);
    hipLaunchKernelGGL(fixtau_fill_eta_kernel, dim3(grid), dim3(256), 0, c->stream, eta, eta_trace, n);
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}

int k_fixtau_add_const(dsm_ctx *c, int n, double K)
{
    const int grid = std::max(1, std::min((n + 255) / 256, 1024));
    hipLaunchKernelGGL(fixtau_add_const_kernel, dim3(grid), dim3(256), 0, c->stream, c->ll_trace, c->lp_trace, n, c->star, c->scalars, K);
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}
