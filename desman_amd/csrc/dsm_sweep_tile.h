// dsm_sweep_tile.h -- the frame of a kernel that visits every position of the resident tau with one group of LPV lanes, NSL sample slots
// per lane (slot j of lane l = sample l + j LPV; the tiling of the full sweep: kernels_gibbs.hip, tau_shape) on the plain fp64 tile:
// 256 threads, the grid strides over the positions.  held_sweep_kernel (kernels_heldtau.hip) and pair_sweep_kernel (kernels_pairtau.hip)
// are this frame around their own step: sweep_tile_stage, a loop over the group's positions (sweep_tile_counts, the steps, lane 0 writes
// the word; no barrier, nothing shared between positions), sweep_tile_nchange; launched through sweep_tile_dispatch.
#pragma once
#include <algorithm>

#include "dsm_device.h"
#include "dsm_host.h"
#include "log_table.h"

struct SweepTileParams {       // what every kernel of the frame is given; its own parameter block derives from this
    const int32_t *cnt_vs;     // [V][S][4]
    uint64_t *tau;             // [V] packed, 2 bits per haplotype
    const double *gamma, *eta; // [S][G], [4][4]
    const double *log_tab;     // [256][2]
    int *nchange;
    int V, S, G;
    uint32_t k0, k1, iter;     // Philox key (the chain's counter seed) and iteration counter
};

struct SweepTileLds {
    const double *gT, *eS;     // [G][LPV NSL] gamma transposed, [16] eta
    const double2 *ltab;       // [256] the logarithm's table
};

// Stages the three tables into dynamic LDS (sweep_tile_lds_bytes) and ends with the one barrier of the frame.  `pad` is gamma of a slot
// beyond S, by the caller's arithmetic: 1.0 under sweep_candidate's padded-slot rule, 0.0 under dsm_pair_candidates_row.
template <int LPV, int NSL>
__device__ __forceinline__ SweepTileLds sweep_tile_stage(const SweepTileParams &p, double pad)
{
    extern __shared__ __attribute__((aligned(16))) char sweep_tile_smem[];
    constexpr int SP = LPV * NSL;
    const int tid = threadIdx.x, G = p.G, S = p.S;
    double *gT = reinterpret_cast<double *>(sweep_tile_smem);
    double *eS = gT + (size_t)G * SP;
    double2 *ltab = reinterpret_cast<double2 *>(eS + 16);
    if (tid < DSM_LOG_TAB_N) ltab[tid] = reinterpret_cast<const double2 *>(p.log_tab)[tid];
    for (int i = tid; i < G * SP; i += 256) {
        const int g = i / SP, s = i % SP;
        gT[i] = (s < S) ? p.gamma[(size_t)s * G + g] : pad;
    }
    if (tid < 16) eS[tid] = p.eta[tid];
    __syncthreads();
    return {gT, eS, ltab};
}

// the count cells of position v at the NSL slots of lane `lig` of its group; zeros beyond S.  The conversion is the caller's
template <int LPV, int NSL>
__device__ __forceinline__ void sweep_tile_counts(const SweepTileParams &p, int v, int lig, int4 (&c)[NSL])
{
#pragma unroll
    for (int j = 0; j < NSL; ++j) {
        const int s = lig + j * LPV;
        c[j] = make_int4(0, 0, 0, 0);
        if (s < p.S) c[j] = reinterpret_cast<const int4 *>(p.cnt_vs)[(size_t)v * p.S + s];
    }
}

// the workgroup's changed digits (every thread's `nchg`; a group counts on its lane 0) -> one atomicAdd
__device__ __forceinline__ void sweep_tile_nchange(int *nchange, int nchg)
{
    __shared__ int redi[4];
    const int tid = threadIdx.x;
    const int wn = (int)group_allreduce_sum_u32<64>((unsigned)nchg);
    if ((tid & 63) == 0) redi[tid >> 6] = wn;
    __syncthreads();
    if (tid == 0) {
        const int tot = redi[0] + redi[1] + redi[2] + redi[3];
        if (tot) atomicAdd(nchange, tot);
    }
}

// ---------------------------------------------------------------- host side
static inline size_t sweep_tile_lds_bytes(int G, int LPV, int NSL) { return ((size_t)G * LPV * NSL + 16 + 2 * DSM_LOG_TAB_N) * sizeof(double); }
static inline int sweep_tile_grid(int V, int LPV) { const int gpb = 256 / LPV; return std::max(1, std::min((V + gpb - 1) / gpb, DSM_MAX_GRID)); }

template <auto Kernel, class P>
static int sweep_tile_launch(dsm_ctx *c, const P &p, int grid, size_t sh)
{
    static bool attr_set = false;                  // more than 64 KB of dynamic LDS has to be asked for, once per instantiation
    if (sh > 64 * 1024 && !attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(256), sh, c->stream, p);
    return DSM_OK;
}

// One launch over the V positions of p on the tiling of its S samples: launch(L, N, grid, lds bytes), L / N the tiling as
// std::integral_constant, is to call sweep_tile_launch<kernel<L.value, N.value>>.  `lds_what` / `what` open the error texts.
template <class P, class Launch>
static int sweep_tile_dispatch(const P &p, const char *lds_what, const char *what, Launch &&launch)
{
    int LPV, NSL;
    { const int rc = tau_shape(p.S, &LPV, &NSL); if (rc != DSM_OK) return rc; }
    const size_t sh = sweep_tile_lds_bytes(p.G, LPV, NSL);
    if (sh > 160 * 1024) { dsm_set_error("%sgamma tile (%zu B) exceeds LDS", lds_what, sh); return DSM_ERR_UNSUPPORTED; }
    const int rc = tau_tiling_dispatch(LPV, NSL, [&](auto L, auto N) { return launch(L, N, sweep_tile_grid(p.V, LPV), sh); });
    if (rc != DSM_OK) { if (rc == DSM_ERR_UNSUPPORTED) dsm_set_error("%s: no kernel for %d lanes x %d samples", what, LPV, NSL); return rc; }
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}
