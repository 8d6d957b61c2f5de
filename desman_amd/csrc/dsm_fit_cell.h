// dsm_fit_cell.h -- the likelihood's own cell probabilities p_b = sum_g gamma_t[s][g] eta_t[tau_t[v][g]][b] as the trace reductions of the
// posterior predictive checks form them: trace_fit_kernel (kernels_fit.hip) and trace_ppc_kernel (kernels_ppc.hip,
// sec. 8k) call the same two functions, so a cell's p is the same bits in both -- and the same as check.cell_terms restates.
#pragma once
#include "dsm_device.h"

// The mixture over the four true bases m_a = sum_g gamma_t[s][g] [digit_g = a] of a thread's NSL cells (slot j of lane l = sample
// l + j LPV, LPV = 2^lpv_log2 lanes per position, SP = LPV NSL sample slots), g ascending.  gamma_t [S][G] is staged in LDS transposed --
// lgam [g][slot], so that the lanes of a group read consecutive doubles -- in chunks of gc haplotypes, eta_t [16] into leta with the first
// chunk.  Every thread of the 256-thread workgroup calls it (it holds barriers); `word` is the packed tau of the thread's position.
// A slot past S reads gamma 0: m = 0.  leta stays valid until the next call.
template <int NSL>
__device__ __forceinline__ void fit_cell_mixture(const double *__restrict__ gam_t, const double *__restrict__ eta_t, uint64_t word, int S, int G,
                                                 int gc, int lpv_log2, double *lgam, double *leta, double (&m0)[NSL], double (&m1)[NSL],
                                                 double (&m2)[NSL], double (&m3)[NSL])
{
    const int LPV = 1 << lpv_log2, SP = LPV * NSL;
    const int tid = threadIdx.x, l = tid & (LPV - 1);
#pragma unroll
    for (int j = 0; j < NSL; ++j) { m0[j] = 0.0; m1[j] = 0.0; m2[j] = 0.0; m3[j] = 0.0; }
    for (int g0 = 0; g0 < G; g0 += gc) {
        const int gn = min(gc, G - g0);
        __syncthreads();                                    // the readers of the previous chunk are done
        for (int i = tid; i < gn * SP; i += 256) {
            const int gg = i / SP, s = i - gg * SP;
            lgam[i] = s < S ? gam_t[(size_t)s * G + g0 + gg] : 0.0;
        }
        if (g0 == 0 && tid < 16) leta[tid] = eta_t[tid];
        __syncthreads();
        for (int gg = 0; gg < gn; ++gg) {
            const int d = (int)(word >> (2 * (g0 + gg))) & 3;
#pragma unroll
            for (int j = 0; j < NSL; ++j) {
                const double ga = lgam[gg * SP + l + j * LPV];
                m0[j] += d == 0 ? ga : 0.0;
                m1[j] += d == 1 ? ga : 0.0;
                m2[j] += d == 2 ? ga : 0.0;
                m3[j] += d == 3 ? ga : 0.0;
            }
        }
    }
}

// p_b of a cell from its mixture weights: the true bases in ascending order
__device__ __forceinline__ double fit_cell_p(double m0, double m1, double m2, double m3, const double *leta, int b)
{
    return ((m0 * leta[b] + m1 * leta[4 + b]) + m2 * leta[8 + b]) + m3 * leta[12 + b];
}
