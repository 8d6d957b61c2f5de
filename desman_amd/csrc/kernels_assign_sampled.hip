// kernels_assign_sampled.hip -- sampled joint haplotype assignment of positions that were not in the fit: the form of dsm_assign_tau
// (kernels_assign.hip) that runs to G = DSM_MAX_G (include/desman_hip.h: dsm_assign_tau_sampled).
//
// Given gamma [S][G] and eta [4][4] the positions are independent, so every position carries C = 4 private Gibbs chains over its G
// sites.  Chain c starts at "every haplotype = base c"; sweeps t = 0 .. B+T-1 visit g = 0 .. G-1 in order; the first B sweeps are
// burn-in, the last T are kept.  A step of site g:
//     m_a[s]    = sum_{h != g, a_h = a} gamma[s][h]                         (h in order; formed afresh at every step)
//     rest[s][b]= ((m_0 eta[0][b] + m_1 eta[1][b]) + m_2 eta[2][b]) + m_3 eta[3][b]
//     L_a       = sum_{s,b: x > 0} x[s][b] ln(rest[s][b] + eta[a][b] gamma[s][g])      (the L of the whole state with a_g = a)
//     q_a       = exp(L_a - max) / ((e_0 + e_1) + e_2 + e_3);  all four -inf: q = 0 and the base stays
//     new base  = inverse CDF (u < q_0 ? 0 : u < q_0 + q_1 ? 1 : u < q_0 + q_1 + q_2 ? 2 : 3),
//     u         = word 0 / 2^32 of Philox4x32-10(key = (lo32, hi32) seed; counter = (lo32 i, hi32 i, t, DSM_STREAM_ASMP + c)),
//                 i = (position index within the call) G + g
// Outputs per position: the Rao-Blackwellised marginals (mean of q over the chains and the kept sweeps), their spread between the
// chains, the best state seen at any step of any chain polished by coordinate ascent, the share of the kept end-of-sweep states equal
// to it, and chain 0's last state.
//
// Shape of the work (the lane-group tiling of kernels_fit.hip: trace_fit_kernel):
//   * a group of LPV = 2^k >= min(S, 64) lanes per (position, chain), NSL = 1/2/4/8 sample slots per lane (slot j of lane l = sample
//     l + j LPV); the four chains of a position are four adjacent groups of one workgroup, PPW positions per workgroup.
//   * a thread keeps the counts of its NSL cells in registers for all sweeps; gamma is staged in LDS transposed ([g][slot]) -- once
//     where S G fits ASMP_LDS_GAMMA doubles (ONE = true), else in chunks of gc haplotypes at every step -- eta and the logarithm's
//     table beside it.  The state is a packed u64, two bits per haplotype; its digits are picked by compares against constants.
//   * the four candidate sums of a step meet over the lane group by xor halving (every lane ends with the same bits); the per-chain sums
//     of q sit in LDS ([group][g][a], added to by lane 0 of the group) and meet in chain order at the end.
//   * the kept end-of-sweep states go to device scratch [position][chain][T]; after the polish every group counts its own chain's.
//   * every loop bound is workgroup-uniform (the polish runs until no position of the workgroup is active; a finished position is
//     frozen), and a decision that only a chain shares (a step whose candidates are all -inf) skips no code that stages gamma, so
//     the barriers of the chunked staging are safe.
// Every sum runs in a fixed order, there are no atomics: the results depend on (seed, position index, counts, gamma, eta, B, T) only.
//
// Pair moves (PAIRS = true; dsm_assign_tau_sampled_pairs with pair_every = E > 0; E = 0 launches the PAIRS = false code above): sweep t
// is followed by a pair pass when (t + 1) mod E = 0 -- after its G steps, before its end-of-sweep state is kept.  The pass visits
// (g, h), g < h, in lexicographic order.  A step of pair (g, h):
//     m_a[s]    = sum_{k != g, h; a_k = a} gamma[s][k]                      (k in order), rest[s][b] as above
//     L_k       = sum_{s,b: x > 0} x[s][b] ln((rest[s][b] + eta[a][b] gamma[s][g]) + eta[a'][b] gamma[s][h]),  k = 4 a + a'
//     q_k       = exp(L_k - max) / (e_0 + e_1 + ... + e_15, in this order);  all sixteen -inf: q = 0 and the pair stays
//     new pair  = inverse CDF over ascending k (the last edge forced),
//     u         = word 0 / 2^32 of Philox4x32-10(key as above; counter = (lo32 j, hi32 j, t, DSM_STREAM_APAR + c)),
//                 j = (position index within the call) G^2 + g G + h
// The largest of the sixteen totals (the lowest k among equals), with the state that has this pair, enters the best-state tracking like
// a single-site step's chosen total; marg and spread see the single-site q only.
// The polish then alternates: coordinate ascent to its fixed point, one pass of pair ascent over g < h (arg-max of the sixteen; a tie
// with the current pair keeps it, else the lowest k), again while the pair pass changed something; ASMP_POLISH_CAP bounds the
// coordinate sweeps and pair passes that changed something, together (rounding orders totals that tie in the model differently under
// each pair: pair ascent alone need not end).  The sixteen totals are formed four at a time (one a, four a') from the m of the step.
// The polish keeps none of them (a running best and the current pair's); the chain's step keeps the sixteen and their exponentials
// in registers up to four slots per lane and, at eight, forms them three times (largest, sum, CDF) and keeps nothing.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dsm_device.h"
#include "dsm_host.h"
#include "dsm_host_util.h"
#include "log_table.h"

#define ASMP_LDS_GAMMA 4096         // doubles of LDS a chunk of gamma columns may take (32 KiB)
#define ASMP_LDS_ACC 2048           // doubles of LDS the chains' sums of q may take (16 KiB): bounds the positions per workgroup
#define ASMP_MAX_SWEEPS 65536
#define ASMP_POLISH_CAP 64

struct SampledParams {
    const int32_t *cnt;         // [N][S][4] of this launch
    const double *gamma;        // [S][G]
    const double *eta;          // [16]
    const double *log_tab;      // [256][2]
    int N, S, G;
    int lpv_log2, gc, ppw;      // log2 of the lanes per (position, chain); haplotypes per staged chunk; positions per workgroup
    int B, T;
    uint32_t k0, k1;            // Philox key
    unsigned long long pos0;    // index within the call of this launch's first position
    uint64_t *kept;             // [N][4][T] scratch
    uint64_t *map_state, *draw_state;       // [N] packed
    double *map_ll, *conf, *marg, *spread;  // [N], [N], [N][G][4], [N]
    int E;                      // a pair pass after every E-th sweep (PAIRS instantiations; 0 otherwise)
};

// (dsm_pair_candidates_row, the sixteen pair totals four at a time, dsm_put_row / dsm_get_row and the sixteen-way draw dsm_pair_draw16
// live in dsm_device.h: the pair pass of the Gibbs chain, kernels_pairtau.hip, shares them)
template <int NSL, bool ONE, bool PAIRS>
__global__ __launch_bounds__(256) void assign_sampled_kernel(const SampledParams p)
{
    extern __shared__ double2 asmp_smem[];
    const int LPV = 1 << p.lpv_log2, SP = LPV * NSL, PPW = p.ppw, NG = PPW * 4;
    const int tid = threadIdx.x, l = tid & (LPV - 1), grp = tid >> p.lpv_log2, pl = grp >> 2, c = grp & 3;
    const int S = p.S, G = p.G, gc = p.gc, nthr = NG * LPV;
    const long long v = (long long)blockIdx.x * PPW + pl;
    const bool vin = v < p.N;
    const double NINF = -INFINITY;

    double2 *const ltab = asmp_smem;
    double *const leta = reinterpret_cast<double *>(ltab + DSM_LOG_TAB_N);       // [16]
    double *const lgam = leta + 16;                                             // [gc][SP]
    double *const acc = lgam + (size_t)gc * SP;                                 // [NG][G][4]
    double *const redL = acc + (size_t)NG * G * 4;                              // [NG]
    uint64_t *const redS = reinterpret_cast<uint64_t *>(redL + NG);             // [NG]
    int *const redC = reinterpret_cast<int *>(redS + NG);                       // [NG]

    for (int i = tid; i < DSM_LOG_TAB_N; i += nthr) ltab[i] = reinterpret_cast<const double2 *>(p.log_tab)[i];
    for (int i = tid; i < 16; i += nthr) leta[i] = p.eta[i];
    for (int i = tid; i < NG * G * 4; i += nthr) acc[i] = 0.0;
    if (ONE)
        for (int i = tid; i < G * SP; i += nthr) {
            const int h = i / SP, s = i - h * SP;
            lgam[i] = s < S ? p.gamma[(size_t)s * G + h] : 0.0;
        }
    __syncthreads();

    double x[NSL][4];
#pragma unroll
    for (int j = 0; j < NSL; ++j) {
        const int s = l + j * LPV;
        int4 q = make_int4(0, 0, 0, 0);
        if (vin && s < S) q = *reinterpret_cast<const int4 *>(p.cnt + ((size_t)v * S + s) * 4);
        x[j][0] = (double)q.x; x[j][1] = (double)q.y; x[j][2] = (double)q.z; x[j][3] = (double)q.w;
    }

    // The masses of a step at the thread's slots, one pass over the haplotypes in order: m_a = the abundance of those that carry base a in
    // `state`, the step's own left out -- site g (gamma -> gg) and, `pair` a std::true_type, site h (gamma -> gh; else h and gh are not
    // looked at).  !ONE: the one place that stages gamma, chunk by chunk between its two barriers; every thread comes through here
    auto masses = [&](auto pair, uint64_t state, int g, int h, double (&m0)[NSL], double (&m1)[NSL], double (&m2)[NSL], double (&m3)[NSL],
                      double (&gg)[NSL], double (&gh)[NSL]) __attribute__((always_inline)) {
        constexpr bool PAIR = decltype(pair)::value;
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            m0[j] = 0.0; m1[j] = 0.0; m2[j] = 0.0; m3[j] = 0.0; gg[j] = 0.0;
            if constexpr (PAIR) gh[j] = 0.0;
        }
        for (int g0 = 0; g0 < G; g0 += gc) {
            const int gn = min(gc, G - g0);
            if (!ONE) {
                __syncthreads();                                    // the readers of the previous chunk are done
                for (int i = tid; i < gn * SP; i += nthr) {
                    const int kk = i / SP, s = i - kk * SP;
                    lgam[i] = s < S ? p.gamma[(size_t)s * G + g0 + kk] : 0.0;
                }
                __syncthreads();
            }
            for (int kk = 0; kk < gn; ++kk) {
                const int k = g0 + kk;
                const bool isg = k == g, ish = PAIR && k == h;
                const int d = (isg || ish) ? 4 : (int)(state >> (2 * k)) & 3;
#pragma unroll
                for (int j = 0; j < NSL; ++j) {
                    const double ga = lgam[kk * SP + l + j * LPV];
                    m0[j] += d == 0 ? ga : 0.0;
                    m1[j] += d == 1 ? ga : 0.0;
                    m2[j] += d == 2 ? ga : 0.0;
                    m3[j] += d == 3 ? ga : 0.0;
                    gg[j] = isg ? ga : gg[j];
                    if constexpr (PAIR) gh[j] = ish ? ga : gh[j];
                }
            }
        }
    };

    // the four candidate totals of site g of `state`, the same bits on every lane of the group
    auto candidates = [&](uint64_t state, int g, double (&L)[4]) {
        double m0[NSL], m1[NSL], m2[NSL], m3[NSL], gg[NSL];
        masses(std::false_type(), state, g, 0, m0, m1, m2, m3, gg, gg);
        L[0] = 0.0; L[1] = 0.0; L[2] = 0.0; L[3] = 0.0;
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double rest = ((m0[j] * leta[b] + m1[j] * leta[4 + b]) + m2[j] * leta[8 + b]) + m3[j] * leta[12 + b];
                const bool seen = x[j][b] > 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const double pr = rest + leta[a * 4 + b] * gg[j];
                    double lg = 0.0;
                    if (__builtin_expect(dsm_log_ok(pr), 1)) lg = dsm_log_core(pr, ltab);
                    else if (seen) lg = dsm_log_slow(pr);           // 0 under a positive count: -inf (an unseen cell is never evaluated)
                    L[a] += seen ? x[j][b] * lg : 0.0;
                }
            }
        }
        for (int off = LPV >> 1; off > 0; off >>= 1) {
            L[0] += __shfl_xor(L[0], off); L[1] += __shfl_xor(L[1], off); L[2] += __shfl_xor(L[2], off); L[3] += __shfl_xor(L[3], off);
        }
    };

    // the sixteen candidate totals of the pair (g, h) of `state`, four at a time: row(a, R) is called for a = 0 .. 3 in order with
    // R[a'] = L_{4 a + a'}, the same bits on every lane of the group.  Nothing of a row outlives its call here: what a caller keeps of the
    // sixteen is its own choice (eight slots per lane leave no registers for all of them)
    auto pair_rows = [&](uint64_t state, int g, int h, auto &&row) __attribute__((always_inline)) {
        double m0[NSL], m1[NSL], m2[NSL], m3[NSL], gg[NSL], gh[NSL];
        masses(std::true_type(), state, g, h, m0, m1, m2, m3, gg, gh);
#pragma unroll 1
        for (int a = 0; a < 4; ++a) {                               // four candidates at a time: the register budget of a single-site step
            double R[4];
            dsm_pair_candidates_row<NSL>(x, m0, m1, m2, m3, gg, gh, leta, ltab, a, R);
            for (int off = LPV >> 1; off > 0; off >>= 1) {
                R[0] += __shfl_xor(R[0], off); R[1] += __shfl_xor(R[1], off); R[2] += __shfl_xor(R[2], off); R[3] += __shfl_xor(R[3], off);
            }
            row(a, R);
        }
    };
    constexpr bool KEEP16 = NSL < 8;    // the chain's pair step keeps the sixteen totals; at eight slots it forms them three times instead

    // ---- the chain
    const uint64_t gmask = G == 32 ? ~0ull : ((1ull << (2 * G)) - 1ull);
    uint64_t state = (0x5555555555555555ull * (uint64_t)c) & gmask;
    double bestL = NINF;
    uint64_t bestS = 0ull;
    const unsigned long long ibase = (p.pos0 + (unsigned long long)(vin ? v : 0)) * (unsigned long long)G;
    double *const myacc = acc + (size_t)grp * G * 4;
    const int nsweep = p.B + p.T;
    for (int t = 0; t < nsweep; ++t) {
        const bool keep = t >= p.B;
        for (int g = 0; g < G; ++g) {
            double L[4];
            candidates(state, g, L);
            const unsigned long long i = ibase + (unsigned long long)g;
            uint32_t w[4];
            philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)t, DSM_STREAM_ASMP + (uint32_t)c, p.k0, p.k1, w);
            const double mx = fmax(fmax(L[0], L[1]), fmax(L[2], L[3]));
            if (mx == NINF) continue;                               // group-uniform: the base stays, q = 0; the uniform is spent
            const double e0 = L[0] == NINF ? 0.0 : exp(L[0] - mx), e1 = L[1] == NINF ? 0.0 : exp(L[1] - mx);
            const double e2 = L[2] == NINF ? 0.0 : exp(L[2] - mx), e3 = L[3] == NINF ? 0.0 : exp(L[3] - mx);
            const double sum = ((e0 + e1) + e2) + e3;
            const double q0 = e0 / sum, q1 = e1 / sum, q2 = e2 / sum, q3 = e3 / sum;
            const double c0 = q0, c1 = c0 + q1, c2 = c1 + q2;
            const double u = (double)w[0] * 2.3283064365386963e-10;
            const int a = u < c0 ? 0 : (u < c1 ? 1 : (u < c2 ? 2 : 3));
            state = (state & ~(3ull << (2 * g))) | ((uint64_t)a << (2 * g));
            const double La = a == 0 ? L[0] : (a == 1 ? L[1] : (a == 2 ? L[2] : L[3]));
            if (La > bestL) { bestL = La; bestS = state; }
            if (keep && l == 0) {
                double *o = myacc + g * 4;
                o[0] += q0; o[1] += q1; o[2] += q2; o[3] += q3;
            }
        }
        if (PAIRS && (t + 1) % p.E == 0) {
            // ---- the pair pass of sweep t: after its G steps, before its end-of-sweep state is kept
            const unsigned long long jbase = (p.pos0 + (unsigned long long)(vin ? v : 0)) * (unsigned long long)G * (unsigned long long)G;
            for (int g = 0; g < G; ++g)
                for (int h = g + 1; h < G; ++h) {
                    double L[16], mx = NINF;
                    int kmax = 0;                                   // the lowest k of the largest total
#pragma unroll
                    for (int k = 0; k < 16; ++k) L[k] = 0.0;
                    pair_rows(state, g, h, [&](int a, const double (&R)[4]) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (R[i] > mx) { mx = R[i]; kmax = 4 * a + i; }
                        if (KEEP16) dsm_put_row(L, a, R);
                    });
                    // all sixteen -inf: the pair stays, its uniform is spent unseen.  The decision is per chain (group-uniform only), so
                    // it may skip code only where no barrier follows: with the sixteen kept nothing below stages gamma; without them
                    // the two further formations run in every chain of the workgroup and `live` guards their arithmetic instead
                    const bool live = mx != NINF;
                    if (KEEP16 && !live) continue;
                    const uint64_t others = state & ~((3ull << (2 * g)) | (3ull << (2 * h)));
                    if (mx > bestL) { bestL = mx; bestS = others | ((uint64_t)(kmax >> 2) << (2 * g)) | ((uint64_t)(kmax & 3) << (2 * h)); }
                    const unsigned long long jj = jbase + (unsigned long long)(g * G + h);
                    uint32_t w[4];
                    philox4x32_10((uint32_t)jj, (uint32_t)(jj >> 32), (uint32_t)t, DSM_STREAM_APAR + (uint32_t)c, p.k0, p.k1, w);
                    const double u = (double)w[0] * 2.3283064365386963e-10;
                    int kn = 15;                                    // the last edge is forced
                    if (KEEP16) {
                        kn = dsm_pair_draw16<true>(L, mx, u);
                    } else {                                        // the same totals again, bit for bit: twice more
                        double sum = 0.0, cdf = 0.0;
                        bool found = false;
                        pair_rows(state, g, h, [&](int, const double (&R)[4]) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) sum += (!live || R[i] == NINF) ? 0.0 : exp(R[i] - mx);
                        });
                        pair_rows(state, g, h, [&](int a, const double (&R)[4]) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                cdf += live ? (R[i] == NINF ? 0.0 : exp(R[i] - mx)) / sum : 0.0;
                                if (!found && 4 * a + i < 15 && u < cdf) { kn = 4 * a + i; found = true; }
                            }
                        });
                    }
                    if (live) state = others | ((uint64_t)(kn >> 2) << (2 * g)) | ((uint64_t)(kn & 3) << (2 * h));
                }
        }
        if (keep && l == 0 && vin) p.kept[((size_t)v * 4 + c) * p.T + (t - p.B)] = state;
    }

    // ---- the best state of the four chains: ties to the lowest chain
    if (l == 0) { redL[grp] = bestL; redS[grp] = bestS; }
    __threadfence();
    __syncthreads();
    double curL = NINF;
    uint64_t cur = 0ull;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double Lk = redL[pl * 4 + k];
        if (Lk > curL) { curL = Lk; cur = redS[pl * 4 + k]; }
    }
    const bool dead = curL == NINF;

    // ---- marginals, spread, the draw: one thread per position
    if (vin && c == 0 && l == 0) {
        const double *a0 = acc + (size_t)(pl * 4) * G * 4, *a1 = a0 + G * 4, *a2 = a1 + G * 4, *a3 = a2 + G * 4;
        double *mg = p.marg + (size_t)v * G * 4;
        const double T1 = (double)p.T, T4 = 4.0 * (double)p.T;
        double sp = 0.0;
        for (int k = 0; k < G * 4; ++k) {
            const double s0 = a0[k], s1 = a1[k], s2 = a2[k], s3 = a3[k];
            const double hi = fmax(fmax(s0, s1), fmax(s2, s3)), lo = fmin(fmin(s0, s1), fmin(s2, s3));
            mg[k] = dead ? 0.0 : (((s0 + s1) + s2) + s3) / T4;
            sp = fmax(sp, (hi - lo) / T1);
        }
        p.spread[v] = dead ? 0.0 : sp;
        p.draw_state[v] = dead ? 0ull : state;
    }

    // ---- polish by coordinate ascent: the arg-max candidate of every site, ties keep the base, else the lowest a.  PAIRS: rounds of
    // (coordinate ascent to its fixed point, one pass of pair ascent) until a pair pass changes nothing
    bool open = vin && !dead;       // the position's polish has not ended (read by the pair pass only)
    bool active = open;
    int nsw = 0;
    for (;;) {
        for (;;) {
            bool changed = false;
            for (int g = 0; g < G; ++g) {
                double L[4];
                candidates(cur, g, L);
                const int d = (int)(cur >> (2 * g)) & 3;
                double best = d == 0 ? L[0] : (d == 1 ? L[1] : (d == 2 ? L[2] : L[3]));
                int a = d;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (L[k] > best) { best = L[k]; a = k; }
                if (active) {
                    if (a != d) { cur = (cur & ~(3ull << (2 * g))) | ((uint64_t)a << (2 * g)); changed = true; }
                    curL = best;
                }
            }
            if (active && (!changed || ++nsw == ASMP_POLISH_CAP)) { active = false; open = open && !changed; }
            if (!__syncthreads_or(active ? 1 : 0)) break;
        }
        if (!PAIRS) break;
        bool moved = false;
        for (int g = 0; g < G; ++g)
            for (int h = g + 1; h < G; ++h) {
                const int k0 = (((int)(cur >> (2 * g)) & 3) << 2) | ((int)(cur >> (2 * h)) & 3);
                double best = NINF, L0 = NINF;                      // the largest total (kn: its lowest k) and the current pair's
                int kn = 0;
                pair_rows(cur, g, h, [&](int a, const double (&R)[4]) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (R[i] > best) { best = R[i]; kn = 4 * a + i; }
                        L0 = 4 * a + i == k0 ? R[i] : L0;
                    }
                });
                const bool cur_is_best = L0 == best;                // the current pair's total equals the largest: it stays
                if (open) {
                    if (!cur_is_best) {
                        cur = (cur & ~((3ull << (2 * g)) | (3ull << (2 * h)))) | ((uint64_t)(kn >> 2) << (2 * g)) | ((uint64_t)(kn & 3) << (2 * h));
                        moved = true;
                    }
                    curL = best;
                }
            }
        if (open && (!moved || ++nsw == ASMP_POLISH_CAP)) open = false;     // a pair pass that changed nothing ends the polish
        active = open;
        if (!__syncthreads_or(open ? 1 : 0)) break;
    }

    // ---- conf: the kept end-of-sweep states equal to the polished state
    int n = 0;
    if (vin && !dead) {
        const uint64_t *kp = p.kept + ((size_t)v * 4 + c) * p.T;
        for (int k = l; k < p.T; k += LPV) n += kp[k] == cur ? 1 : 0;
    }
    for (int off = LPV >> 1; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (l == 0) redC[grp] = n;
    __syncthreads();
    if (vin && c == 0 && l == 0) {
        const int tot = redC[pl * 4] + redC[pl * 4 + 1] + redC[pl * 4 + 2] + redC[pl * 4 + 3];
        p.conf[v] = (double)tot / (4.0 * (double)p.T);
        p.map_state[v] = dead ? 0ull : cur;
        p.map_ll[v] = curL;
    }
}

// ---------------------------------------------------------------- host side
static int g_asmp_chunk = 0;        // dsm_assign_sampled_debug_set_chunk: positions per launch (0 = by the scratch bound)

extern "C" int dsm_assign_sampled_debug_set_chunk(int positions)
{
    return dsm_set_knob(&g_asmp_chunk, positions, "assign_sampled", "chunk");
}

namespace {
struct SampledPlan { int inst, lpv, lpv_log2, nsl, gc, ppw; size_t lds; };
}  // namespace

static int asmp_plan(int S, int G, SampledPlan *pl)
{
    if (S < 1 || G < 1) { dsm_set_error("assign_sampled: S=%d, G=%d", S, G); return DSM_ERR_ARG; }
    if (S > DSM_MAX_S) { dsm_set_error("assign_sampled: S=%d exceeds DSM_MAX_S=%d", S, DSM_MAX_S); return DSM_ERR_UNSUPPORTED; }
    if (G > DSM_MAX_G) { dsm_set_error("assign_sampled: G=%d exceeds DSM_MAX_G=%d", G, DSM_MAX_G); return DSM_ERR_UNSUPPORTED; }
    int lg = 0;
    while (lg < 6 && (1 << lg) < S) ++lg;
    const int need = (S + 63) / 64;
    pl->lpv_log2 = lg; pl->lpv = 1 << lg;
    pl->nsl = need <= 1 ? 1 : (need <= 2 ? 2 : (need <= 4 ? 4 : 8));
    const int SP = pl->lpv * pl->nsl;
    pl->gc = std::max(1, std::min(G, ASMP_LDS_GAMMA / SP));
    int ppw = 64 / pl->lpv;
    while (ppw > 1 && ppw * 16 * G > ASMP_LDS_ACC) ppw >>= 1;
    pl->ppw = ppw;
    const int nslot = pl->nsl == 1 ? 0 : (pl->nsl == 2 ? 1 : (pl->nsl == 4 ? 2 : 3));
    pl->inst = nslot * 2 + (pl->gc < G ? 1 : 0);
    const int NG = ppw * 4;
    pl->lds = (size_t)DSM_LOG_TAB_N * 16 + ((size_t)16 + (size_t)pl->gc * SP + (size_t)NG * G * 4 + NG + NG) * 8 + (size_t)NG * 4;
    return DSM_OK;
}

// out[5]: instantiation (2 log2 NSL + 1 where gamma is staged in chunks), LPV, NSL, haplotypes per gamma chunk, positions per workgroup
extern "C" int dsm_assign_sampled_debug_path(int S, int G, int *out)
{
    if (!out) { dsm_set_error("assign_sampled_debug_path: null pointer"); return DSM_ERR_ARG; }
    SampledPlan pl;
    DSM_TRY(asmp_plan(S, G, &pl));
    out[0] = pl.inst; out[1] = pl.lpv; out[2] = pl.nsl; out[3] = pl.gc; out[4] = pl.ppw;
    return DSM_OK;
}

static int asmp_check_model(int S, int G, const double *gamma, const double *eta, long long burn, long long kept, long long pair_every)
{
    SampledPlan pl;
    DSM_TRY(asmp_plan(S, G, &pl));
    if (kept < 1 || burn < 0) { dsm_set_error("assign_sampled: burn=%lld, kept=%lld", burn, kept); return DSM_ERR_ARG; }
    if (pair_every < 0) { dsm_set_error("assign_sampled: pair_every=%lld", pair_every); return DSM_ERR_ARG; }
    if (pair_every > ASMP_MAX_SWEEPS) {
        dsm_set_error("assign_sampled: pair_every = %lld exceeds %d", pair_every, ASMP_MAX_SWEEPS);
        return DSM_ERR_UNSUPPORTED;
    }
    if (burn + kept > ASMP_MAX_SWEEPS) {
        dsm_set_error("assign_sampled: burn + kept = %lld exceeds %d sweeps", burn + kept, ASMP_MAX_SWEEPS);
        return DSM_ERR_UNSUPPORTED;
    }
    DSM_TRY(dsm_check_gamma("assign_sampled", gamma, (size_t)S * G));
    return dsm_check_eta("assign_sampled", eta);
}

template <int NSL, bool ONE, bool PAIRS>
static int asmp_launch_as(const SampledPlan &pl, const SampledParams &q)
{
    const void *fn = reinterpret_cast<const void *>(&assign_sampled_kernel<NSL, ONE, PAIRS>);
    DSM_TRY(dsm_allow_lds(fn, pl.lds, "assign_sampled"));      // (asmp_plan keeps the tile below 64 KB: only the upper half of the gate can act)
    const unsigned blocks = (unsigned)((q.N + pl.ppw - 1) / pl.ppw), threads = (unsigned)(pl.ppw * 4 * pl.lpv);
    hipLaunchKernelGGL((assign_sampled_kernel<NSL, ONE, PAIRS>), dim3(blocks), dim3(threads), pl.lds, 0, q);
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}

template <int NSL, bool ONE>
static int asmp_launch(const SampledPlan &pl, const SampledParams &q)
{
    return q.E > 0 ? asmp_launch_as<NSL, ONE, true>(pl, q) : asmp_launch_as<NSL, ONE, false>(pl, q);
}

// d_cnt: the whole tensor on the device (context form), or null with h_cnt = the caller's int64 tensor (uploaded chunk by chunk)
static int asmp_run(const int32_t *d_cnt, const int64_t *h_cnt, int N, int S, int G, const double *gamma, const double *eta, uint64_t seed,
                    int burn, int kept, int pair_every, uint8_t *map_state, double *map_ll, double *conf, double *marg, double *spread,
                    uint8_t *draw_state)
{
    SampledPlan pl;
    DSM_TRY(asmp_plan(S, G, &pl));
    // positions per launch: everything sized by it -- the kept states, the uploaded counts, the outputs -- stays below 32 MB together
    // whatever N, S, G and T are
    const size_t per_pos = (size_t)4 * kept * sizeof(uint64_t) + (d_cnt ? 0 : (size_t)S * 4 * sizeof(int32_t)) + (size_t)4 * G * sizeof(double) +
                           2 * sizeof(uint64_t) + 3 * sizeof(double);
    int NC = (int)std::max<size_t>(1, std::min<size_t>((size_t)1 << 16, ((size_t)32 << 20) / per_pos));
    if (g_asmp_chunk > 0) NC = g_asmp_chunk;
    NC = std::min(NC, N);
    DevBuf<int32_t> d_x; DevBuf<double> d_gamma, d_eta, d_ltab, d_ll, d_conf, d_marg, d_spread;
    DevBuf<uint64_t> d_kept, d_map, d_draw;
    if (!d_cnt) DSM_TRY(d_x.alloc((size_t)NC * S * 4));
    DSM_TRY(d_gamma.alloc((size_t)S * G)); DSM_TRY(d_eta.alloc(16)); DSM_TRY(d_ltab.alloc(2 * DSM_LOG_TAB_N));
    DSM_TRY(d_kept.alloc((size_t)NC * 4 * kept)); DSM_TRY(d_map.alloc(NC)); DSM_TRY(d_draw.alloc(NC));
    DSM_TRY(d_ll.alloc(NC)); DSM_TRY(d_conf.alloc(NC)); DSM_TRY(d_marg.alloc((size_t)NC * 4 * G)); DSM_TRY(d_spread.alloc(NC));
    HIP_TRY(hipMemcpy(d_gamma, gamma, (size_t)S * G * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_eta, eta, 16 * sizeof(double), hipMemcpyHostToDevice));
    DSM_TRY(dsm_upload_log_table(d_ltab));
    std::vector<int32_t> x32;
    std::vector<uint64_t> word((size_t)NC);
    auto unpack = [&](uint8_t *dst, int n0, int n) {
        for (int i = 0; i < n; ++i)
            for (int g = 0; g < G; ++g) dst[(size_t)(n0 + i) * G + g] = (uint8_t)((word[i] >> (2 * g)) & 3u);
    };
    for (int n0 = 0; n0 < N; n0 += NC) {
        const int n = std::min(NC, N - n0);
        const int32_t *cnt = d_cnt ? d_cnt + (size_t)n0 * S * 4 : d_x.p;
        if (!d_cnt) DSM_TRY(dsm_stage_counts(h_cnt + (size_t)n0 * S * 4, (size_t)n * S * 4, d_x, x32, nullptr));
        SampledParams q;
        q.cnt = cnt; q.gamma = d_gamma; q.eta = d_eta; q.log_tab = d_ltab;
        q.N = n; q.S = S; q.G = G; q.lpv_log2 = pl.lpv_log2; q.gc = pl.gc; q.ppw = pl.ppw; q.B = burn; q.T = kept; q.E = pair_every;
        q.k0 = (uint32_t)seed; q.k1 = (uint32_t)(seed >> 32); q.pos0 = (unsigned long long)n0;
        q.kept = d_kept; q.map_state = d_map; q.draw_state = d_draw; q.map_ll = d_ll; q.conf = d_conf; q.marg = d_marg; q.spread = d_spread;
        switch (pl.inst) {
        case 0: DSM_TRY((asmp_launch<1, true>(pl, q))); break;
        case 1: DSM_TRY((asmp_launch<1, false>(pl, q))); break;
        case 2: DSM_TRY((asmp_launch<2, true>(pl, q))); break;
        case 3: DSM_TRY((asmp_launch<2, false>(pl, q))); break;
        case 4: DSM_TRY((asmp_launch<4, true>(pl, q))); break;
        case 5: DSM_TRY((asmp_launch<4, false>(pl, q))); break;
        case 6: DSM_TRY((asmp_launch<8, true>(pl, q))); break;
        default: DSM_TRY((asmp_launch<8, false>(pl, q))); break;
        }
        HIP_TRY(hipMemcpy(word.data(), d_map, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        unpack(map_state, n0, n);
        HIP_TRY(hipMemcpy(marg + (size_t)n0 * 4 * G, d_marg, (size_t)n * 4 * G * sizeof(double), hipMemcpyDeviceToHost));
        if (map_ll) HIP_TRY(hipMemcpy(map_ll + n0, d_ll, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        if (conf) HIP_TRY(hipMemcpy(conf + n0, d_conf, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        if (spread) HIP_TRY(hipMemcpy(spread + n0, d_spread, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        if (draw_state) {
            HIP_TRY(hipMemcpy(word.data(), d_draw, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
            unpack(draw_state, n0, n);
        }
    }
    return DSM_OK;
}

extern "C" int dsm_assign_tau_sampled_pairs(int device, const int64_t *counts, int N, int S, int G, const double *gamma, const double *eta,
                                            uint64_t seed, int burn, int kept, int pair_every, uint8_t *map_state, double *map_ll,
                                            double *conf, double *marg, double *spread, uint8_t *draw_state)
{
    if (N < 0 || !gamma || !eta || (N > 0 && (!counts || !map_state || !marg))) {
        dsm_set_error("assign_tau_sampled: bad arguments");
        return DSM_ERR_ARG;
    }
    DSM_TRY(asmp_check_model(S, G, gamma, eta, burn, kept, pair_every));
    DSM_TRY(dsm_check_counts("assign_tau_sampled", counts, (size_t)N, S));
    if (N == 0) return DSM_OK;
    DSM_TRY(dsm_bind_device(device));
    return asmp_run(nullptr, counts, N, S, G, gamma, eta, seed, burn, kept, pair_every, map_state, map_ll, conf, marg, spread, draw_state);
}

extern "C" int dsm_assign_tau_sampled(int device, const int64_t *counts, int N, int S, int G, const double *gamma, const double *eta,
                                      uint64_t seed, int burn, int kept, uint8_t *map_state, double *map_ll, double *conf, double *marg,
                                      double *spread, uint8_t *draw_state)
{
    return dsm_assign_tau_sampled_pairs(device, counts, N, S, G, gamma, eta, seed, burn, kept, 0, map_state, map_ll, conf, marg, spread,
                                        draw_state);
}

extern "C" int dsm_ctx_assign_tau_sampled_pairs(dsm_ctx *c, const double *gamma, const double *eta, int G, uint64_t seed, int burn, int kept,
                                                int pair_every, uint8_t *map_state, double *map_ll, double *conf, double *marg,
                                                double *spread, uint8_t *draw_state)
{
    DSM_TRY(dsm_ctx_enter(c, true));
    if (!gamma || !eta || !map_state || !marg) { dsm_set_error("ctx_assign_tau_sampled: null pointer"); return DSM_ERR_ARG; }
    DSM_TRY(asmp_check_model(c->S, G, gamma, eta, burn, kept, pair_every));
    return asmp_run(c->cnt_vs, nullptr, c->V, c->S, G, gamma, eta, seed, burn, kept, pair_every, map_state, map_ll, conf, marg, spread,
                    draw_state);
}

extern "C" int dsm_ctx_assign_tau_sampled(dsm_ctx *c, const double *gamma, const double *eta, int G, uint64_t seed, int burn, int kept,
                                          uint8_t *map_state, double *map_ll, double *conf, double *marg, double *spread,
                                          uint8_t *draw_state)
{
    return dsm_ctx_assign_tau_sampled_pairs(c, gamma, eta, G, seed, burn, kept, 0, map_state, map_ll, conf, marg, spread, draw_state);
}
