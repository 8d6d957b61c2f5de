// kernels_stats.hip -- A2, the auxiliary-count sums (HaploSNP_Sampler.py:284-309 via :266,:276), "spec v2":
// the aggregated sampler restated in oracle/stats_agg.c (the law and its derivation are in that header).
//
//   stats_agg_kernel     stage 1: one wavefront per (variant, 64 samples); lane = sample, the 16 B count slab
//                        of (v,s) is one coalesced int4 load (the tau kernel's layout: no second copy of the
//                        tensor).  tau_v is wave-uniform, so the haplotype sets H_a(v) and the branches of the
//                        Gamma_a accumulation are scalar.  Per lane: Multinomial(x_b; eta[a,b] Gamma_a) for the
//                        four observed bases (dsm_binom.h: mult4) -> Esum (lane-private LDS columns) and the
//                        subset counts N[H_a(v)][s] (one coalesced row of global atomics per true base).
//                        Cost per cell ~ O(G + errors).  Inversion only: an item whose rarer outcome has a mean
//                        above 64 (DSM_LEAN_CAP), or more than DSM_XS reads off its heaviest base, is pushed onto a
//                        work list instead (lean kernel: <= 80 VGPRs, no rejection loop).  The lists: one per kind of
//                        item (rejection sampler / long search / search + two more binomials) x DSM_BIG_NL, each with
//                        its own counter -- workgroup b appends to list b mod DSM_BIG_NL of the kind.
//   stats_big_kernel     the listed items, one lane each (compacted, a wavefront holds items of one kind: no idle
//                        lanes, no path run for one lane only).  Items are independent work units (own Philox
//                        stream each): which kernel draws an item does not change the draw.
//   stats_stage2_kernel  stage 2: one workgroup per sample spreads N[.][s] over the haplotypes by recursive
//                        halving of the haplotype range (one large-count binomial per (node, subset): BTRS).
//   stats v1 (per-read draws, kernels_gibbs.hip: stats_kernel) remains for G > 16 / tables above 64 MB.
#include "dsm_binom.h"
#include "dsm_host.h"
#include "dsm_big_item.h"
#include "log_table.h"

#include <string.h>

#include <algorithm>
#include <vector>

// ablation switches of DESMAN_HIP_STATS_DBG: only in the experiment build (dsm_host.h: DSM_AB_SWITCHES); the product kernel has none of the tests
#ifdef DSM_AB_SWITCHES
#define STATS_DBG(p, mask) ((p).dbg & (mask))
#else
#define STATS_DBG(p, mask) 0
#endif
#ifdef DSM_AB_SWITCHES           // wave time stamps of stage 1 (experiment build only; dsm_debug_s1_clocks reads them): [wave][entry, tables staged, after pass 1, 2, ..., before the epilogue, end]
#define S1_NCLK 16
__device__ unsigned long long s1_clk[8192 * S1_NCLK];
#define S1_CLK(k) do { if ((threadIdx.x & 63) == 0 && blockIdx.y == 0) s1_clk[(size_t)(blockIdx.x * 4 + (threadIdx.x >> 6)) * S1_NCLK + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" int dsm_debug_s1_clocks(unsigned long long *out, int nwaves)
{
    if (nwaves > 8192) nwaves = 8192;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(s1_clk), (size_t)nwaves * S1_NCLK * sizeof(unsigned long long)) != hipSuccess) return -1;
    return S1_NCLK;
}
#else
#define S1_CLK(k) do { } while (0)
#endif
#define S1_CLKP(j) do { if (s1_pass < 3) S1_CLK(2 + 4 * s1_pass + (j)); } while (0)
struct StatsAggParams {
    const int32_t *cnt_vs;
    const uint64_t *tau;
    const double *gamma, *eta;
    int V, S, G;
    int v_off, V_tot;               // a chain sharded over GPUs by positions: this context holds positions v_off .. v_off + V of V_tot; the
                                    // counter-based streams are keyed by GLOBAL cell indices, so the draws do not depend on the sharding
    uint32_t k0, k1, iter;
    uint32_t *ntab;                 // [rep][2^G][ld]; workgroup b adds to copy b mod rep
    int rep, ld;                    // ld: row stride in words, >= S (ensure_ntab)
    unsigned long long *esum;       // [16]
    const double *log_tab;
    unsigned long long *big_list;   // deferred items: cell * 4 + observed base; DSM_BIG_NL sub-lists of big_seg entries each
    uint32_t *big_count;            // [DSM_BIG_NL] counters, 64 B apart (workgroup b appends to sub-list b % DSM_BIG_NL: one
                                    // counter took every deferring wavefront's atomic in turn, ~8 ns each -- 35k of them = the
                                    // whole pass on deep data)
    size_t big_seg;
    double lean_cap;                // stage 1 hands an item whose rarer outcome has a mean above this to the compacted kernel
    uint32_t swz;                   // ... + (s >> 4) * swz: the four 64 B lines of a subset's 64 samples sit in four different rows (dsm_host.h: DSM_NTAB_SWZ)
    uint32_t hmul;                  // the row of subset H is (H * hmul) mod 2^G (dsm_stage2.h: s2_row): an odd multiplier scatters the hot
                                    // subsets over the memory channels whatever the table's address
    int xcd;                        // 1: the table has a copy per XCD (rep = 8 k); a workgroup adds to a copy of ITS XCD (HW_REG_XCC_ID) with
                                    // workgroup-scope atomics, which execute in that XCD's L2 instead of at the memory side (the host passes 0)
    // spec 4 (pattern-aggregated stage 1): non-null -> only the REPRESENTATIVE positions (lowest position of each packed tau word:
    // pat_rep[word] & 0xFFFFFFFF) carry cells, with the counts of all positions of their word summed in pat_x [V][4][S]
    const unsigned long long *pat_rep;
    uint32_t *pat_x;
    const uint32_t *pat_list, *pat_n;   // the representatives of this pass (any order) and their number: stage 1 walks this list
    int dbg;                        // timing experiments only (DESMAN_HIP_STATS_DBG; compiled out of the product kernel: STATS_DBG above): bit 0 no draws, 1 no item seeding, 2 no E/N atomics, 3 no cell Philox
};

__device__ __forceinline__ uint64_t wave_uniform_u64(uint64_t x)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// LPV = lanes per variant: a wavefront works on 64 / LPV (variant, LPV-sample chunk) tasks at a time, so that tables of 16,
// 32, 48 or 96 samples fill its lanes (lane = sample alone leaves 3/4 of a wavefront idle at S = 16 and 1/4 at S = 96).
// SPEC: 2 or 3 (dsm_binom.h).  (gamma in registers instead of the LDS tile: measured slower, 54-57 vs 48-49 us at config 3, and removed)
template <int LPV, int SPEC, bool PAT = false>
__device__ __forceinline__ void stats_agg_body(const StatsAggParams &p)
{
    extern __shared__ __attribute__((aligned(16))) char smem_s[];
    S1_CLK(0);
#ifdef DSM_AB_SWITCHES
    if ((threadIdx.x & 63) == 0 && blockIdx.y == 0)          // where the wavefront runs: HW_REG_HW_ID (wave, SIMD, CU, SH, SE) and the XCC id
        s1_clk[(size_t)(blockIdx.x * 4 + (threadIdx.x >> 6)) * S1_NCLK + 13] =
            ((unsigned long long)(__builtin_amdgcn_s_getreg((31 << 11) | 4)) << 8) | (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u) | (1ull << 63);
#endif
    constexpr int NG = 64 / LPV;
    constexpr int NTAB = SPEC >= 3 ? (2 * DSM_LOG_TAB_N + DSM_EXP_TAB_N) : 0;      // doubles: log table, then exp table
    const int S = p.S, G = p.G, V = p.V;
    const int NCH = (S + LPV - 1) / LPV, SP = NCH * LPV;
    double *tabs = reinterpret_cast<double *>(smem_s);                // [NTAB]
    double *gT = tabs + NTAB;                                         // [G][SP] gamma transposed
    double *rcp = gT + (size_t)G * SP;                                // [256]  1/k
    double *es = rcp + DSM_RCP_TAB_N;                                 // [16]   eta
    uint32_t *eacc = reinterpret_cast<uint32_t *>(es + 16);           // [16][256] lane-private Esum columns
    const double2 *ltab = reinterpret_cast<const double2 *>(tabs);
    const int tid = threadIdx.x, lane = tid & 63;
    const int grp = lane / LPV, lig = lane % LPV;
    const int nwaves = gridDim.x * 4;
    const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (tid >> 6));
    // spec 4: only the representatives carry cells -- the tasks are (entry of the pass's list, chunk); the list is in no
    // particular order (atomic appends), which changes no sum: a cell's stream is keyed by its position, the sums are integers
    const int nunit = PAT ? (int)__builtin_amdgcn_readfirstlane((int)*p.pat_n) : V;
    const int ntask = nunit * NCH;                                    // (variant, chunk of LPV samples)
    const int nslot = (ntask + NG - 1) / NG;                          // NG tasks per wavefront pass
    for (int i = tid; i < G * SP; i += 256) {
        const int g = i / SP, s = i - g * SP;
        gT[i] = (s < S) ? p.gamma[(size_t)s * G + g] : 0.0;
    }
    if constexpr (SPEC >= 3) { for (int i = tid; i < NTAB; i += 256) tabs[i] = p.log_tab[i]; }
    for (int k = tid; k < DSM_RCP_TAB_N; k += blockDim.x) rcp[k] = k ? 1.0 / (double)k : 0.0;
    if (tid < 16) es[tid] = p.eta[tid];
#pragma unroll
    for (int i = 0; i < 16; ++i) eacc[i * 256 + tid] = 0u;
    __syncthreads();

    S1_CLK(1);
    ISA_MARK("slot_setup");
    int s1_pass = 0;
    (void)s1_pass;
    // which copy of the subset table this workgroup adds to
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;                // HW_REG_XCC_ID[3:0] (gfx942 / gfx950)
    const unsigned copy = p.xcd ? xcc + 8u * ((blockIdx.x >> 3) % (unsigned)(p.rep >> 3)) : blockIdx.x % (unsigned)p.rep;
    for (int slot = wid; slot < nslot; slot += nwaves) {
        const int task = slot * NG + grp;
        const bool tv = task < ntask;
        const int u = tv ? task / NCH : 0, j = tv ? task - u * NCH : 0;
        const int v = PAT ? (int)p.pat_list[u] : u;
        const int s = j * LPV + lig;
        const bool active = tv && s < S;
        S1_CLKP(0);
        ISA_MARK("cell_load");
        uint64_t t;
        int4 c = make_int4(0, 0, 0, 0);
        if constexpr (PAT) {
            t = p.tau[v];
            if (active) {
                const uint32_t *xr = p.pat_x + (size_t)v * 4 * S + s;
                c.x = (int)xr[0]; c.y = (int)xr[(size_t)S]; c.z = (int)xr[2 * (size_t)S]; c.w = (int)xr[3 * (size_t)S];
            }
        } else {
            // (issuing a pass's loads one pass ahead -- the first before the tables are staged -- was built and measured in round 6: no
            // difference at any shape, 16 instructions and six registers more: profiles/r06_stats_ab.txt, builds `new` / `nopf`)
            t = p.tau[v];
            if (active) c = reinterpret_cast<const int4 *>(p.cnt_vs)[(size_t)v * S + s];
        }
        // haplotype sets of the four bases and the abundance each base carries in this sample; t is uniform over a lane
        // group, so the base of haplotype g and the branches below are scalar -- one group after the other when the
        // wavefront holds several
        ISA_MARK("cell_gamma");
        uint32_t H0 = 0, H1 = 0, H2 = 0, H3 = 0;
        double G0 = 0.0, G1 = 0.0, G2 = 0.0, G3 = 0.0;
        const double *gcol = gT + s;
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            const uint32_t tlo = __builtin_amdgcn_readlane((uint32_t)t, gi * LPV), thi = __builtin_amdgcn_readlane((uint32_t)(t >> 32), gi * LPV);
            const uint64_t tg = ((uint64_t)thi << 32) | tlo;
            if (NG == 1 || grp == gi) {
                for (int g = 0; g < G; ++g) {
                    const int a = (int)((tg >> (2 * g)) & 3);
                    const double x = gcol[g * SP];
                    const uint32_t bit = 1u << g;
                    if (a == 0) { H0 |= bit; G0 = G0 + x; }
                    else if (a == 1) { H1 |= bit; G1 = G1 + x; }
                    else if (a == 2) { H2 |= bit; G2 = G2 + x; }
                    else { H3 |= bit; G3 = G3 + x; }
                }
            }
        }
        const double Gam[4] = {G0, G1, G2, G3};
        ISA_MARK("cell_philox");
        const uint32_t cell = (uint32_t)s * (uint32_t)p.V_tot + (uint32_t)(p.v_off + v);
        uint32_t cbase[4];
        if (STATS_DBG(p, 8)) { cbase[0] = cell; cbase[1] = p.iter; cbase[2] = p.k0; cbase[3] = p.k1; }
        else philox4x32_10(cell, 0u, p.iter, DSM_STREAM_STA1, p.k0, p.k1, cbase);         // one Philox-10 per cell
        uint32_t nacc[4] = {0, 0, 0, 0};
        S1_CLKP(1);
        // Round 6: the four observed bases are straight-line code (the base is a compile-time constant: the count is a register, the
        // Esum column an immediate offset, no loop counter kept in a vector register, no copies at the loop's back edge), and the rare
        // outcome -- an item handed to the compacted kernel -- is collected in `hand` and tested ONCE per cell below.
        uint32_t hand = 0;                                                  // bit b: item b is handed over; bits 4 + 2 b: its kind
        const uint32_t xs[4] = {(uint32_t)c.x, (uint32_t)c.y, (uint32_t)c.z, (uint32_t)c.w};     // (aggregated counts may pass 2^31)
        auto item = [&](const int b, const uint32_t xb) __attribute__((always_inline)) {
            if (xb > 0) {
                ISA_MARK("item_w");
                double W[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) W[a] = es[a * 4 + b] * Gam[a];
                const double Wt = ((W[0] + W[1]) + W[2]) + W[3];
                if (!(Wt > 0.0)) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) W[a] = Gam[a];
                }
                ISA_MARK("item_seed");
                uint32_t n[4];
                const Xo128 rng = STATS_DBG(p, 2) ? Xo128{cbase[0] + b, cbase[1], cbase[2], cbase[3] | 1u} : item_seed<SPEC>(cbase, (uint32_t)b, p.k0, p.k1);
                bool ok = true;
                int kind = 0;
                if (STATS_DBG(p, 1)) { n[0] = (uint32_t)xb + (uint32_t)(W[0] > W[1]) + rng.s0; n[1] = n[2] = n[3] = 0; }
                else if constexpr (SPEC == 2) ok = s1_item<SPEC>(rng, xb, W, n, rcp, ltab, p.lean_cap, kind);
                else {
                    Xo128 r2 = rng;
                    bool defer = false;
                    mult4<false, SPEC>(r2, xb, W, n, rcp, ltab, defer, p.lean_cap, &kind);
                    ok = !defer;
                }
#ifdef DSM_S1_PAD                  // experiment: DSM_S1_PAD dependent 32-bit adds per item (is the pass VALU-bound?)
                {
                    uint32_t pad = n[0];
#pragma unroll
                    for (int i_ = 0; i_ < DSM_S1_PAD; ++i_) asm volatile("v_add_u32 %0, %0, %1" : "+v"(pad) : "v"(xb));
                    n[0] += (pad == 0x7FFFFFF1u) ? 1u : 0u;
                }
#endif
                ISA_MARK("item_esum");
                if (ok) {
                    // an aggregated count is consumed exactly once -- here, or by the compacted kernel when the item is handed over -- and
                    // whoever consumes it leaves zero behind for the next pass
                    if constexpr (PAT) p.pat_x[((size_t)v * 4 + b) * S + s] = 0u;
                    if (STATS_DBG(p, (4 | 16))) {
#pragma unroll
                        for (int a = 0; a < 4; ++a) nacc[a] += n[a];
                    } else {
                        uint32_t *erow = eacc + (b * 4) * 256 + tid;           // lane-private column: ds_add_u32, never a conflict
#pragma unroll
                        for (int a = 0; a < 4; ++a) { atomicAdd(erow + a * 256, n[a]); nacc[a] += n[a]; }
                    }
                } else hand |= (1u << b) | ((uint32_t)kind << (4 + 2 * b));
            }
        };
        if constexpr (SPEC == 2) { item(0, xs[0]); item(1, xs[1]); item(2, xs[2]); item(3, xs[3]); }
        else {
            // (the table-exp variant keeps the rolled loop: four copies of its item do not fit the 80 registers of six wavefronts per SIMD)
#pragma unroll 1
            for (int b = 0; b < 4; ++b) item(b, (b == 0) ? xs[0] : (b == 1) ? xs[1] : (b == 2) ? xs[2] : xs[3]);
        }
        S1_CLKP(2);
        ISA_MARK("cell_handover");
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(hand != 0u) != 0ull, 0)) {
            // needs the rejection sampler / a long search: the compacted kernel re-does the item from its own stream.  One list per kind
            // of item (and DSM_BIG_NL of each): the wavefronts of the compacted kernel then hold items that take the same path; one
            // atomic per wavefront, base and kind, the lanes that hand over take consecutive slots
#pragma unroll 1
            for (int b = 0; b < 4; ++b) {
                const bool mine = (hand >> b) & 1u;
                const int kind = (int)((hand >> (4 + 2 * b)) & 3u);
#pragma unroll 1
                for (int kd = 0; kd < DSM_BIG_NT; ++kd) {
                    const unsigned long long mask = __builtin_amdgcn_ballot_w64(mine && kind == kd);
                    if (mask == 0ull) continue;
                    const uint32_t sub = (uint32_t)kd * DSM_BIG_NL + blockIdx.x % DSM_BIG_NL;
                    const int leader = __builtin_ctzll(mask);
                    uint32_t base = 0;
                    if (lane == leader) base = atomicAdd(p.big_count + sub * DSM_BIG_STRIDE, (uint32_t)__builtin_popcountll(mask));
                    base = __builtin_amdgcn_readlane(base, leader);
                    const uint32_t slot = base + (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
                    if (mine && kind == kd) p.big_list[(size_t)sub * p.big_seg + slot] = (unsigned long long)cell * 4ull + (unsigned long long)b;
                }
            }
        }
        ISA_MARK("cell_table");
        // N[H_a(v)][s] += reads whose true base is a: adjacent lanes -> adjacent words of one table row
        const size_t ld = (size_t)p.ld;                                    // row stride of the subset table in words (>= S: ensure_ntab)
        uint32_t *const nt = p.ntab + (size_t)copy * (((size_t)1 << G) * ld);
        const uint32_t hmask = (1u << G) - 1u;
        // row of (subset, sample): (H hmul + (s >> 4) swz) mod 2^G -- the subset's part is scalar, the sample's a lane constant of the slot
        const uint32_t sw = ((uint32_t)s >> 4) * p.swz;
        const uint32_t r0 = (H0 * p.hmul + sw) & hmask, r1 = (H1 * p.hmul + sw) & hmask, r2 = (H2 * p.hmul + sw) & hmask, r3 = (H3 * p.hmul + sw) & hmask;
        if (STATS_DBG(p, (4 | 32))) { if ((nacc[0] ^ nacc[1] ^ nacc[2] ^ nacc[3] ^ r0 ^ r1 ^ r2 ^ r3) == 0x12345u) atomicAdd(nt + s, 1u); continue; }
        if (STATS_DBG(p, 64)) {        // plain stores instead of atomics (wrong sums; what the adds cost beyond a store)
            nt[(size_t)r0 * ld + s] = nacc[0]; nt[(size_t)r1 * ld + s] = nacc[1]; nt[(size_t)r2 * ld + s] = nacc[2]; nt[(size_t)r3 * ld + s] = nacc[3];
            continue;
        }
        if (p.xcd) {
            // this XCD's copy: every adder of the copy shares the L2 the atomic executes in (relaxed, workgroup scope: no sc1, the
            // line stays in L2); the kernel boundary writes the lines back for stage 2, which sums the copies
            if (nacc[0]) __hip_atomic_fetch_add(nt + (size_t)r0 * ld + s, nacc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (nacc[1]) __hip_atomic_fetch_add(nt + (size_t)r1 * ld + s, nacc[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (nacc[2]) __hip_atomic_fetch_add(nt + (size_t)r2 * ld + s, nacc[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (nacc[3]) __hip_atomic_fetch_add(nt + (size_t)r3 * ld + s, nacc[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            if (nacc[0]) atomicAdd(nt + (size_t)r0 * ld + s, nacc[0]);
            if (nacc[1]) atomicAdd(nt + (size_t)r1 * ld + s, nacc[1]);
            if (nacc[2]) atomicAdd(nt + (size_t)r2 * ld + s, nacc[2]);
            if (nacc[3]) atomicAdd(nt + (size_t)r3 * ld + s, nacc[3]);
        }
        S1_CLKP(3);
        ++s1_pass;
    }
    S1_CLK(14);
    ISA_MARK("epilogue");
    // Esum: a wavefront's lane-private columns -> one transposing butterfly -> 16 adds to ONE OF DSM_ESUM_PARTS COPIES of Esum (round 6).
    // Rounds 2-5 summed the four wavefronts of a workgroup in LDS (three barriers) and sent 16 adds per workgroup to Esum itself: 1 488
    // workgroups adding to the same two cache lines take their turns at the memory side (~8 ns each), and the wavefronts that left
    // the pass loop last waited 4-5 us for the launch's final adds -- 10 % of the launch at config 3 (wave time stamps,
    // profiles/r06_stats_timeline.txt).  A copy takes 1/64 of the adds, no wavefront waits for another, and the consumer (the eta
    // rows of dirichlet_kernel; esum_fold_kernel on the API paths) sums the copies and leaves them zero.
    {
        uint32_t e[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) e[i] = eacc[i * 256 + tid];
        const uint32_t tot = wave_transpose_reduce<16>(e);
        const int idx = transpose_index<16>(lane);
        if (lane < 16 && tot) atomicAdd(&p.esum[16 + ((unsigned)wid % DSM_ESUM_PARTS) * 16 + idx], (unsigned long long)tot);
    }
    S1_CLK(15);
}

// six wavefronts per SIMD (the persistent grid's six workgroups per CU): the register allocation must leave room for them
template <int LPV, int SPEC>
__global__ __launch_bounds__(256, 6) void stats_agg_kernel(StatsAggParams p) { stats_agg_body<LPV, SPEC>(p); }
template <int LPV>      // (five workgroups per CU: at six the 16- and 32-lane forms spill)
__global__ __launch_bounds__(256, 5) void stats_pat_kernel(StatsAggParams p) { stats_agg_body<LPV, 2, true>(p); }

// ---- spec 4: the two small passes ahead of stage 1 ------------------------------------------------------------------------
// Cells (v, s) and (v', s) of positions with the same packed tau word have the same weights W_a = eta[a,b] Gamma_a for every
// observed base b, and only sums over positions are consumed (Esum, N[H][s]): Multinomial(x; W) + Multinomial(x'; W) is
// Multinomial(x + x'; W), so the counts are summed per (word, sample, base) first and stage 1 runs once per word instead of once per
// position -- the same law (oracle twin: cbind.stats_agg(spec=4) sums the counts the same way and calls the spec-2 code), other draws.
// Which position stands for a word must not depend on the order the hardware runs things in (the cell's Philox key is built from
// it): the LOWEST position carrying the word, found by atomicMin.  Table entries are (~generation << 32 | position): a later pass
// always writes smaller values than anything an earlier one left, so the table is never cleared.
__global__ __launch_bounds__(256) void pat_rep_kernel(const uint64_t *__restrict__ tau, int V, int G, unsigned long long *__restrict__ rep, uint32_t hi)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    atomicMin(&rep[tau[v] & ((1ull << (2 * G)) - 1ull)], ((unsigned long long)hi << 32) | (unsigned long long)(uint32_t)v);
}
// up to 4096 words (G <= 6): thousands of positions per word would queue on the same few addresses (16 words in two cache lines at
// G = 2: ~100 us for V = 50k), so a 1024-thread workgroup takes the minimum of its share of the positions in LDS first and sends
// one atomicMin per word it met
__global__ __launch_bounds__(1024) void pat_rep_lds_kernel(const uint64_t *__restrict__ tau, int V, int G, unsigned long long *__restrict__ rep, uint32_t hi)
{
    __shared__ uint32_t lo[4096];
    const int words = 1 << (2 * G), tid = threadIdx.x;
    for (int i = tid; i < words; i += 1024) lo[i] = 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t mask = (1ull << (2 * G)) - 1ull;
    for (int v = blockIdx.x * 1024 + tid; v < V; v += gridDim.x * 1024) atomicMin(&lo[tau[v] & mask], (uint32_t)v);
    __syncthreads();
    for (int i = tid; i < words; i += 1024)
        if (lo[i] != 0xFFFFFFFFu) atomicMin(&rep[i], ((unsigned long long)hi << 32) | (unsigned long long)lo[i]);
}
// Few words (G <= 3 with 64-sample chunks, G = 4 with 32-sample chunks): thousands of positions add to the same few blocks, and
// same-address global atomics resolve one after the other (V = 50k, S = 96: 248 us at G = 2, 153 at G = 3 with pat_agg_kernel).
// Here a 1024-thread workgroup pools its share of the positions in LDS first -- table [4^G][4][LPW], indexed by the word itself, so
// no look-up on the way in -- and adds the table to the representatives' blocks once at the end: workgroups x 4^G x 4 LPW global
// atomics instead of V x S x 4.  LPW = lanes per position (64: one position per wavefront pass; 32: two).
template <int LPW>
__global__ __launch_bounds__(1024) void pat_agg_lds_kernel(const int32_t *__restrict__ cnt_vs, const uint64_t *__restrict__ tau, int V, int S, int G,
                                                           const unsigned long long *__restrict__ rep, uint32_t *__restrict__ x, int nvsplit)
{
    extern __shared__ uint32_t ptab[];                       // [words][4][LPW]
    const int words = 1 << (2 * G);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < words * 4 * LPW; i += 1024) ptab[i] = 0u;
    __syncthreads();
    constexpr int PPW = 64 / LPW;                            // positions per wavefront pass
    const int chunk = (int)blockIdx.x / nvsplit, part = (int)blockIdx.x % nvsplit;      // sample chunk, share of the positions
    const int s = chunk * LPW + (lane % LPW);
    const uint64_t mask = (1ull << (2 * G)) - 1ull;
    for (int v0 = (part * 16 + wv) * PPW; v0 < V; v0 += nvsplit * 16 * PPW) {
        const int v = v0 + lane / LPW;
        if (v < V && s < S) {
            const int4 c = reinterpret_cast<const int4 *>(cnt_vs)[(size_t)v * S + s];
            uint32_t *row = ptab + (size_t)(tau[v] & mask) * 4 * LPW + (lane % LPW);
            if (c.x) atomicAdd(row, (uint32_t)c.x);
            if (c.y) atomicAdd(row + LPW, (uint32_t)c.y);
            if (c.z) atomicAdd(row + 2 * LPW, (uint32_t)c.z);
            if (c.w) atomicAdd(row + 3 * LPW, (uint32_t)c.w);
        }
    }
    __syncthreads();
    for (int i = tid; i < words * 4 * LPW; i += 1024) {
        const uint32_t n = ptab[i];
        if (!n) continue;
        const int w = i / (4 * LPW), b = (i / LPW) & 3, sl = chunk * LPW + i % LPW;
        atomicAdd(x + ((size_t)(uint32_t)rep[w] * 4 + b) * S + sl, n);      // (n != 0: some position carries the word, so it has a representative)
    }
}

// the representatives of the pass as a list (one thread per word; appended in whatever order the atomics resolve): stage 1 then has
// an even share of them per wavefront -- walking the positions instead, the lowest positions of the words (all within the first few
// thousand) made a few wavefronts do most of the work (V = 50k, S = 96, G = 6: 175 us).  The counter of the NEXT pass is cleared here.
__global__ __launch_bounds__(256) void pat_list_kernel(const unsigned long long *__restrict__ rep, int words, uint32_t hi, uint32_t *__restrict__ list,
                                                       uint32_t *__restrict__ n_this, uint32_t *__restrict__ n_next)
{
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w == 0) *n_next = 0u;
    if (w >= words) return;
    const unsigned long long e = rep[w];
    if ((uint32_t)(e >> 32) == hi) list[atomicAdd(n_this, 1u)] = (uint32_t)e;
}

// thread = (position, sample): the slab's four counts are added to the representative's [4][S] block -- lanes are consecutive samples,
// so an instruction's atomics fall on consecutive words.  Integer sums: the order of the adds changes nothing.
__global__ __launch_bounds__(256) void pat_agg_kernel(const int32_t *__restrict__ cnt_vs, const uint64_t *__restrict__ tau, int V, int S, int G,
                                                      const unsigned long long *__restrict__ rep, uint32_t *__restrict__ x)
{
    const size_t n = (size_t)V * S;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int v = (int)(i / (size_t)S), s = (int)(i - (size_t)v * S);
        const int4 c = reinterpret_cast<const int4 *>(cnt_vs)[i];
        const uint32_t r = (uint32_t)rep[tau[v] & ((1ull << (2 * G)) - 1ull)];
        uint32_t *xr = x + (size_t)r * 4 * S + s;
        if (c.x) atomicAdd(xr, (uint32_t)c.x);
        if (c.y) atomicAdd(xr + S, (uint32_t)c.y);
        if (c.z) atomicAdd(xr + 2 * (size_t)S, (uint32_t)c.z);
        if (c.w) atomicAdd(xr + 3 * (size_t)S, (uint32_t)c.w);
    }
}
template <int LPV, int SPEC>
__global__ __launch_bounds__(256, 6) void stats_agg_kernel_b(BatchArgs<StatsAggParams> b) { stats_agg_body<LPV, SPEC>(b.p[blockIdx.y]); }
template <int LPV>
__global__ __launch_bounds__(256, 5) void stats_pat_kernel_b(BatchArgs<StatsAggParams> b) { stats_agg_body<LPV, 2, true>(b.p[blockIdx.y]); }

// ---------------------------------------------------------------------------------------------------
// the deferred items (rarer outcome with a mean above 64: burn-in states, very deep data), one lane per item:
// the same arithmetic as stats_agg_kernel with the full sampler (BTRS).  tau_v differs from lane to lane here,
// so the haplotype sets / abundances are built with vector selects.
// ---------------------------------------------------------------------------------------------------
template <int SPEC>
__device__ __forceinline__ void stats_big_body(const StatsAggParams &p)
{
    __shared__ double2 ltab[DSM_LOG_TAB_N + DSM_EXP_TAB_N / 2];          // log table, then the exp table (dsm_binom.h: binom)
    __shared__ double rcp[DSM_RCP_TAB_N];
    __shared__ double es[16];
    __shared__ unsigned long long acc[16];
    __shared__ uint32_t eacc[16 * 256];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t sub = blockIdx.x % (DSM_BIG_NT * DSM_BIG_NL), bi = blockIdx.x / (DSM_BIG_NT * DSM_BIG_NL), nb = gridDim.x / (DSM_BIG_NT * DSM_BIG_NL);
    const uint32_t nbig = p.big_count[sub * DSM_BIG_STRIDE];
    if (bi * 256u >= nbig) return;
    const unsigned long long *list = p.big_list + (size_t)sub * p.big_seg;
    ltab[tid] = reinterpret_cast<const double2 *>(p.log_tab)[tid];
    if (tid < DSM_EXP_TAB_N / 2) ltab[DSM_LOG_TAB_N + tid] = reinterpret_cast<const double2 *>(p.log_tab)[DSM_LOG_TAB_N + tid];
    for (int k = tid; k < DSM_RCP_TAB_N; k += blockDim.x) rcp[k] = k ? 1.0 / (double)k : 0.0;
    if (tid < 16) { es[tid] = p.eta[tid]; acc[tid] = 0ull; }
#pragma unroll
    for (int i = 0; i < 16; ++i) eacc[i * 256 + tid] = 0u;
    __syncthreads();
    BigItemParams bp;
    bp.cnt_vs = p.cnt_vs; bp.tau = p.tau; bp.gamma = p.gamma; bp.pat_x = p.pat_x; bp.ntab = p.ntab; bp.rep = p.rep; bp.ld = p.ld;
    bp.S = p.S; bp.G = p.G; bp.v_off = p.v_off; bp.V_tot = p.V_tot; bp.k0 = p.k0; bp.k1 = p.k1; bp.iter = p.iter; bp.hmul = p.hmul; bp.swz = p.swz;
    for (uint32_t i = bi * 256u + tid; i < nbig; i += nb * 256u) {
        uint32_t n[4];
        const int b = big_item_draw<SPEC>(bp, list[i], blockIdx.x, es, rcp, ltab, n);
        uint32_t *erow = eacc + (b * 4) * 256 + tid;
#pragma unroll
        for (int a = 0; a < 4; ++a) erow[a * 256] += n[a];
    }
    {
        uint32_t e[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) e[i] = eacc[i * 256 + tid];
        const uint32_t tot = wave_transpose_reduce<16>(e);
        const int idx = transpose_index<16>(lane);
        if (lane < 16 && tot) atomicAdd(&acc[idx], (unsigned long long)tot);
    }
    __syncthreads();
    if (tid < 16 && acc[tid]) atomicAdd(&p.esum[tid], acc[tid]);
    // a consumed list is left empty: the last of the list's workgroups to get here (every one that had items read the counter before it
    // drew its ticket) clears the counter and notes that the pass handed items over.  The launch that runs stage 2 finds all counters zero
    // and goes its usual way; where this launch was left out it finds the items and draws them itself (dsm_stage2.h: s2_inline_items).
    if (tid == 0) {
        const uint32_t nwg = min(nb, (nbig + 255u) / 256u);
        uint32_t *cw = p.big_count + sub * DSM_BIG_STRIDE;
        if (atomicAdd(cw + DSM_BIG_W_TICKET, 1u) == nwg - 1u) { cw[DSM_BIG_W_TICKET] = 0u; cw[0] = 0u; atomicAdd(p.big_count + DSM_BIG_W_SEEN, 1u); }
    }
}

// the copies of Esum stage 1 adds to (stats_agg_body's last lines) -> Esum, copies zero again.  The Gibbs loop never launches this: the
// eta rows of dirichlet_kernel do the same sum on their way in.  For the paths that read Esum otherwise (dsm_ctx_sample_stats,
// dsm_ctx_debug_stage1, the exchange of a chain sharded by positions).
__global__ __launch_bounds__(256) void esum_fold_kernel(unsigned long long *__restrict__ esum)
{
    static_assert(DSM_ESUM_PARTS * 4 == 256, "one thread per (copy, group of four counters)");
    const int k = threadIdx.x >> 2, q = threadIdx.x & 3;
    unsigned long long *pp = esum + 16 + k * 16 + q * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned long long v = pp[i];
        if (v) { pp[i] = 0ull; atomicAdd(&esum[q * 4 + i], v); }
    }
}
int k_esum_fold(dsm_ctx *c)
{
    hipLaunchKernelGGL(esum_fold_kernel, dim3(1), dim3(256), 0, c->stream, c->esum);
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}

template <int SPEC>
__global__ __launch_bounds__(256) void stats_big_kernel(StatsAggParams p) { stats_big_body<SPEC>(p); }
template <int SPEC>
__global__ __launch_bounds__(256) void stats_big_kernel_b(BatchArgs<StatsAggParams> b) { stats_big_body<SPEC>(b.p[blockIdx.y]); }

#include "dsm_stage2.h"

struct Stage2Batch { Stage2Params p[DSM_MAX_BATCH]; S2Lists ls[DSM_MAX_BATCH]; S2Plan plan; };
template <int SPEC>
__global__ __launch_bounds__(1024) void stats_stage2_kernel(Stage2Params p, S2Plan plan, S2Lists ls)
{
    __shared__ __attribute__((aligned(16))) char smem2[S2_SMEM_BYTES];
    stage2_sample<SPEC>(p, plan, (int)blockIdx.x / p.nsplit, smem2, true, (int)blockIdx.x % p.nsplit, ls);
}
template <int SPEC>
__global__ __launch_bounds__(1024) void stats_stage2_kernel_b(Stage2Batch b)
{
    __shared__ __attribute__((aligned(16))) char smem2[S2_SMEM_BYTES];
    stage2_sample<SPEC>(b.p[blockIdx.y], b.plan, blockIdx.x, smem2, true, 0, b.ls[blockIdx.y]);
}

// test hook: variate i of a sampler from the stream Philox({i, 0, 0, 'TEST'})  (oracle: orc_binom_test / orc_mult4_test)
template <int SPEC>
__global__ __launch_bounds__(256) void binom_test_kernel(int kind, uint32_t n, double wa, double wb, double w2, double w3,
                                                         uint32_t k0, uint32_t k1, int nsamp, const double *log_tab,
                                                         uint32_t *out)
{
    __shared__ double2 ltab[DSM_LOG_TAB_N + DSM_EXP_TAB_N / 2];
    __shared__ double rcp[DSM_RCP_TAB_N];
    const int tid = threadIdx.x;
    ltab[tid] = reinterpret_cast<const double2 *>(log_tab)[tid];
    if (tid < DSM_EXP_TAB_N / 2) ltab[DSM_LOG_TAB_N + tid] = reinterpret_cast<const double2 *>(log_tab)[DSM_LOG_TAB_N + tid];
    for (int k = tid; k < DSM_RCP_TAB_N; k += blockDim.x) rcp[k] = k ? 1.0 / (double)k : 0.0;
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    if (i >= nsamp) return;
    Xo128 rng = xo_seed((uint32_t)i, 0u, 0u, DSM_STREAM_TEST, k0, k1);
    bool dummy = false;
    if (kind != 2) out[i] = binom<true, SPEC>(rng, n, wa, wb, rcp, ltab, dummy, kind == 0 ? DSM_BINV_MEAN_CAP : DSM_BINV_MEAN_CAP_S2);
    else {
        const double W[4] = {wa, wb, w2, w3};
        uint32_t m[4];
        mult4<true, SPEC>(rng, n, W, m, rcp, ltab, dummy);
        out[i * 4 + 0] = m[0]; out[i * 4 + 1] = m[1]; out[i * 4 + 2] = m[2]; out[i * 4 + 3] = m[3];
    }
}

// =====================================================================
// host side
// =====================================================================
// spec v2 applies when the subset table fits (G <= 16, 2^G * S * 4 B <= 64 MB, every sample's depth < 2^32).  Where both
// apply the cheaper one runs, by a cost model of the two passes fitted on MI355X (us per iteration, 933 x 64 ... 50k x 96):
//   per-read pass (v1)   25 + (0.25 + 0.02 G + 0.0029 G^2) per million reads   -- O(depth x G): 0.30 at G = 2, 0.60 at 8, 1.31 at 16
//   aggregated pass (v2) 24 + 0.062 per thousand cells + 14 + 0.03 x 3V / 2^G (one table; ~0 with copies)   -- O(cells); cells = V x S rounded up to
//                        the kernel's lane groups; + 14 for stage 2 in the Dirichlet launch (G >= 10: its own launch over
//                        2^G subsets per sample, + 0.012 x 2^G); the last term is the
//                        same-address contention of the subset-table atomics (3 per cell onto 2^G x S counters: 9 375 per
//                        counter at V = 50k, G = 4 -> 410 us; 117 at config 3), spread over rep copies of the table
//                        (stats_ntab_rep below)
// so shallow data (< ~100 reads per cell) and problems below ~200k cells keep the per-read pass.
// The rule is a function of the shape and the read totals only: the same on every run and every GPU.
// lanes per variant of stats_agg_kernel: the chunk size that pads S least (ties: the larger one)
static int stats_agg_lpv(int S)
{
    int best = 64;
    for (int l : {32, 16}) if ((S + l - 1) / l * l < (S + best - 1) / best * best) best = l;
    return best;
}

int stats_spec(const dsm_ctx *c)
{
    int force = c->force_stats_spec;
    if (force == 0) {                       // DESMAN_HIP_STATS_SPEC=1|2: the choice for every context that has none of its own
        const char *e = getenv("DESMAN_HIP_STATS_SPEC");   // (2 = the draws of a batched run, also for chains run one by one)
        if (e && (e[0] == '1' || e[0] == '2' || e[0] == '3' || e[0] == '4') && e[1] == 0) force = e[0] - '0';
    }
    if (force == 1) return 1;
    if (c->G < 1 || c->G > 16) return 1;
    if (((size_t)1 << c->G) * (size_t)c->S * 4 > ((size_t)64 << 20)) return 1;
    if (c->max_depth >= ((uint64_t)1 << 32)) return 1;
    // spec 4 = spec 2's samplers over tau PATTERNS (positions sharing their packed word share a cell per sample; pat_rep_kernel above).
    // It needs the direct-address table of 4^G words (G <= 8) and a chain that is not sharded by positions (representatives would be
    // per shard: a sharded chain is the unsharded chain UNDER SPEC 2, desman_amd/vshard.py); asked for where it does not apply, spec 2
    // runs.  A batch runs what its chains would run alone (round 5: the pooling passes chain by chain, stage 1 over the words as one launch).
    const bool pat_ok = c->G <= 8 && !c->shard_on;
    if (force == 4) return pat_ok ? 4 : 2;
    if (force >= 2) return force;                        // 2 = the default version of the aggregated draws, 3 = the table exp/log variant
    double reads = 0.0;
    for (int64_t d : c->depth) reads += (double)d;
    const int lpv = stats_agg_lpv(c->S);
    const double cells = (double)c->V * (double)((c->S + lpv - 1) / lpv * lpv);
    const double g = (double)c->G;
    const double t1 = 25.0 + (0.25 + 0.02 * g + 0.0029 * g * g) * 1e-6 * reads;    // per read: its uniform + G - 1 threshold tests (0.30 / 0.60 / 1.31 at G = 2 / 8 / 16)
    const double stage2 = 14.0 + (c->G >= 10 ? 0.012 * (double)(1u << c->G) : 0.0);      // its own launch from G = 10: 62 us at G = 12
    const int rep = stats_ntab_rep(c);
    const double per = 3.0 * (double)c->V / (double)(1u << c->G);                // atomics per counter of the subset table
    const double t2 = 24.0 + stage2 + 0.062e-3 * cells + (rep == 1 ? 0.03 * per : 0.003 * per / rep);   // with copies: no measurable penalty
    // over tau words (spec 4): one more pass over the counts (~60 us per 77 MB incl. its atomics) + two small launches, then stage 1 over
    // the words the chain's tau actually holds instead of its V positions.  What it saves is stage 1's per-cell work, not its
    // per-error-read work (the pooled cells hold the same reads), so it pays on large tables with few words -- and most where stage 1 is
    // most expensive, in the chains of a G-sweep that have fewer haplotypes than the table has strains.  Measured, ms per iteration,
    // spec 4 vs 2 (profiles/r04_misfit_scan_spec4.txt): six-strain 50k x 96 table G = 2 0.14 vs 0.91, 3 0.21 vs 0.84, 4 0.27 vs 0.42,
    // 5 0.33 vs 0.44, 6 0.34 vs 0.47, 7 0.41 vs 0.49, 8 0.42 vs 0.51 (at 7 and 8 the six real strains keep the words few although
    // 4^G > V); four-strain 20k x 64: 0.10 vs 0.22, 0.15 vs 0.18, then 0.16 vs 0.13, 0.17 vs 0.14; 10k x 64: 0.10 vs 0.12, 0.13 vs 0.12,
    // 0.14 vs 0.09.  A table whose words are all different pays the pooling pass for nothing (+12 % at 50k x 96).  The rule -- shape
    // only, like everything here: G <= 2 from half a million cells, G = 3 from a million, G = 4 ... 8 from 2.5 million cells where
    // even 64 x 2^G words (several times what biallelic positions can form: 12 (2^G - 2) + 4) stay below V.  Anything else can ask for
    // it (dsm_ctx_force_stats_spec(4), DESMAN_HIP_STATS_SPEC=4).
    if (pat_ok && force == 0 && t2 < t1) {
        const bool small_g = (c->G <= 2 && cells >= 0.5e6) || (c->G == 3 && cells >= 1.0e6);
        const bool mid_g = c->G >= 4 && cells >= 2.5e6 && 64.0 * (double)((size_t)1 << c->G) <= (double)c->V;
        if (small_g || mid_g) return 4;
    }
    return t2 < t1 ? DSM_STATS_AGG : 1;
}

// Few subsets and many positions put thousands of atomics on every counter of the subset table (3 V / 2^G each: 9 375 at
// V = 50k, G = 4 -- 410 us of same-address serialisation).  The table is then kept in `rep` copies, workgroup b adds to copy
// b mod rep and stage 2 reads their sum: integers, so nothing changes but the time.  What decides is the rate of atomics per
// 64 B line of the table(s): stage 1 issues 3 per cell and takes ~0.06 us per thousand cells, so the rate is ~48 000 /
// (lines x rep) per us whatever V is, and the measurements (scripts/shape_scan.py) put the knee at
// lines x rep ~ 300: V = 100k, S = 64, G = 2 (16 lines) 585 us with 16 copies, 304 with 32; V = 50k, S = 96, G = 5 (192 lines)
// 472 us with one table, 300 with two; V = 20k, S = 32, G = 5 (64 lines) 0.127 ms per iteration with two copies, 0.094 with
// sixteen.  So: one table while a counter takes <= 128 atomics (config 3: 117, config 5: 37); otherwise at least two copies
// (V = 20k, S = 64, G = 8: 145 -> 88 us) and as many as bring lines x rep to 384 -- every copy is one more read per subset at
// stage 2's root (64 copies: +20 us on the Dirichlet launch).
int stats_ntab_rep(const dsm_ctx *c)
{
    // a chain sharded by positions: every rank must lay its table out alike (the tables are all-reduced element by element), so
    // the rule reads the WHOLE table's position count, never the shard's own (shards differ by one position: V = 21 845, G = 8 on
    // two ranks gave 10 922 -> one copy and 10 923 -> two).  More copies than a shard needs cost one read each at stage 2's root.
    const double per = 3.0 * (double)(c->shard_on ? c->shard_vtot : c->V) / (double)((size_t)1 << c->G);
    if (per <= 128.0) return 1;
    const double lines = (double)((((size_t)1 << c->G) * (size_t)c->S * 4 + 63) / 64);
    int rep = 2;
    while (lines * rep < 384.0 && rep < 64 && (size_t)(2 * rep) * ((size_t)1 << c->G) * (size_t)c->S * 4 <= ((size_t)64 << 20)) rep *= 2;
    return rep;
}

// The subset table's row map: row of (subset H, sample s) = (H DSM_NTAB_HMUL + (s >> 4) DSM_NTAB_SWZ) mod 2^G (dsm_host.h).  The odd
// multiplier scatters the low-popcount subsets that take most of stage 1's atomics; the sample's part puts the four 64 B lines of a
// subset's 64 samples into four different rows.  Together they make every place of the table cost the same: stage 1 40.5 us at config 3
// at each of eight places, where the identity map had 45-47 us at the good ones and 55-59 at the bad (profiles/r06_swz_scan.txt).  So the
// table is allocated and zeroed once per layout and freed with its chain; rows are S words.  A copy per XCD, padded rows, other row maps
// and a place measured per table were tried and removed.
void stats_release_ntab(dsm_ctx *c)
{
    if (c->ntab_raw) (void)hipFree(c->ntab_raw);
    c->ntab_raw = nullptr; c->ntab = nullptr; c->ntab_len = 0;
}
static int ensure_ntab(dsm_ctx *c)
{
    const int rep = stats_ntab_rep(c), ld = c->S;
    const size_t need = (size_t)rep * ((size_t)1 << c->G) * (size_t)ld;
    if (c->ntab && c->ntab_len == need && c->ntab_ld == ld && c->ntab_rep == rep) return DSM_OK;
    stats_release_ntab(c);
    c->ntab_rep = rep; c->ntab_ld = ld;
    // test hook of the experiment build: DESMAN_HIP_NTAB_OFF=<bytes> starts the table that far (in 256 B steps) past its 4 KB-aligned base
    const char *eo = DSM_AB_ENV("DESMAN_HIP_NTAB_OFF");
    const size_t off = eo ? ((size_t)strtoull(eo, nullptr, 0) & ~(size_t)255) : 0;
    const size_t spare = off + 4096;
    hipError_t e = hipMalloc((void **)&c->ntab_raw, need * sizeof(uint32_t) + spare);
    if (e != hipSuccess) { dsm_set_error("hipMalloc(%zu B) failed: %s", need * 4 + spare, hipGetErrorString(e)); return DSM_ERR_NOMEM; }
    c->ntab = reinterpret_cast<uint32_t *>(((uintptr_t)c->ntab_raw + 4095) & ~(uintptr_t)4095) + off / 4;
    c->ntab_len = need;
    HIP_TRY(hipMemsetAsync(c->ntab, 0, need * sizeof(uint32_t), c->stream));
    return DSM_OK;
}

int stats_ensure_ntab(dsm_ctx *c)
{
    return stats_spec(c) < 2 ? DSM_OK : ensure_ntab(c);
}

static int ensure_big_list(dsm_ctx *c, size_t seg)
{
    const size_t need = seg * DSM_BIG_NT * DSM_BIG_NL;
    if (c->big_list && c->big_cap == need) return DSM_OK;
    if (c->big_list) { (void)hipFree(c->big_list); c->big_list = nullptr; }
    if (!c->big_count) {
        hipError_t e = hipMalloc((void **)&c->big_count, DSM_BIG_NT * DSM_BIG_NL * DSM_BIG_STRIDE * sizeof(uint32_t));
        if (e != hipSuccess) { dsm_set_error("hipMalloc failed: %s", hipGetErrorString(e)); return DSM_ERR_NOMEM; }
    }
    hipError_t e = hipMalloc((void **)&c->big_list, need * sizeof(unsigned long long));
    if (e != hipSuccess) { dsm_set_error("hipMalloc(%zu B) failed: %s", need * 8, hipGetErrorString(e)); return DSM_ERR_NOMEM; }
    c->big_cap = need;
    // the counters are zero between passes: whoever consumes a list leaves it empty (stats_big_body; dsm_stage2.h: s2_lists_close)
    HIP_TRY(hipMemsetAsync(c->big_count, 0, DSM_BIG_NT * DSM_BIG_NL * DSM_BIG_STRIDE * sizeof(uint32_t), c->stream));
    c->big_seen = 0; c->big_hot = true;              // (the running count went with them)
    return DSM_OK;
}

// Where the launch of stats_big_kernel is a choice.  Chains with G >= 10 (stage 2 as its own 1024-thread launch), the per-read pass
// (specification 1), stage 1 over tau words (4), chains sharded by positions (the tables are exchanged between the two stages) and the
// held and fixed-tau chains (api.hip: gibbs_update) keep the launch unconditionally.
bool stats_big_optional(const dsm_ctx *c)
{
    const int spec = stats_spec(c);
    return (spec == 2 || spec == 3) && c->G < 10 && !c->shard_on;
}
int stats_big_mode(const dsm_ctx *c)
{
    int mode = c->big_launch_mode;
    if (mode == -1) {                       // DESMAN_HIP_BIG_LAUNCH=0|1: the choice for every context that has none of its own
        const char *e = getenv("DESMAN_HIP_BIG_LAUNCH");
        if (e && (e[0] == '0' || e[0] == '1') && e[1] == 0) mode = e[0] - '0';
    }
    return mode;
}
bool stats_big_wanted(const dsm_ctx *c)
{
    const int mode = stats_big_mode(c);
    return mode == -1 ? c->big_hot : mode == 1;
}
void stats_big_take(dsm_ctx *c, uint32_t seen)
{
    c->big_hot = seen != c->big_seen;
    c->big_seen = seen;
}
// what the launch that runs stage 2 needs to draw deferred items itself -- where it can: one workgroup per sample (G < 10), the counts
// themselves (not the pooled ones of specification 4), positions not sharded
void stats_s2_lists(const dsm_ctx *c, Stage2Params *p)
{
    p->big_list = nullptr; p->cnt_vs = nullptr; p->tau = nullptr; p->eta = nullptr; p->big_seg = 0; p->V = c->V;
    const size_t seg = c->big_cap / (DSM_BIG_NT * DSM_BIG_NL);
    if (!stats_big_optional(c) || !c->big_list || !c->big_count || seg > 0xFFFFFFFFull) return;
    p->big_list = c->big_list; p->big_seg = (uint32_t)seg; p->cnt_vs = c->cnt_vs; p->tau = c->tau; p->eta = c->eta;
}

// spec 4: the word table (4^G entries, all ones = "no pass has written here") and the aggregated counts (zero between passes)
static int ensure_pat(dsm_ctx *c)
{
    const size_t nrep = (size_t)1 << (2 * c->G), nx = (size_t)c->V * 4 * (size_t)c->S;
    if (!c->pat_rep || c->pat_rep_len != nrep) {
        if (c->pat_rep) { (void)hipFree(c->pat_rep); c->pat_rep = nullptr; }
        hipError_t e = hipMalloc((void **)&c->pat_rep, nrep * sizeof(unsigned long long));
        if (e != hipSuccess) { dsm_set_error("hipMalloc(%zu B) failed: %s", nrep * 8, hipGetErrorString(e)); return DSM_ERR_NOMEM; }
        c->pat_rep_len = nrep;
        c->pat_gen = 0;
        HIP_TRY(hipMemsetAsync(c->pat_rep, 0xFF, nrep * sizeof(unsigned long long), c->stream));
    }
    if (!c->pat_list || c->pat_rep_len != nrep || c->pat_gen == 0) {
        if (c->pat_list) { (void)hipFree(c->pat_list); c->pat_list = nullptr; }
        hipError_t e = hipMalloc((void **)&c->pat_list, (nrep + 2) * sizeof(uint32_t));
        if (e != hipSuccess) { dsm_set_error("hipMalloc(%zu B) failed: %s", (nrep + 2) * 4, hipGetErrorString(e)); return DSM_ERR_NOMEM; }
        HIP_TRY(hipMemsetAsync(c->pat_list + nrep, 0, 2 * sizeof(uint32_t), c->stream));
    }
    if (!c->pat_x || c->pat_x_len != nx) {
        if (c->pat_x) { (void)hipFree(c->pat_x); c->pat_x = nullptr; }
        hipError_t e = hipMalloc((void **)&c->pat_x, nx * sizeof(uint32_t));
        if (e != hipSuccess) { dsm_set_error("hipMalloc(%zu B) failed: %s", nx * 4, hipGetErrorString(e)); return DSM_ERR_NOMEM; }
        c->pat_x_len = nx;
        HIP_TRY(hipMemsetAsync(c->pat_x, 0, nx * sizeof(uint32_t), c->stream));
    }
    return DSM_OK;
}

int k_stats_stage1(dsm_ctx *c, uint32_t iter, bool launch_big)
{
    int r = ensure_ntab(c);
    if (r != DSM_OK) return r;
    const int S = c->S, G = c->G, V = c->V;
    const int LPV = stats_agg_lpv(S);
    const int NCH = (S + LPV - 1) / LPV, SP = NCH * LPV, NG = 64 / LPV;
    const int spec_full = stats_spec(c);                  // 2, 3 or 4 (the caller checked that the aggregated pass applies)
    const bool pat = spec_full == 4;
    const int spec = stats_draw_version(spec_full);
    const size_t sh = ((size_t)G * SP + (spec >= 3 ? 2 * DSM_LOG_TAB_N + DSM_EXP_TAB_N : 0) + DSM_RCP_TAB_N + 16) * sizeof(double) +
                      16 * 256 * sizeof(uint32_t);
    if (sh > 160 * 1024) { dsm_set_error("stats_agg: gamma tile (%zu B) exceeds LDS", sh); return DSM_ERR_UNSUPPORTED; }
    // the instantiation of this shape and specification: {single, batched}
    const void *fn = nullptr, *fn_b = nullptr;
#define AGG_CASE(L, SP_) if (LPV == L && spec == SP_) { fn = (const void *)stats_agg_kernel<L, SP_>; fn_b = (const void *)stats_agg_kernel_b<L, SP_>; }
    AGG_CASE(16, 2) AGG_CASE(32, 2) AGG_CASE(64, 2) AGG_CASE(16, 3) AGG_CASE(32, 3) AGG_CASE(64, 3)
#undef AGG_CASE
    if (pat) {
        fn = LPV == 16 ? (const void *)stats_pat_kernel<16> : LPV == 32 ? (const void *)stats_pat_kernel<32> : (const void *)stats_pat_kernel<64>;
        fn_b = LPV == 16 ? (const void *)stats_pat_kernel_b<16> : LPV == 32 ? (const void *)stats_pat_kernel_b<32> : (const void *)stats_pat_kernel_b<64>;
    }
    if (!fn) { dsm_set_error("stats_agg: no kernel for spec %d", spec); return DSM_ERR_UNSUPPORTED; }
    if (c->stats_grid == 0 || c->stats_grid_key != spec_full) {
        int occ = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 256, sh));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, c->device));
        const int wgs = std::min(6, std::max(1, occ));      // six workgroups per CU: measured optimum (below)
        // ... on all CUs but one per XCD when the sweep's uniforms are MT19937 words: the generator's workgroup keeps a CU to itself
        // (kernels_gibbs.hip: k_mt_fill) and workgroups go to the XCDs in turn whatever room they have, so a persistent grid sized for
        // every CU leaves six workgroups of that XCD waiting for others to finish -- a launch that starts while the generator runs took
        // 51 us instead of 46 (scripts/dbg/trace_stats_vs_mt.sh).  Leaving 8 CUs: 106.7 vs 107.5 us per iteration at config 3 (1 CU: no
        // change; 16 and more: slower).
        const int n_xcd = prop.multiProcessorCount % 8 == 0 && prop.multiProcessorCount >= 64 ? 8 : 1;
        // (only while a wavefront makes a pass or two: over many passes the smaller grid is simply 3 % less machine -- config 5, twelve
        // passes: 384 vs 368 us)
        const long passes4 = (((long)V * NCH + NG - 1) / NG) / std::max(1L, (long)wgs * prop.multiProcessorCount);   // workgroup = 4 wavefronts: passes x 4
        const int leave = (c->tau_rng == DSM_RNG_MT19937 && passes4 <= 12) ? n_xcd : 0;
        c->stats_grid = wgs * std::max(1, prop.multiProcessorCount - leave);
        c->stats_grid_key = spec_full;
    }
    const long ntask = ((long)V * NCH + NG - 1) / NG;            // wavefront passes (NG lane groups = NG tasks each)
    // a persistent grid of six workgroups (24 wavefronts) per CU, passes dealt round-robin: the kernel is issue-bound, and a SIMD
    // with six wavefronts of one or two passes each keeps its VALU busier than five with exactly two (48 vs 52 us at config 3,
    // 143 vs 152 at V = 20k); a seventh workgroup per CU or a second partial round costs more than it brings (7168 wavefronts
    // 53 us, 8192 57 us)
    const long max_waves = (long)c->stats_grid * 4 / (g_batch.K ? g_batch.K : 1);   // the chains of a batch share the persistent grid
    const long waves = std::min<long>(ntask, max_waves);
    const int grid = (int)std::max<long>(1, (waves + 3) / 4);
    // a sub-list holds what its workgroups can defer at most: passes per wavefront x 4 wavefronts x 64 lanes x 4 bases each
    const long per_wg = ((ntask + waves - 1) / waves) * 4 * 64 * 4;
    const size_t seg = (size_t)std::min<long>((long)V * S * 4, ((grid + DSM_BIG_NL - 1) / DSM_BIG_NL) * per_wg);
    r = ensure_big_list(c, seg);
    if (r != DSM_OK) return r;
    StatsAggParams p;
    p.cnt_vs = c->cnt_vs; p.tau = c->tau; p.gamma = c->gamma; p.eta = c->eta;
    p.V = V; p.S = S; p.G = G; p.big_seg = seg;
    p.v_off = c->shard_on ? c->shard_voff : 0; p.V_tot = c->shard_on ? c->shard_vtot : V;
    p.k0 = (uint32_t)c->ctr_seed; p.k1 = (uint32_t)(c->ctr_seed >> 32); p.iter = iter;
    p.ntab = c->ntab; p.rep = c->ntab_rep; p.ld = c->ntab_ld; p.esum = c->esum; p.log_tab = c->log_tab;
    p.xcd = 0;                                                   // (a copy of the table per XCD: measured slower, removed)
    p.hmul = DSM_NTAB_HMUL; p.swz = DSM_NTAB_SWZ;
    p.big_list = c->big_list; p.big_count = c->big_count;
    p.pat_rep = nullptr; p.pat_x = nullptr; p.pat_list = nullptr; p.pat_n = nullptr;
    if (pat) {
        r = ensure_pat(c);
        if (r != DSM_OK) return r;
        p.pat_rep = c->pat_rep; p.pat_x = c->pat_x;
        KTimer tm(c, DSM_K_STATSPAT);
        const uint32_t hi = 0xFFFFFFFFu - (++c->pat_gen);             // later passes write smaller entries: nothing to clear
        const int words = 1 << (2 * G);
        uint32_t *n_this = c->pat_list + words + (c->pat_gen & 1u), *n_next = c->pat_list + words + ((c->pat_gen + 1u) & 1u);
        p.pat_list = c->pat_list; p.pat_n = n_this;
        if (G <= 6) hipLaunchKernelGGL(pat_rep_lds_kernel, dim3(std::max(1, std::min(64, V / 4096))), dim3(1024), 0, c->stream, c->tau, V, G, c->pat_rep, hi);
        else hipLaunchKernelGGL(pat_rep_kernel, dim3((V + 255) / 256), dim3(256), 0, c->stream, c->tau, V, G, c->pat_rep, hi);
        hipLaunchKernelGGL(pat_list_kernel, dim3((words + 255) / 256), dim3(256), 0, c->stream, c->pat_rep, words, hi, c->pat_list, n_this, n_next);
        const size_t ncell = (size_t)V * S;
        // few words: pooled in LDS first (one 1024-thread workgroup per CU and share of the positions); else straight to the blocks
        const int lpw = G <= 3 ? 64 : 32;
        const size_t lds = ((size_t)1 << (2 * G)) * 4 * lpw * sizeof(uint32_t);
        if (G <= 4 && lds <= 128 * 1024 && V >= 4096) {
            const int nchunk = (S + lpw - 1) / lpw;
            const int nvsplit = std::max(1, std::min(256 / nchunk, V / (16 * (64 / lpw) * 8)));     // >= 8 passes per wavefront
            const void *fl = lpw == 64 ? (const void *)pat_agg_lds_kernel<64> : (const void *)pat_agg_lds_kernel<32>;
            static bool attr_done[2] = {false, false};
            if (!attr_done[lpw == 32]) { HIP_TRY(hipFuncSetAttribute(fl, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024)); attr_done[lpw == 32] = true; }
            const int32_t *cv = c->cnt_vs; const uint64_t *tp = c->tau; const unsigned long long *rp = c->pat_rep; uint32_t *xp = c->pat_x;
            int Vv = V, Ss = S, Gg = G, nvs = nvsplit;
            void *args[] = {(void *)&cv, (void *)&tp, (void *)&Vv, (void *)&Ss, (void *)&Gg, (void *)&rp, (void *)&xp, (void *)&nvs};
            HIP_TRY(hipLaunchKernel(fl, dim3(nchunk * nvsplit), dim3(1024), args, lds, c->stream));
        } else
            hipLaunchKernelGGL(pat_agg_kernel, dim3((unsigned)std::min<size_t>((ncell + 255) / 256, 16384)), dim3(256), 0, c->stream,
                               c->cnt_vs, c->tau, V, S, G, c->pat_rep, c->pat_x);
        HIP_TRY(hipGetLastError());
    }
    {
        // who draws an item, not what is drawn: an item whose rarer outcome has a mean above lean_cap goes to the compacted
        // kernel although inversion still applies to it -- its search would hold its 63 neighbours of the wavefront for
        // ~lean_cap more steps.  Config 3 at 10 x depth (us, this pass + compacted kernel): 128 -> 150 + 35, 64 -> 119 + 53,
        // 48 -> 105 + 81, 32 -> 86 + 134.  Data of ordinary depth has no such item once the chain has converged.
        static const char *e = DSM_AB_ENV("DESMAN_HIP_LEAN_CAP");
        p.lean_cap = e ? atof(e) : DSM_LEAN_CAP;
        static const int dbg = DSM_AB_ENV("DESMAN_HIP_STATS_DBG") ? atoi(DSM_AB_ENV("DESMAN_HIP_STATS_DBG")) : 0;
        p.dbg = dbg;
        if (!(p.lean_cap > 0.0 && p.lean_cap <= DSM_BINV_MEAN_CAP)) p.lean_cap = DSM_LEAN_CAP;
    }
    // (a batch: fewer workgroups per list, the launch holds K times as many lists; fewer for a single chain measured no faster at config 3
    // and slower at ten times the depth, profiles/r06_big_wgs.txt)
    const int big_wgs = 16;
    const int big_grid = DSM_BIG_NT * DSM_BIG_NL *
        (int)std::max<long>(1, std::min<long>((ntask * 64 * 4 / DSM_BIG_NL + 255) / 256, g_batch.K ? std::max(2, big_wgs / g_batch.K) : big_wgs));
    if (g_batch.K) {
        // two launches of the chain's pass, each collected on its own: stage 1, then the deferred items
        static thread_local BatchArgs<StatsAggParams> acc;
        acc.p[g_batch.k] = p;
        if (g_batch.k == g_batch.K - 1) {
            const dim3 g(grid, g_batch.K);
            void *args[] = {(void *)&acc};
            HIP_TRY(hipLaunchKernel(fn_b, g, dim3(256), args, sh, c->stream));
            if (!launch_big) { }                        // (the caller's choice for the whole batch; see below)
            else if (spec >= 3) hipLaunchKernelGGL(stats_big_kernel_b<3>, dim3(big_grid, g_batch.K), dim3(256), 0, c->stream, acc);
            else hipLaunchKernelGGL(stats_big_kernel_b<2>, dim3(big_grid, g_batch.K), dim3(256), 0, c->stream, acc);
        }
        HIP_TRY(hipGetLastError());
        return DSM_OK;
    }
    {
        KTimer tm(c, DSM_K_STATS);
        void *args[] = {(void *)&p};
        HIP_TRY(hipLaunchKernel(fn, dim3(grid), dim3(256), args, sh, c->stream));
    }
    // Left out (launch_big = false, only where stats_big_optional): the lists stay as stage 1 left them, and the launch that runs stage 2
    // draws whatever they hold.  An empty launch is a dependent launch boundary of 5.5-6.7 us whatever its grid (profiles/r06_big_wgs.txt).
    if (!launch_big) return DSM_OK;
    KTimer tm(c, DSM_K_STATSBIG);
    // the deferred items (none once the chain has converged on data of ordinary depth: the launch then returns at once);
    // up to 16 workgroups per list = 4096 items of a list per round (a list one item longer than a round doubles the launch:
    // every wavefront is one long dependent chain); the workgroups of an empty list leave at once
    if (spec >= 3) hipLaunchKernelGGL(stats_big_kernel<3>, dim3(big_grid), dim3(256), 0, c->stream, p);
    else hipLaunchKernelGGL(stats_big_kernel<2>, dim3(big_grid), dim3(256), 0, c->stream, p);
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}

// the halving tree of stage 2 depends on G only: laid out on the host, read through scalar registers on the device
S2Plan make_stage2_plan(int G)
{
    S2Plan pl;
    memset(&pl, 0, sizeof pl);
    int n = 0, off = 0;
    pl.lo[0] = 0; pl.hi[0] = G; pl.off[0] = 0; pl.idx[0] = 0; pl.child[0] = -1;
    n = 1;
    int lvl_begin = 0, lvl_end = 1, level = 0;
    pl.level_start[0] = 0;
    while (lvl_begin < lvl_end) {
        for (int i = lvl_begin; i < lvl_end; ++i) {
            const int w = pl.hi[i] - pl.lo[i];
            if (w == 1) { pl.child[i] = -1; continue; }
            const int wl = w / 2, mid = pl.lo[i] + wl;
            pl.child[i] = n;
            pl.lo[n] = pl.lo[i]; pl.hi[n] = mid; pl.off[n] = off; pl.idx[n] = 2 * pl.idx[i]; off += 1 << wl; ++n;
            pl.lo[n] = mid; pl.hi[n] = pl.hi[i]; pl.off[n] = off; pl.idx[n] = 2 * pl.idx[i] + 1; off += 1 << (w - wl); ++n;
        }
        lvl_begin = lvl_end; lvl_end = n;
        pl.level_start[++level] = lvl_begin;
    }
    pl.nlevels = level;                 // levels 0 .. nlevels-1 hold nodes; level_start[nlevels] = n
    pl.tab_entries = off;
    return pl;
}

int k_stats_stage2(dsm_ctx *c, uint32_t iter)
{
    KTimer tm(c, DSM_K_STATS2);
    Stage2Params p;
    p.ntab = c->ntab; p.rep = c->ntab_rep; p.ld = c->ntab_ld; p.gamma = c->gamma; p.sum_mu = c->sum_mu; p.log_tab = c->log_tab;
    p.S = c->S; p.G = c->G; p.hmul = DSM_NTAB_HMUL; p.swz = DSM_NTAB_SWZ;
    p.k0 = (uint32_t)c->ctr_seed; p.k1 = (uint32_t)(c->ctr_seed >> 32); p.iter = iter;
    p.big_count = c->big_count;
    stats_s2_lists(c, &p);
    const S2Lists ls = {c->esum, c->S};                      // (G < 10: one workgroup per sample, each reads the deferred lists' counters)
    // 2^G subsets per sample at the root: 256 threads up to G = 9, 1024 above
    const int nthr = c->G >= 10 ? 1024 : 256;
    const bool v3 = stats_draw_version(stats_spec(c)) >= 3;          // (spec 4 draws with version 2's samplers)
    // many subsets per sample (G >= 11): the root level -- one large-count binomial per subset that straddles the halves, 2^G / 1024 of
    // them per thread one after the other -- is dealt over `nsplit` workgroups per sample; the last one to finish takes the level-1
    // tables the others left in `s2_scratch` and runs the lower levels (dsm_stage2.h).  Same draws: a binomial's stream is keyed by
    // (subset, sample, node, level), the tables are integer sums.
    p.nsplit = 1; p.scratch = nullptr; p.ticket = nullptr;
    if (g_batch.K == 0 && c->G >= 11) {
        if (!c->s2_scratch) {
            hipError_t e = hipMalloc((void **)&c->s2_scratch, ((size_t)DSM_MAX_S * (S2_TAB_ENTRIES + 1)) * sizeof(uint32_t));
            if (e != hipSuccess) { dsm_set_error("hipMalloc failed: %s", hipGetErrorString(e)); return DSM_ERR_NOMEM; }
            HIP_TRY(hipMemsetAsync(c->s2_scratch, 0, ((size_t)DSM_MAX_S * (S2_TAB_ENTRIES + 1)) * sizeof(uint32_t), c->stream));
        }
        p.nsplit = c->G >= 12 ? 4 : 2;
        p.scratch = c->s2_scratch; p.ticket = c->s2_scratch + (size_t)DSM_MAX_S * S2_TAB_ENTRIES;
    }
    if (g_batch.K == 0) {
        if (v3) hipLaunchKernelGGL(stats_stage2_kernel<3>, dim3(c->S * p.nsplit), dim3(nthr), 0, c->stream, p, make_stage2_plan(c->G), ls);
        else hipLaunchKernelGGL(stats_stage2_kernel<2>, dim3(c->S * p.nsplit), dim3(nthr), 0, c->stream, p, make_stage2_plan(c->G), ls);
    } else {
        static thread_local Stage2Batch acc;
        acc.p[g_batch.k] = p; acc.ls[g_batch.k] = ls;
        if (g_batch.k == g_batch.K - 1) {
            acc.plan = make_stage2_plan(c->G);
            if (v3) hipLaunchKernelGGL(stats_stage2_kernel_b<3>, dim3(c->S, g_batch.K), dim3(nthr), 0, c->stream, acc);
            else hipLaunchKernelGGL(stats_stage2_kernel_b<2>, dim3(c->S, g_batch.K), dim3(nthr), 0, c->stream, acc);
        }
    }
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}

// A2 for the resident state: the aggregated pass (spec DSM_STATS_AGG = 2, or 3 when forced) where it applies, else the per-read pass (spec 1)
int k_stats(dsm_ctx *c, uint32_t iter, bool launch_big)
{
    if (stats_spec(c) >= 2) {
        int r = k_stats_stage1(c, iter, launch_big);
        if (r != DSM_OK) return r;
        return k_stats_stage2(c, iter);
    }
    return k_stats_v1(c, iter);
}

int k_binom_test(dsm_ctx *c, int kind, uint32_t n, const double *w, uint64_t seed, int nsamp, uint32_t *d_out, int spec)
{
    if (spec >= 3) hipLaunchKernelGGL(binom_test_kernel<3>, dim3((nsamp + 255) / 256), dim3(256), 0, c->stream, kind, n, w[0], w[1], w[2], w[3],
                                      (uint32_t)seed, (uint32_t)(seed >> 32), nsamp, c->log_tab, d_out);
    else hipLaunchKernelGGL(binom_test_kernel<2>, dim3((nsamp + 255) / 256), dim3(256), 0, c->stream, kind, n, w[0], w[1], w[2], w[3],
                       (uint32_t)seed, (uint32_t)(seed >> 32), nsamp, c->log_tab, d_out);
    HIP_TRY(hipGetLastError());
    return DSM_OK;
}
