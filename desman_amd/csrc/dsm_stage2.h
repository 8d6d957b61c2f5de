// dsm_stage2.h -- stage 2 of the aggregated mu/E pass (spec: oracle/stats_agg.c, stage2_sample): one workgroup
// per sample spreads the subset counts N[.][s] over the haplotypes by halving the haplotype range recursively.
// Node (level, idx) owns the range [lo,hi) and a table of 2^(hi-lo) subset counts; its lower child gets
// floor(w/2) haplotypes.  A subset that lies in one half passes through; one that straddles is split by one
// binomial with odds (sum gamma lower : sum gamma upper) from the stream
// Philox({subset, s | idx << 16 | level << 24, iter, 'STA2'}).  Leaves (w = 1) are sum_mu[s][lo].
// The tree depends on G only: the host lays it out (S2Plan, kernel argument -> scalar registers), every node
// below the root has its own zero-initialised LDS table, so a level costs one workgroup barrier.
// Shared by stats_stage2_kernel (kernels_stats.hip) and dirichlet_kernel (kernels_gibbs.hip, fused form).
#pragma once
#include "dsm_binom.h"
#include "dsm_big_item.h"
#include "log_table.h"

#define S2_MAX_NODES 32
#define S2_MAX_LEVELS 6
#define S2_TAB_ENTRIES 1024
struct S2Plan {
    int nlevels, tab_entries;
    int level_start[S2_MAX_LEVELS + 2];
    signed char lo[S2_MAX_NODES], hi[S2_MAX_NODES], child[S2_MAX_NODES];
    unsigned char idx[S2_MAX_NODES];
    short off[S2_MAX_NODES];
};

struct Stage2Params {
    uint32_t *ntab;                 // [rep][2^G][S], zeroed after reading
    int rep, ld;                    // copies of the table (their sum is the count); row stride in words (>= S)
    const double *gamma;            // [S][G]
    unsigned long long *sum_mu;     // [S][G] accumulated into (stand-alone kernel)
    const double *log_tab;
    int S, G;
    uint32_t k0, k1, iter;
    uint32_t hmul, swz;             // row of (subset H, sample s) in ntab: (H * hmul + (s >> 4) * swz) mod 2^G (dsm_host.h: DSM_NTAB_HMUL / _SWZ)
    uint32_t *big_count;            // work-list counters of stage 1 (or null)
    // The deferred items of stage 1 (big_list non-null: G < 10, one workgroup per sample).  stats_big_kernel leaves every list it consumed
    // empty; where the host left that launch out, the counters are still up and the workgroups of this launch draw the items themselves
    // (s2_inline_items below).  The host's choice is a matter of speed only: either way every item is drawn exactly once.
    // (only what the rest of the block does not hold already: the chains of a batch share one argument segment)
    const unsigned long long *big_list;
    const int32_t *cnt_vs;          // [V][S][4]
    const uint64_t *tau;            // [V]
    const double *eta;              // [4][4] the matrix stage 1 ran with
    uint32_t big_seg;               // entries per list
    int V;
    int nsplit;                     // workgroups that share a sample's root level (stand-alone kernel, G >= 11), else 1
    uint32_t *scratch, *ticket;     // [S][S2_TAB_ENTRIES] level-1 tables handed over, [S] arrival counters; zero between passes
};                                  // the plan of the halving tree (a function of G) travels beside it: one per launch

S2Plan make_stage2_plan(int G);     // kernels_stats.hip
struct dsm_ctx;
void stats_s2_lists(const dsm_ctx *c, Stage2Params *p);     // kernels_stats.hip: the deferred-list fields above
// ... and what differs between the launches that run stage 2 (an argument of its own)
struct S2Lists {
    unsigned long long *esum;       // [16] the items' E sums are added here (device-scope atomics)
    int n_arrive;                   // workgroups of the launch that read the counters: whoever arrives last closes the lists
};

#define S2_NLIST (DSM_BIG_NT * DSM_BIG_NL)
// every thread of the first three wavefronts loads one list counter (early: the load flies while the tables are staged) ...
__device__ __forceinline__ uint32_t s2_list_count(const Stage2Params &p)
{
    return (p.big_list && threadIdx.x < S2_NLIST) ? p.big_count[threadIdx.x * DSM_BIG_STRIDE] : 0u;
}
// ... and posts, ahead of a barrier the caller has anyway, whether its wavefront saw a non-empty list; after that barrier s2_lists_any()
// is the same for every thread of the workgroup -- and of the launch: the counters change only once every workgroup has read them
__device__ __forceinline__ void s2_lists_post(uint32_t *wflag, uint32_t my_cnt)
{
    const bool nz = __builtin_amdgcn_ballot_w64(my_cnt != 0u) != 0ull;
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 256) wflag[threadIdx.x >> 6] = nz ? 1u : 0u;
}
__device__ __forceinline__ bool s2_lists_any(const uint32_t *wflag) { return (wflag[0] | wflag[1] | wflag[2]) != 0u; }
// one arrival per workgroup that found the lists non-empty; true in the workgroup that arrives last (all threads; ends with a barrier and
// a device-scope fence).  The caller's own device-scope adds must have been fenced before.
__device__ __forceinline__ bool s2_lists_arrive(const Stage2Params &p, int n_arrive, int *last_flag)
{
    if (threadIdx.x == 0) *last_flag = (atomicAdd(p.big_count + DSM_BIG_W_ARRIVE, 1u) == (uint32_t)(n_arrive - 1)) ? 1 : 0;
    __syncthreads();
    const bool last = *last_flag != 0;
    __threadfence();
    return last;
}
// the last arriver: every list has been consumed (each sample's workgroup drew its own items), so the counters go back to zero
__device__ __forceinline__ void s2_lists_close(const Stage2Params &p)
{
    if (threadIdx.x < S2_NLIST) p.big_count[threadIdx.x * DSM_BIG_STRIDE] = 0u;
    if (threadIdx.x == 0) { p.big_count[DSM_BIG_W_ARRIVE] = 0u; atomicAdd(p.big_count + DSM_BIG_W_SEEN, 1u); }
}
// The inline list phase of sample s's workgroup (all threads; the samplers' tables are staged).  It draws the items of ITS sample from
// every non-empty list -- a list holds items of any sample, so it filters by the item's sample; the adds go to row s of the subset table
// and to Esum -- then fences, arrives, and returns whether it arrived last.  No workgroup waits for another.
template <int SPEC>
__device__ __forceinline__ bool s2_inline_items(const Stage2Params &p, const S2Lists &ls, int s, uint32_t my_cnt, const double *rcp, const double2 *ltab)
{
    BigItemParams big;              // (never a chain sharded by positions, never the pooled counts of specification 4: those keep stats_big_kernel)
    big.cnt_vs = p.cnt_vs; big.tau = p.tau; big.gamma = p.gamma; big.pat_x = nullptr; big.ntab = p.ntab; big.rep = p.rep; big.ld = p.ld;
    big.S = p.S; big.G = p.G; big.v_off = 0; big.V_tot = p.V; big.k0 = p.k0; big.k1 = p.k1; big.iter = p.iter; big.hmul = p.hmul; big.swz = p.swz;
    __shared__ uint32_t cnt[S2_NLIST];
    __shared__ unsigned long long eacc[16];
    __shared__ double es[16];
    __shared__ int last_flag;
    const int tid = threadIdx.x, nthr = blockDim.x;
    if (tid < S2_NLIST) cnt[tid] = my_cnt;
    if (tid < 16) { eacc[tid] = 0ull; es[tid] = p.eta[tid]; }
    __syncthreads();
    for (int sub = 0; sub < S2_NLIST; ++sub) {
        const uint32_t nb = cnt[sub];
        if (!nb) continue;
        const unsigned long long *list = p.big_list + (size_t)sub * p.big_seg;
        for (uint32_t i = tid; i < nb; i += nthr) {
            const unsigned long long item = list[i];
            if (big_item_sample(big, item) != s) continue;
            uint32_t n[4];
            const int b = big_item_draw<SPEC>(big, item, (unsigned)sub, es, rcp, ltab, n);
#pragma unroll
            for (int a = 0; a < 4; ++a) if (n[a]) atomicAdd(&eacc[b * 4 + a], (unsigned long long)n[a]);
        }
    }
    __syncthreads();
    if (tid < 16 && eacc[tid]) atomicAdd(&ls.esum[tid], eacc[tid]);
    __threadfence();                    // this thread's adds to the table and to Esum are performed ...
    __syncthreads();                    // ... every thread's are
    return s2_lists_arrive(p, ls.n_arrive, &last_flag);      // (its closing fence: what stage 2 loads below is loaded afresh)
}

#define S2_SMEM_BYTES (DSM_LOG_TAB_N * 16 + DSM_EXP_TAB_N * 8 + DSM_RCP_TAB_N * 8 + 32 * 8 + S2_TAB_ENTRIES * 4 + 32 * 4 + 5 * S2_MAX_NODES * 4)

#ifdef DSM_AB_SWITCHES           // phase stamps of the Dirichlet launch's gamma rows (experiment build): [row][entry, tables staged, level 0, 1, 2, 3, stage 2 done, draw done]
__device__ unsigned long long s2_clk[1024 * 8];
#define S2_CLK(row, k) do { if (threadIdx.x == 0 && blockIdx.y == 0 && (row) < 1024) s2_clk[(size_t)(row) * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define S2_CLK(row, k) do { } while (0)
#endif
// leaf counts end in LDS (returned pointer, [G] u32, valid after the function's final barrier); to_global also adds
// them to p.sum_mu[s][.]
// last_out (or null): set where this workgroup arrived last at the end of an inline list phase
template <int SPEC>
__device__ __forceinline__ const uint32_t *stage2_sample(const Stage2Params &p, const S2Plan &pl, int s, char *smem, bool to_global, int part = 0,
                                                         const S2Lists &ls = S2Lists{nullptr, 0}, bool *last_out = nullptr)
{
    __shared__ uint32_t lists_wflag[4];
    const int G = p.G, tid = threadIdx.x, nthr = blockDim.x;      // 256 (fused form) or 1024 (many subsets)
    double2 *ltab = reinterpret_cast<double2 *>(smem);                         // [256] log table, then [64] exp table
    double *etab = reinterpret_cast<double *>(ltab + DSM_LOG_TAB_N);
    double *rcp = etab + DSM_EXP_TAB_N;                                        // [256]
    double *gs = rcp + DSM_RCP_TAB_N;                                          // [32]
    uint32_t *tab = reinterpret_cast<uint32_t *>(gs + 32);                     // [S2_TAB_ENTRIES] tables of all nodes below the root
    uint32_t *leaf = tab + S2_TAB_ENTRIES;                                     // [32]
    int *n_lo = reinterpret_cast<int *>(leaf + 32);                            // the plan's node arrays (lane-indexed below)
    int *n_hi = n_lo + S2_MAX_NODES, *n_off = n_hi + S2_MAX_NODES, *n_idx = n_off + S2_MAX_NODES, *n_child = n_idx + S2_MAX_NODES;

    const int nsplit = p.nsplit > 1 ? p.nsplit : 1;
    S2_CLK(s, 0);
    // Round 6: a thread's first root-level count is on its way while the tables are staged (the load has nothing to do with them: 0.9 us of
    // the launch's ~21 us critical path, phase stamps of the experiment build: profiles/r06_s2_clocks.txt).  One copy of the table only.
    uint32_t pre_n = 0;
    bool pre_ok = false;
    {
        const int total0 = 1 << G, share0 = nsplit > 1 ? (total0 + nsplit - 1) / nsplit : total0;
        const int j0 = (nsplit > 1 ? part * share0 : 0) + tid, jh0 = nsplit > 1 ? min(total0, part * share0 + share0) : total0;
        if (p.rep == 1 && j0 < jh0 && j0 != 0) {
            pre_n = p.ntab[(size_t)(((uint32_t)j0 * p.hmul + ((uint32_t)s >> 4) * p.swz) & ((1u << G) - 1u)) * (size_t)p.ld + s];
            pre_ok = true;
        }
    }
    const uint32_t my_cnt = s2_list_count(p);
    // (without the lists -- stage 2 of G >= 10, which always follows stats_big_kernel -- the counters are cleared here as they always were)
    if (!p.big_list && s == 0 && part == 0 && tid < DSM_BIG_NT * DSM_BIG_NL && p.big_count) p.big_count[tid * DSM_BIG_STRIDE] = 0u;
    if (tid < DSM_LOG_TAB_N) ltab[tid] = reinterpret_cast<const double2 *>(p.log_tab)[tid];
    if (tid < DSM_EXP_TAB_N) etab[tid] = p.log_tab[2 * DSM_LOG_TAB_N + tid];
    for (int k = tid; k < DSM_RCP_TAB_N; k += nthr) rcp[k] = k ? 1.0 / (double)k : 0.0;
    if (tid < 32) {
        gs[tid] = (tid < G) ? p.gamma[(size_t)s * G + tid] : 0.0; leaf[tid] = 0u;
        n_lo[tid] = pl.lo[tid]; n_hi[tid] = pl.hi[tid]; n_off[tid] = pl.off[tid]; n_idx[tid] = pl.idx[tid];
        n_child[tid] = pl.child[tid];
    }
    for (int i = tid; i < S2_TAB_ENTRIES; i += nthr) tab[i] = 0u;
    if (p.big_list) s2_lists_post(lists_wflag, my_cnt);
    __syncthreads();
    if (p.big_list && s2_lists_any(lists_wflag)) {
        const bool last = s2_inline_items<SPEC>(p, ls, s, my_cnt, rcp, ltab);
        if (last) s2_lists_close(p);
        if (last_out) *last_out = last;
        pre_ok = false;                 // the count loaded ahead is from before this sample's items were added
    }
    S2_CLK(s, 1);

    // Round 6: a node's count goes straight into leaf[] where its child is a single haplotype, so the tree's last level -- leaves only: a pass
    // over the level and a barrier to copy table entries, 1.0 us of the launch -- is not walked (integer adds: the same sums)
    const int nlev = pl.nlevels > 1 ? pl.nlevels - 1 : pl.nlevels;
    for (int level = 0; level < nlev; ++level) {
        // all (node, subset) pairs of the level at once: the tables of a level are contiguous in `tab`, so entry j of
        // the level belongs to the node whose table covers it (root: the 2^G words of this sample in HBM)
        const int n0 = pl.level_start[level], n1 = pl.level_start[level + 1];
        const int base = pl.off[n0];
        const int total = (level == 0) ? (1 << G) : (pl.off[n1 - 1] + (1 << (pl.hi[n1 - 1] - pl.lo[n1 - 1]))) - base;
        // (the root level of a sample that several workgroups share: this one's contiguous share of the subsets)
        const int share = (level == 0 && nsplit > 1) ? (total + nsplit - 1) / nsplit : total;
        const int j_lo = (level == 0 && nsplit > 1) ? part * share : 0, j_hi = (level == 0 && nsplit > 1) ? min(total, j_lo + share) : total;
        for (int j = j_lo + tid; j < j_hi; j += nthr) {
            int i = n0;
            for (int k = n0 + 1; k < n1; ++k) if (j + base >= pl.off[k]) i = k;      // scalar plan, <= 16 nodes per level
            const int lo = n_lo[i], hi = n_hi[i], w = hi - lo;
            const uint32_t Hs = (uint32_t)(j + base - n_off[i]);
            if (Hs == 0) continue;
            uint32_t n;
            if (level == 0) {
                uint32_t *cell = p.ntab + (size_t)((Hs * p.hmul + ((uint32_t)s >> 4) * p.swz) & ((1u << G) - 1u)) * (size_t)p.ld + s;
                const size_t cstride = ((size_t)1 << G) * (size_t)p.ld;
                if (p.rep == 8) {
                    // one copy per XCD (kernels_stats.hip): all eight loads in flight at once -- read one after the other (a store may
                    // alias the next load, so the compiler keeps the order) they cost eight memory round trips: +3.5 us on the launch
                    uint32_t m[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) m[r] = __builtin_nontemporal_load(cell + r * cstride);
                    n = 0;
#pragma unroll
                    for (int r = 0; r < 8; ++r) { n += m[r]; if (m[r]) cell[r * cstride] = 0u; }
                } else {
                    n = (pre_ok && j == j_lo + tid) ? pre_n : *cell;
                    if (n) *cell = 0u;
                    for (int r = 1; r < p.rep; ++r) {           // few subsets, many positions: the atomics of stage 1 were spread over copies
                        const uint32_t m = cell[r * cstride];
                        if (m) { cell[r * cstride] = 0u; n += m; }
                    }
                }
            } else n = tab[base + j];
            if (w == 1) {                                   // leaf: Hs == 1.  Only the root can be one here (G = 1): every other leaf was added to by its parent
                if (level == 0) leaf[lo] = n;
                continue;
            }
            if (!n) continue;
            const int wl = w / 2, wh = w - wl, mid = lo + wl;
            const int ch = n_child[i];
            uint32_t *L = tab + n_off[ch], *R = tab + n_off[ch + 1];
            const uint32_t HL = Hs & ((1u << wl) - 1u), HR = Hs >> wl;
            if (wl == 1) L = leaf + lo - 1;                  // (HL is 1 wherever it is added to: L[HL] = leaf[lo])
            if (wh == 1) R = leaf + mid - 1;
            if (!HR) { atomicAdd(&L[HL], n); continue; }
            if (!HL) { atomicAdd(&R[HR], n); continue; }
            double wL = 0.0, wR = 0.0;
            for (int jj = 0; jj < wl; ++jj) if ((HL >> jj) & 1u) wL = wL + gs[lo + jj];
            for (int jj = 0; jj < wh; ++jj) if ((HR >> jj) & 1u) wR = wR + gs[mid + jj];
            Xo128 rng = xo_seed(Hs, (uint32_t)s | ((uint32_t)n_idx[i] << 16) | ((uint32_t)level << 24), p.iter, DSM_STREAM_STA2,
                                p.k0, p.k1);
            bool dummy = false;
            const uint32_t k = binom<true, SPEC>(rng, n, wL, wR, rcp, ltab, dummy, DSM_BINV_MEAN_CAP_S2);
            if (k) atomicAdd(&L[HL], k);
            if (n - k) atomicAdd(&R[HR], n - k);
        }
        __syncthreads();
        if (level < 4) S2_CLK(s, 2 + level);
        if (level == 0 && nsplit > 1) {
            // hand the level-1 tables over: device-scope atomics onto the sample's scratch rows (they execute at the memory side, so
            // the reader below sees every one of them), then a ticket; whoever draws the last ticket owns the rest of the tree
            const int l1 = pl.level_start[1], l2 = pl.level_start[2];
            const int b1 = pl.off[l1], n1 = (pl.off[l2 - 1] + (1 << (pl.hi[l2 - 1] - pl.lo[l2 - 1]))) - b1;
            uint32_t *row = p.scratch + (size_t)s * S2_TAB_ENTRIES;
            // (the adds RETURN their old value: a thread passes the barrier below only when its adds have been performed, so the
            // ticket -- issued after the barrier -- is ordered behind every add of this workgroup without a cache-flushing fence)
            uint32_t sink = 0;
            for (int i = tid; i < n1; i += nthr) { const uint32_t v = tab[b1 + i]; if (v) sink += atomicAdd(&row[i], v); }
            asm volatile("" :: "v"(sink));
            __syncthreads();
            __shared__ int last_wg;
            if (tid == 0) last_wg = (atomicAdd(&p.ticket[s], 1u) == (uint32_t)(nsplit - 1)) ? 1 : 0;
            __syncthreads();
            if (!last_wg) return leaf;                         // (callers of the split form use nothing of the returned tables)
            for (int i = tid; i < n1; i += nthr) tab[b1 + i] = atomicExch(&row[i], 0u);      // read at the memory side, left zero for the next pass
            if (tid == 0) p.ticket[s] = 0u;
            __syncthreads();
        }
    }
    if (to_global && tid < G && leaf[tid]) p.sum_mu[(size_t)s * G + tid] += leaf[tid];
    return leaf;
}
