// api_trace.hip -- the entry points that reduce the chain's resident traces, and the test hooks that plant a trace (host code only; the
// kernels are in kernels_relabel / _diag / _fit / _rbtau / _rbpair / _ppc.hip).  dsm_ctx_trace_predictive lies next to its kernels in
// kernels_pred.hip.  The scaffolding all of them share is dsm_trace_host.h.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "dsm_trace_host.h"

// digits [rows][G] -> packed words; DSM_ERR_ARG on a digit outside 0..3
static int pack_digits(const char *who, const int64_t *digits, size_t rows, int G, std::vector<uint64_t> &out)
{
    out.assign(rows, 0ull);
    for (size_t r = 0; r < rows; ++r) {
        uint64_t t = 0;
        for (int g = 0; g < G; ++g) {
            const int64_t d = digits[r * G + g];
            if (d < 0 || d > 3) { dsm_set_error("%s: digit %lld at row %zu, haplotype %d is not a base 0..3", who, (long long)d, r, g); return DSM_ERR_ARG; }
            t |= (uint64_t)d << (2 * g);
        }
        out[r] = t;
    }
    return DSM_OK;
}

// ---------------------------------------------------------------- relabelling (kernels_relabel.hip)
extern "C" int dsm_ctx_trace_snd(dsm_ctx *c, int mode, const int64_t *ref_tau, int Gr, int it0, int n_it, int32_t *snd)
{
    DSM_TRY(trace_range(c, "trace_snd", it0, n_it));
    if (mode != DSM_SND_STAR && mode != DSM_SND_SELF && mode != DSM_SND_GIVEN) { dsm_set_error("trace_snd: mode %d is none of DSM_SND_STAR / SELF / GIVEN", mode); return DSM_ERR_ARG; }
    if (mode == DSM_SND_GIVEN) {
        if (Gr < 1 || Gr > DSM_MAX_G) { dsm_set_error("trace_snd: Gr=%d outside 1..%d", Gr, DSM_MAX_G); return DSM_ERR_ARG; }
        if (!ref_tau) { dsm_set_error("trace_snd: DSM_SND_GIVEN without a reference"); return DSM_ERR_ARG; }
    } else {
        if (Gr != 0 && Gr != c->G) { dsm_set_error("trace_snd: Gr=%d, but this mode's reference has the chain's %d haplotypes (pass 0 or G)", Gr, c->G); return DSM_ERR_ARG; }
        Gr = c->G;
    }
    if (n_it > 0 && !snd) { dsm_set_error("trace_snd: no output buffer"); return DSM_ERR_ARG; }
    std::vector<uint64_t> packed;
    if (mode == DSM_SND_GIVEN) DSM_TRY(pack_digits("trace_snd", ref_tau, (size_t)c->V, Gr, packed));
    if (n_it == 0) return DSM_OK;
    BIND(c);
    const size_t V = (size_t)c->V;
    const uint64_t *ref = nullptr;
    DevBuf<uint64_t> d_ref;
    if (mode == DSM_SND_STAR) {
        double st[2];
        HIP_TRY(hipMemcpyAsync(st, c->star, sizeof st, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!(st[1] >= 0.0 && st[1] <= (double)c->n_trace)) { dsm_set_error("trace_snd: the MAP record's slot lies outside the trace of %d", c->n_trace); return DSM_ERR_STATE; }
        ref = trace_tau_slot(c, (int)st[1]);
    } else if (mode == DSM_SND_GIVEN) {
        DSM_TRY(d_ref.alloc(V));
        HIP_TRY(hipMemcpyAsync(d_ref, packed.data(), V * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        ref = d_ref;
    }
    const size_t nout = (size_t)n_it * c->G * Gr;
    DevBuf<int> d_out;
    DSM_TRY(d_out.alloc(nout));
    DSM_TRY(k_trace_snd(c, trace_view(c, it0), ref, Gr, n_it, d_out));
    HIP_TRY(hipMemcpyAsync(snd, d_out, nout * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_get_tau_sum_perm(dsm_ctx *c, const uint8_t *perm, int it0, int n_it, int64_t *tau_sum)
{
    DSM_TRY(trace_range(c, "get_tau_sum_perm", it0, n_it));
    if (!tau_sum || (n_it > 0 && !perm)) { dsm_set_error("get_tau_sum_perm: null pointer"); return DSM_ERR_ARG; }
    std::vector<uint8_t> inv;
    DSM_TRY(trace_perm_rows("get_tau_sum_perm", perm, n_it, c->G, 0, true, inv));
    BIND(c);
    const size_t nt = (size_t)c->V * c->G * 4;
    DevBuf<int64_t> d_out;
    DevBuf<uint8_t> d_inv;
    DSM_TRY(d_out.alloc(nt));
    DSM_TRY(d_inv.alloc(inv.size()));
    if (n_it > 0) HIP_TRY(hipMemcpyAsync(d_inv, inv.data(), inv.size(), hipMemcpyHostToDevice, c->stream));
    DSM_TRY(k_tau_sum_perm(c, trace_view(c, it0), d_inv, n_it, d_out));
    HIP_TRY(hipMemcpyAsync(tau_sum, d_out, nt * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// batch sums of the trace for convergence diagnostics (kernels_diag.hip): the last B L of the n_it iterations
extern "C" int dsm_ctx_trace_batch_stats(dsm_ctx *c, const uint8_t *perm, int it0, int n_it, int batch_len, int64_t *sum, int64_t *first,
                                         int64_t *bsq, int32_t *flips)
{
    DSM_TRY(trace_range(c, "trace_batch_stats", it0, n_it));
    TraceBatches b;
    DSM_TRY(trace_batches("trace_batch_stats", n_it, batch_len, &b));
    std::vector<uint8_t> inv;
    DSM_TRY(trace_perm_rows("trace_batch_stats", perm, n_it, c->G, b.skip, true, inv));
    BIND(c);
    const size_t vg = (size_t)c->V * c->G, nt = vg * 4;
    DevBuf<int64_t> d_sum, d_first, d_bsq;
    DevBuf<int32_t> d_flips;
    DevBuf<uint8_t> d_inv;
    DSM_TRY(d_sum.alloc(nt));
    DSM_TRY(d_first.alloc(nt));
    DSM_TRY(d_bsq.alloc(nt));
    DSM_TRY(d_flips.alloc(vg));
    DSM_TRY(d_inv.alloc(inv.size()));
    if (!inv.empty()) HIP_TRY(hipMemcpyAsync(d_inv, inv.data(), inv.size(), hipMemcpyHostToDevice, c->stream));
    DSM_TRY(k_trace_batch_stats(c, trace_view(c, it0 + b.skip), d_inv, b.B, b.L, d_sum, d_first, d_bsq, d_flips));
    if (sum) HIP_TRY(hipMemcpyAsync(sum, d_sum, nt * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (first) HIP_TRY(hipMemcpyAsync(first, d_first, nt * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (bsq) HIP_TRY(hipMemcpyAsync(bsq, d_bsq, nt * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (flips) HIP_TRY(hipMemcpyAsync(flips, d_flips, vg * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// posterior predictive fit per sample, position and cell over stored iterations (kernels_fit.hip): everything is read
// where it lies -- the counts, the tau, gamma and eta traces -- and nothing of the chain is written
extern "C" int dsm_ctx_trace_fit_stats(dsm_ctx *c, int it0, int n_it, double *sample, double *position, double *cell)
{
    DSM_TRY(trace_range(c, "trace_fit_stats", it0, n_it));
    const size_t V = (size_t)c->V, S = (size_t)c->S;
    if (n_it == 0) {
        if (sample) std::fill(sample, sample + S * 4, 0.0);
        if (position) std::fill(position, position + V * 4, 0.0);
        if (cell) std::fill(cell, cell + V * S, 0.0);
        return DSM_OK;
    }
    FitPlan pl;
    DSM_TRY(fit_plan(c, n_it, &pl));
    BIND(c);
    DevBuf<double> d_sample, d_position, d_cell, samp_part, pos_part, cell_part;
    DSM_TRY(d_sample.alloc(S * 4));
    DSM_TRY(d_position.alloc(V * 4));
    DSM_TRY(samp_part.alloc((size_t)pl.parts * pl.tiles * S * 4));
    DSM_TRY(pos_part.alloc((size_t)pl.parts * V * 4));
    if (cell) {
        DSM_TRY(d_cell.alloc(V * S));
        DSM_TRY(cell_part.alloc((size_t)pl.parts * V * S));
    }
    DSM_TRY(k_trace_fit_stats(c, pl, trace_view(c, it0), n_it, samp_part, pos_part, cell_part, d_sample, d_position, d_cell));
    if (sample) HIP_TRY(hipMemcpyAsync(sample, d_sample, S * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (position) HIP_TRY(hipMemcpyAsync(position, d_position, V * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (cell) HIP_TRY(hipMemcpyAsync(cell, d_cell, V * S * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// test hook: which instantiation of the fit kernel, and which grid, a call over n_it iterations would launch (nothing is launched)
extern "C" int dsm_fit_debug_path(dsm_ctx *c, int n_it, int out[5])
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (!out || n_it < 1) { dsm_set_error("fit_debug_path: bad arguments"); return DSM_ERR_ARG; }
    FitPlan pl;
    DSM_TRY(fit_plan(c, n_it, &pl));
    out[0] = pl.nsl; out[1] = pl.lpv; out[2] = pl.gc; out[3] = pl.tiles; out[4] = pl.parts;
    return DSM_OK;
}

// Rao-Blackwellised tau marginals over stored iterations (kernels_rbtau.hip): the range, perm and batch rules of
// dsm_ctx_trace_batch_stats; the counts and the three traces are read where they lie and nothing of the chain is written
extern "C" int dsm_ctx_trace_rb_marginals(dsm_ctx *c, const uint8_t *perm, int it0, int n_it, int batch_len, double *sum, double *bsq,
                                          long long *dead)
{
    DSM_TRY(trace_range(c, "trace_rb_marginals", it0, n_it));
    TraceBatches b;
    DSM_TRY(trace_batches("trace_rb_marginals", n_it, batch_len, &b));
    std::vector<uint8_t> lab;                                                 // the used rows of perm as they are
    DSM_TRY(trace_perm_rows("trace_rb_marginals", perm, n_it, c->G, b.skip, false, lab));
    const size_t nt = (size_t)c->V * c->G * 4;
    if (n_it == 0) {
        if (sum) std::fill(sum, sum + nt, 0.0);
        if (bsq) std::fill(bsq, bsq + nt, 0.0);
        if (dead) *dead = 0;
        return DSM_OK;
    }
    { int lpv, nsl; DSM_TRY(tau_shape(c->S, &lpv, &nsl)); }                     // S <= DSM_MAX_S, before anything is allocated
    BIND(c);
    DevBuf<double> d_bs, d_sum, d_bsq;
    DevBuf<unsigned long long> d_dead;
    DevBuf<uint8_t> d_perm;
    DSM_TRY(d_bs.alloc(nt));
    DSM_TRY(d_sum.alloc(nt));
    DSM_TRY(d_bsq.alloc(nt));
    DSM_TRY(d_dead.alloc(1));
    DSM_TRY(d_perm.alloc(lab.size()));
    HIP_TRY(hipMemsetAsync(d_sum, 0, nt * sizeof(double), c->stream));
    HIP_TRY(hipMemsetAsync(d_bsq, 0, nt * sizeof(double), c->stream));
    HIP_TRY(hipMemsetAsync(d_dead, 0, sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemcpyAsync(d_perm, lab.data(), lab.size(), hipMemcpyHostToDevice, c->stream));
    DSM_TRY(k_rb_tau(c, trace_view(c, it0 + b.skip), d_perm, b.B * b.L, b.L, d_bs, d_sum, d_bsq, d_dead));
    if (sum) HIP_TRY(hipMemcpyAsync(sum, d_sum, nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (bsq) HIP_TRY(hipMemcpyAsync(bsq, d_bsq, nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (dead) HIP_TRY(hipMemcpyAsync(dead, d_dead, sizeof *dead, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// Rao-Blackwellised joint posterior of two haplotypes' bases over stored iterations (kernels_rbpair.hip): the range and
// perm rules of dsm_ctx_trace_batch_stats, the stride of dsm_ctx_trace_predictive, the batch rule on the iterations the stride takes; the
// positions go through the device in chunks (rb_pairs_chunk), in ascending order; nothing of the chain is written
extern "C" int dsm_ctx_trace_rb_pairs(dsm_ctx *c, const uint8_t *perm, int it0, int n_it, int stride, int batch_len, double *joint,
                                      double *same_batch, long long *dead)
{
    DSM_TRY(trace_range(c, "trace_rb_pairs", it0, n_it));
    if (stride < 1) { dsm_set_error("trace_rb_pairs: stride %d", stride); return DSM_ERR_ARG; }
    const int nu = (int)(((long long)n_it + stride - 1) / stride);
    TraceBatches b;
    DSM_TRY(trace_batches("trace_rb_pairs", nu, batch_len, &b));
    const int G = c->G, V = c->V;
    std::vector<uint8_t> lab;                                                 // all n_it rows of perm as they are
    DSM_TRY(trace_perm_rows("trace_rb_pairs", perm, n_it, G, 0, false, lab));
    if (G > DSM_MAX_G) { dsm_set_error("trace_rb_pairs: G=%d exceeds DSM_MAX_G=%d", G, DSM_MAX_G); return DSM_ERR_UNSUPPORTED; }
    const size_t P = (size_t)G * (G - 1) / 2;
    if (P == 0) return DSM_OK;                                                // one haplotype has no pair: nothing to write
    if (nu == 0) {
        if (joint) std::fill(joint, joint + (size_t)V * P * 16, 0.0);        // (same_batch has no batch)
        if (dead) *dead = 0;
        return DSM_OK;
    }
    { int lpv, nsl; DSM_TRY(tau_shape(c->S, &lpv, &nsl)); }                     // S <= DSM_MAX_S, before anything is allocated
    // per used iteration and pair (g, h) in lexicographic order: the index of the pair of their labels, and whether they descend
    const int n_used = b.B * b.L;
    std::vector<uint16_t> slot((size_t)n_used * P);
    for (int u = 0; u < n_used; ++u) {
        const uint8_t *row = lab.data() + (size_t)(b.skip + u) * stride * G;
        size_t pi = 0;
        for (int g = 0; g < G; ++g)
            for (int h = g + 1; h < G; ++h, ++pi) {
                const int lo = std::min(row[g], row[h]), hi = std::max(row[g], row[h]);
                slot[(size_t)u * P + pi] = (uint16_t)(((lo * (2 * G - lo - 1) / 2 + (hi - lo - 1)) << 1) | (row[g] > row[h] ? 1 : 0));
            }
    }
    BIND(c);
    const int chunk = rb_pairs_chunk(V, G, b.B, joint != nullptr, same_batch != nullptr);
    const size_t bp = (size_t)b.B * P;
    DevBuf<double> d_joint, d_same, d_sb;
    DevBuf<unsigned long long> d_dead;
    DevBuf<uint16_t> d_slot;
    if (joint) DSM_TRY(d_joint.alloc((size_t)chunk * P * 16));
    if (same_batch) {
        DSM_TRY(d_same.alloc(bp * chunk));
        DSM_TRY(d_sb.alloc(bp));
        HIP_TRY(hipMemsetAsync(d_sb, 0, bp * sizeof(double), c->stream));
    }
    DSM_TRY(d_dead.alloc(1));
    DSM_TRY(d_slot.alloc(slot.size()));
    HIP_TRY(hipMemsetAsync(d_dead, 0, sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemcpyAsync(d_slot, slot.data(), slot.size() * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    const TraceView tr = trace_view(c, it0 + b.skip * stride);
    for (int v0 = 0; v0 < V; v0 += chunk) {
        const int nv = std::min(chunk, V - v0);
        DSM_TRY(k_rb_pairs(c, tr, stride, d_slot, n_used, b.L, v0, nv, d_joint, d_same, d_sb, d_dead));
        if (joint) HIP_TRY(hipMemcpyAsync(joint + (size_t)v0 * P * 16, d_joint, (size_t)nv * P * 16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    if (same_batch) HIP_TRY(hipMemcpyAsync(same_batch, d_sb, bp * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (dead) HIP_TRY(hipMemcpyAsync(dead, d_dead, sizeof *dead, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// posterior predictive p-values per sample and position from replicate tables drawn at the stored iterations (kernels_ppc.hip; DESIGN.md
// sec. 8k): the counts and the three traces are read where they lie, the uniforms are the call's own, nothing of the chain is written
extern "C" int dsm_ctx_trace_ppc(dsm_ctx *c, int it0, int n_it, int stride, int R, uint64_t salt, int64_t *ge_sample, int64_t *ge_position,
                                 double *rep_sample, double *rep_position, double *obs_sample, double *obs_position)
{
    DSM_TRY(trace_range(c, "trace_ppc", it0, n_it));
    if (stride < 1 || R < 1) { dsm_set_error("trace_ppc: stride=%d, R=%d: at least 1 is needed", stride, R); return DSM_ERR_ARG; }
    if (R > DSM_PPC_MAX_R) { dsm_set_error("trace_ppc: R=%d above DSM_PPC_MAX_R=%d", R, DSM_PPC_MAX_R); return DSM_ERR_UNSUPPORTED; }
    if ((long long)it0 + n_it > (1LL << 32) / DSM_PPC_MAX_R) {
        dsm_set_error("trace_ppc: iteration %lld does not fit the counter word", (long long)it0 + n_it);
        return DSM_ERR_UNSUPPORTED;
    }
    const size_t V = (size_t)c->V, S = (size_t)c->S;
    const int n_used = (int)(((long long)n_it + stride - 1) / stride);
    // the six outputs, 8-byte words all (all bits zero = 0 and 0.0): ge_sample [S], ge_position [V] counters; rep_sample [S][2],
    // rep_position [V][2] doubles (sum, sum of squares); obs_sample [S], obs_position [V] doubles
    void *const host[6] = {ge_sample, ge_position, rep_sample, rep_position, obs_sample, obs_position};
    const size_t bytes[6] = {S * 8, V * 8, S * 16, V * 16, S * 8, V * 8};
    if (n_used == 0) {
        for (int i = 0; i < 6; ++i) if (host[i]) memset(host[i], 0, bytes[i]);
        return DSM_OK;
    }
    PpcPlan pl;
    DSM_TRY(ppc_plan(c, n_used, R, &pl));
    BIND(c);
    DevBuf<unsigned long long> d[6];
    for (int i = 0; i < 6; ++i) DSM_TRY(d[i].alloc(bytes[i] / 8));
    for (int i = 0; i < 6; ++i) HIP_TRY(hipMemsetAsync(d[i], 0, bytes[i], c->stream));
    double *sums[4];
    for (int i = 0; i < 4; ++i) sums[i] = reinterpret_cast<double *>(d[2 + i].p);
    const uint64_t key = c->ctr_seed ^ salt;
    DSM_TRY(k_trace_ppc(c, pl, trace_view(c, it0), it0, stride, n_used, R, (uint32_t)key, (uint32_t)(key >> 32), d[0], d[1], sums[0], sums[1],
                        sums[2], sums[3]));
    for (int i = 0; i < 6; ++i) if (host[i]) HIP_TRY(hipMemcpyAsync(host[i], d[i], bytes[i], hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// test hook: which instantiation, chunks and grid a dsm_ctx_trace_ppc call would launch (nothing is launched)
extern "C" int dsm_ppc_debug_path(dsm_ctx *c, int n_used, int R, int out[8])
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (!out || n_used < 1 || R < 1 || R > DSM_PPC_MAX_R) { dsm_set_error("ppc_debug_path: bad arguments"); return DSM_ERR_ARG; }
    PpcPlan pl;
    DSM_TRY(ppc_plan(c, n_used, R, &pl));
    out[0] = pl.nsl; out[1] = pl.lpv; out[2] = pl.gc; out[3] = pl.tiles; out[4] = pl.parts; out[5] = pl.ct; out[6] = pl.cr;
    out[7] = DSM_PPC_READS;
    return DSM_OK;
}

// ---------------------------------------------------------------- planted traces
// test hook: the first n rows of the gamma and eta traces (the companion of dsm_ctx_debug_set_trace, called after it)
extern "C" int dsm_ctx_debug_set_param_trace(dsm_ctx *c, const double *gamma, const double *eta, int n)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    const int have = c->tau_trace ? c->n_trace : 0;
    if (n < 0 || n > have || (n > 0 && (!gamma || !eta))) {
        dsm_set_error("debug_set_param_trace: n=%d outside the trace of %d, or a null pointer", n, have);
        return DSM_ERR_ARG;
    }
    BIND(c);
    const size_t sg = (size_t)c->S * c->G;
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(c->gamma_trace, gamma, (size_t)n * sg * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->eta_trace, eta, (size_t)n * 16 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// test hook: a synthetic trace.  Slot 0 = the resident state, slots 1 .. n = the given digits.  A context on which no update has run has
// no MAP record yet: it gets the resident state as one (slot 0, lp = -inf), so that DSM_SND_STAR has a reference; an existing record stays.
extern "C" int dsm_ctx_debug_set_trace(dsm_ctx *c, const int64_t *tau_digits, int n)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (n < 0 || (n > 0 && !tau_digits)) { dsm_set_error("debug_set_trace: bad arguments"); return DSM_ERR_ARG; }
    std::vector<uint64_t> packed;
    DSM_TRY(pack_digits("debug_set_trace", tau_digits, (size_t)n * c->V, c->G, packed));
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    const bool fresh = !c->tau_trace || n > c->trace_cap;
    const bool no_star = !c->tau_trace;
    DSM_TRY(alloc_traces(c, n));
    const size_t V = (size_t)c->V, sg = (size_t)c->S * c->G;
    if (fresh) {                                      // the other traces of a new allocation read as zero
        const size_t cap = (size_t)c->trace_cap;
        HIP_TRY(hipMemsetAsync(c->ll_trace, 0, cap * sizeof(double), c->stream));
        HIP_TRY(hipMemsetAsync(c->lp_trace, 0, cap * sizeof(double), c->stream));
        HIP_TRY(hipMemsetAsync(c->nchange_trace, 0, cap * sizeof(int), c->stream));
        HIP_TRY(hipMemsetAsync(c->gamma_trace, 0, cap * sg * sizeof(double), c->stream));
        HIP_TRY(hipMemsetAsync(c->eta_trace, 0, cap * 16 * sizeof(double), c->stream));
    }
    if (no_star) {
        const double st[2] = {-INFINITY, 0.0};
        HIP_TRY(hipMemcpyAsync(c->star, st, sizeof st, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->gamma_star, c->gamma, sg * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->eta_star, c->eta, 16 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(c->tau_trace, c->tau, V * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
    if (n > 0) HIP_TRY(hipMemcpyAsync(c->tau_trace + V, packed.data(), (size_t)n * V * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}
