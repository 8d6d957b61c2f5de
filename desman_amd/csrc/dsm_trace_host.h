// dsm_trace_host.h -- the host scaffolding of a reduction of the chain's resident traces (internal): where an iteration's rows lie, the
// range, batch and label rules the entry points share.  Plain functions and two small structs, as in dsm_host_util.h; a function whose
// message names the entry point takes it as `who`.  A new trace reduction starts from these, not from a copy of another one's host half.
#pragma once
#include "dsm_host_util.h"

// The tau of trace slot `slot`.  Slot 0 is the state the update call entered with, so iteration t lies in slot t + 1; after an update
// that held tau (tau_fixed_trace) slot 0 is the tau of every iteration and no other slot is written.
static inline const uint64_t *trace_tau_slot(const dsm_ctx *c, int slot) { return c->tau_trace + (c->tau_fixed_trace ? 0 : (size_t)slot * c->V); }

// The rows of the three traces from stored iteration it0 on; tau_stride = words between two iterations' tau rows (0: one row for all).
// gamma and eta have no entry slot: iteration t lies in row t.  Nothing else computes these addresses.
struct TraceView { const uint64_t *tau; size_t tau_stride; const double *gamma, *eta; };
static inline TraceView trace_view(const dsm_ctx *c, int it0)
{
    return {trace_tau_slot(c, it0 + 1), c->tau_fixed_trace ? 0 : (size_t)c->V, c->gamma_trace + (size_t)it0 * c->S * c->G,
            c->eta_trace + (size_t)it0 * 16};
}

// what every trace reduction asks first: counts, a state, a trace, and a range inside it
static inline int trace_range(dsm_ctx *c, const char *who, int it0, int n_it)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (!c->tau_trace) { dsm_set_error("%s: no update has run", who); return DSM_ERR_STATE; }
    if (it0 < 0 || n_it < 0 || it0 > c->n_trace || n_it > c->n_trace - it0) {
        dsm_set_error("%s: iterations %d .. %d + %d outside the trace of %d", who, it0, it0, n_it, c->n_trace);
        return DSM_ERR_ARG;
    }
    return DSM_OK;
}

// the batch rule: B batches of L iterations, B even, over the LAST B L of n_it iterations -- the first `skip` are left out
struct TraceBatches { int L, B, skip; };
static inline int trace_batches(const char *who, int n_it, int L, TraceBatches *b)
{
    if (L < 1) { dsm_set_error("%s: batch_len=%d, at least 1 is needed", who, L); return DSM_ERR_ARG; }
    if (n_it > 0 && n_it / 2 < L) { dsm_set_error("%s: %d iterations are fewer than two batches of %d", who, n_it, L); return DSM_ERR_ARG; }
    const int B = n_it > 0 ? 2 * (n_it / (2 * L)) : 0;       // (n_it > 0: 2 L <= n_it)
    *b = {L, B, n_it - B * L};
    return DSM_OK;
}

// The label rows of the iterations from `skip` on -- as they are or, `inverse`, as inv[t][perm[t][g]] = g; a null perm is identity rows.
// All n_it rows are checked, those of skipped iterations too: DSM_ERR_ARG on a row that is no permutation of 0..G-1.
static inline int trace_perm_rows(const char *who, const uint8_t *perm, int n_it, int G, int skip, bool inverse, std::vector<uint8_t> &rows)
{
    rows.resize((size_t)(n_it - skip) * G);
    for (int t = 0; t < n_it; ++t) {
        uint32_t seen = 0;
        for (int g = 0; g < G; ++g) {
            const int p = perm ? perm[(size_t)t * G + g] : g;
            if (p >= G || (seen >> p & 1u)) { dsm_set_error("%s: row %d of perm is not a permutation of 0..%d", who, t, G - 1); return DSM_ERR_ARG; }
            seen |= 1u << p;
            if (t >= skip) rows[(size_t)(t - skip) * G + (inverse ? p : g)] = (uint8_t)(inverse ? g : p);
        }
    }
    return DSM_OK;
}
