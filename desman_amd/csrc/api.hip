// api.hip -- the C ABI of libdesman_hip.so (see include/desman_hip.h).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <numeric>
#include <thread>

#include "dsm_host.h"
#include "dsm_trace_host.h"
#include "log_table.h"

static thread_local char g_err[512] = "";

void dsm_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

extern "C" const char *dsm_last_error(void) { return g_err; }
extern "C" const char *dsm_version(void) { return "desman_hip 0.1 (gfx950)"; }

extern "C" int dsm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

static const char *const k_names[] = {"stats_kernel", "dirichlet_kernel", "tau_kernel", "finalize_kernel",
                                      "mt_fill_kernel", "nmft_pass_a", "nmft_gamma", "nmft_pass_b",
                                      "stats_stage2_kernel", "stats_big_kernel", "pat_rep_kernel + pat_agg_kernel"};
static_assert(sizeof(k_names) / sizeof(k_names[0]) == DSM_K_COUNT, "one name per DSM_K_* id");
extern "C" const char *dsm_kernel_name(int k) { return (k >= 0 && k < DSM_K_COUNT) ? k_names[k] : "?"; }

// ---------------------------------------------------------------- timing
KTimer::KTimer(dsm_ctx *ctx, int kid, hipStream_t stream) : c(ctx), k(kid), st(stream ? stream : ctx->stream)
{
    c->k_launches[k]++;
    if (!c->timing) return;
    auto take = [&]() {
        hipEvent_t e;
        if (!c->free_events.empty()) { e = c->free_events.back(); c->free_events.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    };
    e0 = take(); e1 = take();
    (void)hipEventRecord(e0, st);
}
KTimer::~KTimer()
{
    if (!e0) return;
    (void)hipEventRecord(e1, st);
    c->spans.push_back({k, e0, e1});
}

static int collect_spans(dsm_ctx *c)
{
    if (c->spans.empty()) return DSM_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream_rng));
    for (auto &s : c->spans) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.e0, s.e1));
        c->k_ms[s.k] += ms;
        c->free_events.push_back(s.e0);
        c->free_events.push_back(s.e1);
    }
    c->spans.clear();
    return DSM_OK;
}

extern "C" int dsm_ctx_set_timing(dsm_ctx *c, int on)
{
    if (!c) return DSM_ERR_ARG;
    int r = collect_spans(c);
    c->timing = on != 0;
    for (int k = 0; k < DSM_K_COUNT; ++k) { c->k_ms[k] = 0; c->k_launches[k] = 0; }
    return r;
}

extern "C" int dsm_ctx_get_timing(dsm_ctx *c, double *ms_total, int64_t *launches)
{
    if (!c) return DSM_ERR_ARG;
    int r = collect_spans(c);
    if (r) return r;
    for (int k = 0; k < DSM_K_COUNT; ++k) {
        if (ms_total) ms_total[k] = c->k_ms[k];
        if (launches) launches[k] = c->k_launches[k];
    }
    return DSM_OK;
}

// ---------------------------------------------------------------- helpers (dev_alloc, DevBuf, DSM_TRY, BIND, dsm_ctx_need: dsm_host_util.h)
template <typename T>
static void dev_free(T **p) { if (*p) { (void)hipFree(*p); *p = nullptr; } }

// Esum and the DSM_ESUM_PARTS copies stage 1 adds to, all zero: what a failed pass left in the copies is not added to the next one
static int esum_reset(dsm_ctx *c)
{
    HIP_TRY(hipMemsetAsync(c->esum, 0, (16 + 16 * DSM_ESUM_PARTS) * sizeof(unsigned long long), c->stream));
    return DSM_OK;
}

// Both slots of the sweep's block order start as the identity and no slot is marked usable: whatever a failed or skipped finalize launch
// leaves behind is then the identity or an order written for the CURRENT grid (the grid changes only with the table: dsm_ctx_set_counts
// calls this again) -- a sweep can never index its blocks through stale or uninitialised words.
static int reset_blk_order(dsm_ctx *c)
{
    static const std::vector<uint32_t> ident = [] { std::vector<uint32_t> v((size_t)2 * DSM_MAX_GRID); for (size_t i = 0; i < v.size(); ++i) v[i] = (uint32_t)(i % DSM_MAX_GRID); return v; }();
    c->blk_order_n[0] = c->blk_order_n[1] = 0;
    if (!c->blk_order) return DSM_OK;
    HIP_TRY(hipMemcpyAsync(c->blk_order, ident.data(), ident.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    return DSM_OK;
}

// ---------------------------------------------------------------- lifecycle
extern "C" int dsm_ctx_create(dsm_ctx **out, int device)
{
    if (!out) return DSM_ERR_ARG;
    *out = nullptr;
    DSM_TRY(dsm_bind_device(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        dsm_set_error("device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
        return DSM_ERR_NODEVICE;
    }
    dsm_ctx *c = new dsm_ctx();
    c->device = device;
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (getenv("DESMAN_HIP_ONE_STREAM")) c->stream_rng = c->stream;      // several chains per GPU: one hardware queue each
    else {   // the single-workgroup MT19937 refill must not queue behind a full grid of the main stream
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(hipStreamCreateWithPriority(&c->stream_rng, hipStreamNonBlocking, hi));
    }
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipEventCreateWithFlags(&c->ev_u_ready[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_u_free[i], hipEventDisableTiming));
    }
    DSM_TRY(dev_alloc(&c->mt_state, 625));
    DSM_TRY(dev_alloc(&c->ll_partial, 2 * DSM_MAX_GRID));     // two parities (updateTau pipelines finalize into the next sweep)
    DSM_TRY(dev_alloc(&c->nchange, 2));
    DSM_TRY(dev_alloc(&c->sweep_stats, 2));
    HIP_TRY(hipMemsetAsync(c->sweep_stats, 0, 2 * sizeof(unsigned long long), c->stream));
    DSM_TRY(dev_alloc(&c->step_cnt, (size_t)2 * 2 * DSM_MAX_GRID));
    HIP_TRY(hipMemsetAsync(c->step_cnt, 0, (size_t)2 * 2 * DSM_MAX_GRID * sizeof(uint32_t), c->stream));
    DSM_TRY(dev_alloc(&c->blk_order, (size_t)2 * DSM_MAX_GRID));
    DSM_TRY(reset_blk_order(c));
    DSM_TRY(dev_alloc(&c->screen_ctl, 4));
    HIP_TRY(hipMemsetAsync(c->screen_ctl, 0, 4 * sizeof(uint32_t), c->stream));
    DSM_TRY(dev_alloc(&c->prior, 2 * (DSM_MAX_S + 4)));
    DSM_TRY(dev_alloc(&c->scalars, 8));
    DSM_TRY(dev_alloc(&c->star, 2));
    DSM_TRY(dev_alloc(&c->eta, 16));
    DSM_TRY(dev_alloc(&c->eta_new, 16));
    DSM_TRY(dev_alloc(&c->eta_star, 16));
    DSM_TRY(dev_alloc(&c->esum, 16 + 16 * DSM_ESUM_PARTS));
    DSM_TRY(dev_alloc(&c->log_tab, 2 * DSM_LOG_TAB_N + DSM_EXP_TAB_N));           // log table, then the exp table of spec 3
    HIP_TRY(hipMemcpyAsync(c->log_tab, dsm_log_table_host, sizeof dsm_log_table_host, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->log_tab + 2 * DSM_LOG_TAB_N, dsm_exp_table_host, sizeof dsm_exp_table_host, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->nchange, 0, 2 * sizeof(int), c->stream));
    DSM_TRY(esum_reset(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = c;
    return DSM_OK;
}

static void free_traces(dsm_ctx *c)
{
    dev_free(&c->tau_trace); dev_free(&c->ll_trace); dev_free(&c->lp_trace); dev_free(&c->nchange_trace);
    dev_free(&c->gamma_trace); dev_free(&c->eta_trace); dev_free(&c->gamma_in); dev_free(&c->eta_in);
    c->in_cap = 0;
    c->n_trace = 0;
    c->trace_cap = 0;
    c->tau_fixed_trace = false;
}

extern "C" int dsm_ctx_destroy(dsm_ctx *c)
{
    if (!c) return DSM_OK;
    if (c->fixtau_child) { dsm_ctx_destroy(c->fixtau_child); c->fixtau_child = nullptr; }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    collect_spans(c);
    for (auto e : c->free_events) (void)hipEventDestroy(e);
    free_traces(c);
    dev_free(&c->cnt_vs); dev_free(&c->items); dev_free(&c->nitems); dev_free(&c->tau);
    dev_free(&c->pat_rep); dev_free(&c->pat_x); dev_free(&c->pat_list); c->pat_rep_len = c->pat_x_len = 0;
    if (c->h_rare) { (void)hipHostFree(c->h_rare); c->h_rare = nullptr; }
    dev_free(&c->s2_scratch);
    dev_free(&c->blk_tab); stats_release_ntab(c); dev_free(&c->big_list); dev_free(&c->big_count);
    dev_free(&c->gamma); dev_free(&c->eta);
    dev_free(&c->eta_new); dev_free(&c->sum_mu); dev_free(&c->esum); dev_free(&c->mt_state); dev_free(&c->mt_jstates); dev_free(&c->u_raw);
    dev_free(&c->ll_partial); dev_free(&c->nchange); dev_free(&c->sweep_stats); dev_free(&c->step_cnt); dev_free(&c->blk_order); dev_free(&c->screen_ctl); dev_free(&c->prior); dev_free(&c->prior_all); dev_free(&c->scalars); dev_free(&c->star);
    dev_free(&c->gamma_star); dev_free(&c->eta_star); dev_free(&c->log_tab); dev_free(&c->shard_vec); dev_free(&c->np_part); if (c->np_bar) { (void)hipFree(c->np_bar); c->np_bar = nullptr; } dev_free(&c->F); dev_free(&c->ntau); dev_free(&c->ntau2); dev_free(&c->ngam); dev_free(&c->ngam_raw);
    dev_free(&c->npart); dev_free(&c->nstat); dev_free(&c->ngam2); dev_free(&c->ngam_raw2);
    for (int i = 0; i < 2; ++i) { (void)hipEventDestroy(c->ev_u_ready[i]); (void)hipEventDestroy(c->ev_u_free[i]); }
    if (c->stream_rng != c->stream) (void)hipStreamDestroy(c->stream_rng);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return DSM_OK;
}

extern "C" int dsm_ctx_sync(dsm_ctx *c)
{
    if (!c) return DSM_ERR_ARG;
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream_rng));
    return DSM_OK;
}

// ---------------------------------------------------------------- data in
extern "C" int dsm_ctx_set_counts(dsm_ctx *c, const int64_t *variants, int V, int S)
{
    if (!c || !variants || V < 1 || S < 1) { dsm_set_error("set_counts: bad arguments"); return DSM_ERR_ARG; }
    if (S > DSM_MAX_S) { dsm_set_error("S=%d exceeds DSM_MAX_S=%d", S, DSM_MAX_S); return DSM_ERR_UNSUPPORTED; }
    if ((int64_t)V * S >= ((int64_t)1 << 32)) { dsm_set_error("V*S must be below 2^32"); return DSM_ERR_UNSUPPORTED; }
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream_rng));
    const size_t n = (size_t)V * S;
    c->V = V; c->S = S;
    c->have_state = false;
    c->G = 0;                       // V/S changed: every state-sized buffer is re-made by set_state
    c->big_hot = true;
    DSM_TRY(dev_alloc(&c->cnt_vs, n * 4));
    DSM_TRY(dev_alloc(&c->nitems, (size_t)S));
    DSM_TRY(dev_alloc(&c->tau, (size_t)V));
    dev_free(&c->F); dev_free(&c->ntau); dev_free(&c->ntau2); dev_free(&c->ngam); dev_free(&c->ngam_raw); c->nG = 0;
    free_traces(c);
    DevBuf<int64_t> d_in; DevBuf<int> d_flag; DevBuf<double> d_part; DevBuf<unsigned long long> d_depth;
    const int nblk = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    DSM_TRY(d_in.alloc(n * 4));
    DSM_TRY(d_flag.alloc(1));
    DSM_TRY(d_part.alloc((size_t)nblk));
    DSM_TRY(d_depth.alloc((size_t)S));
    HIP_TRY(hipMemcpyAsync(d_in, variants, n * 4 * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), c->stream));
    HIP_TRY(hipMemsetAsync(d_depth, 0, (size_t)S * sizeof(unsigned long long), c->stream));
    DSM_TRY(k_convert_counts(c, d_in, d_flag, d_part, nblk, d_depth));
    std::vector<double> part(nblk);
    std::vector<unsigned long long> dep((size_t)S);
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(part.data(), d_part, nblk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dep.data(), d_depth, (size_t)S * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // the work list of the per-read pass (spec v1) is only built if that pass ever runs (build_stats_items)
    c->items_built = false;
    c->max_items = 0;
    c->blk_gmax = 0;
    c->stats_grid = 0;
    dev_free(&c->pat_x); c->pat_x_len = 0;      // the aggregated counts of the old table's positions
    DSM_TRY(reset_blk_order(c));              // another table, another grid: no block order of the old one survives
    HIP_TRY(hipMemsetAsync(c->screen_ctl, 0, 4 * sizeof(uint32_t), c->stream));
    dev_free(&c->items);
    c->depth.assign((size_t)S, 0);
    c->max_depth = 0;
    for (int s = 0; s < S; ++s) { c->depth[s] = (int64_t)dep[s]; c->max_depth = std::max<uint64_t>(c->max_depth, dep[s]); }
    if (flag) {
        dev_free(&c->cnt_vs); dev_free(&c->items);
        dsm_set_error("set_counts: negative count or depth above 2^31-1");
        return DSM_ERR_ARG;
    }
    double s = 0.0;
    for (double p : part) s += p;
    c->ll_const = s;
    return DSM_OK;
}

// Work list of the per-read pass (spec v1, stats_kernel), built from the resident int32 tensor the first time that
// pass runs: per sample, the (variant, base) pairs with a non-zero count, sorted by decreasing count (ties: lower
// id first) -> the lanes of a wavefront run read loops of equal length (k_stats_v1 shares the resident workgroups
// among samples by depth).  One pass over the tensor in memory order fills a (count, id) list per sample; each list
// is then ordered by a counting sort on the count -- comparison sort only for samples with counts above 2^20.
// Small problems are cut into chunks of CH reads (own stream each, oracle: orc_stats_chunk): an item is then
// {id, reads | chunk << 12}; without chunking {id, reads}.
int build_stats_items(dsm_ctx *c)
{
    const int V = c->V, S = c->S;
    std::vector<int32_t> cnt((size_t)V * S * 4);
    HIP_TRY(hipMemcpyAsync(cnt.data(), c->cnt_vs, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t cells = (int64_t)V * S;
    const int CH = cells <= 65536 ? 64 : cells <= 262144 ? 128 : 0;
    c->chunked = CH != 0;
    std::vector<int32_t> nit(S);
    std::vector<std::vector<std::pair<int32_t, int32_t>>> lst((size_t)S);      // (key, id); key = reads [| chunk << 12]
    std::vector<int32_t> top(S, 0);
    for (int s = 0; s < S; ++s) lst[s].reserve((size_t)V * 2);
    for (int v = 0; v < V; ++v) {
        const int32_t *row = cnt.data() + (size_t)v * S * 4;
        for (int s = 0; s < S; ++s)
            for (int b = 0; b < 4; ++b) {
                const int64_t x = row[s * 4 + b];
                if (x <= 0) continue;
                if (!CH) {
                    lst[s].emplace_back((int32_t)x, v * 4 + b);
                    if (x > top[s]) top[s] = (int32_t)x;
                } else {
                    for (int64_t j = 0; j * CH < x; ++j) {
                        const int32_t nrd = (int32_t)(x - j * CH < CH ? x - j * CH : CH);
                        lst[s].emplace_back(nrd | (int32_t)(j << 12), v * 4 + b);
                        if (nrd > top[s]) top[s] = nrd;
                    }
                }
            }
    }
    int max_items = 0;
    for (int s = 0; s < S; ++s) max_items = std::max(max_items, (int)lst[s].size());
    c->item_stride = max_items > 0 ? max_items : 1;
    std::vector<int32_t> items((size_t)S * c->item_stride * 2, 0);
    DSM_TRY(dev_alloc(&c->items, items.size()));
    std::vector<int32_t> first;
    const int32_t rd_mask = CH ? 0xfff : 0x7fffffff;
    for (int s = 0; s < S; ++s) {
        const auto &l = lst[s];
        nit[s] = (int32_t)l.size();
        int32_t *dst = items.data() + (size_t)s * c->item_stride * 2;
        if (top[s] <= (1 << 20)) {
            first.assign((size_t)top[s] + 2, 0);
            for (const auto &e : l) first[e.first & rd_mask]++;                       // histogram of the read counts
            int32_t run = 0;
            for (int32_t cval = top[s]; cval >= 1; --cval) { const int32_t h = first[cval]; first[cval] = run; run += h; }
            for (const auto &e : l) { const int32_t k = first[e.first & rd_mask]++; dst[2 * k] = e.second; dst[2 * k + 1] = e.first; }
        } else {
            std::vector<std::pair<int32_t, int32_t>> t(l);
            std::stable_sort(t.begin(), t.end(), [](const std::pair<int32_t, int32_t> &p, const std::pair<int32_t, int32_t> &q) { return p.first > q.first; });
            for (size_t k = 0; k < t.size(); ++k) { dst[2 * k] = t[k].second; dst[2 * k + 1] = t[k].first; }
        }
    }
    c->max_items = max_items;
    c->nitems_h = nit;
    c->blk_gmax = 0;
    HIP_TRY(hipMemcpyAsync(c->items, items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->nitems, nit.data(), (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->items_built = true;
    return DSM_OK;
}

static int ensure_state_buffers(dsm_ctx *c, int G)
{
    if (G < 1 || G > DSM_MAX_G) { dsm_set_error("G=%d outside 1..%d", G, DSM_MAX_G); return DSM_ERR_UNSUPPORTED; }
    if (G != c->G || !c->gamma) {
        c->G = G;
        const size_t sg = (size_t)c->S * G;
        DSM_TRY(dev_alloc(&c->gamma, sg));
        DSM_TRY(dev_alloc(&c->gamma_star, sg));
        DSM_TRY(dev_alloc(&c->sum_mu, sg));
        HIP_TRY(hipMemsetAsync(c->sum_mu, 0, sg * sizeof(unsigned long long), c->stream));
        c->stats_grid = 0;
        c->u_cap = (size_t)c->V * G;
        // two slots of up to DSM_U_CHUNK sweeps each, at most 64 MB per slot
        c->u_chunk_words = c->u_cap * std::max<size_t>(1, std::min<size_t>(DSM_U_CHUNK, ((size_t)16 << 20) / std::max<size_t>(1, c->u_cap)));
        DSM_TRY(dev_alloc(&c->u_raw, 2 * c->u_chunk_words));
        free_traces(c);
    }
    return DSM_OK;
}

extern "C" int dsm_ctx_set_state(dsm_ctx *c, const int64_t *tau, const double *gamma, const double *eta, int G)
{
    DSM_TRY(dsm_ctx_need(c, true, false));
    if (!tau || !gamma || !eta) { dsm_set_error("set_state: null pointer"); return DSM_ERR_ARG; }
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    DSM_TRY(ensure_state_buffers(c, G));
    const size_t nt = (size_t)c->V * G * 4;
    DevBuf<int64_t> d_t;
    DSM_TRY(d_t.alloc(nt));
    HIP_TRY(hipMemcpyAsync(d_t, tau, nt * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    DSM_TRY(k_pack_tau(c, d_t, c->tau, c->V, G));
    HIP_TRY(hipMemcpyAsync(c->gamma, gamma, (size_t)c->S * G * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->tau_rare_n = tau_rare_from_host(gamma, c->S, G);
    c->big_hot = true;              // a new state: nothing is known about what stage 1 will hand over
    HIP_TRY(hipMemcpyAsync(c->eta, eta, 16 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_state = true;
    return DSM_OK;
}

extern "C" int dsm_ctx_set_gamma_eta(dsm_ctx *c, const double *gamma, const double *eta)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    BIND(c);
    if (gamma) HIP_TRY(hipMemcpyAsync(c->gamma, gamma, (size_t)c->S * c->G * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (gamma) c->tau_rare_n = tau_rare_from_host(gamma, c->S, c->G);
    c->big_hot = true;
    if (eta) HIP_TRY(hipMemcpyAsync(c->eta, eta, 16 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

static int fetch_tau(dsm_ctx *c, const uint64_t *d_packed, int64_t *host_onehot)
{
    const size_t nt = (size_t)c->V * c->G * 4;
    DevBuf<int64_t> d_t;
    DSM_TRY(d_t.alloc(nt));
    DSM_TRY(k_unpack_tau(c, d_packed, d_t, c->V, c->G));
    HIP_TRY(hipMemcpyAsync(host_onehot, d_t, nt * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_get_state(dsm_ctx *c, int64_t *tau, double *gamma, double *eta)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    BIND(c);
    if (tau) DSM_TRY(fetch_tau(c, c->tau, tau));
    if (gamma) HIP_TRY(hipMemcpyAsync(gamma, c->gamma, (size_t)c->S * c->G * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (eta) HIP_TRY(hipMemcpyAsync(eta, c->eta, 16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_set_priors(dsm_ctx *c, double alpha, double delta, double epsilon)
{
    if (!c || !(alpha > 0) || !(delta > 0) || !(epsilon >= 0)) { dsm_set_error("set_priors: bad value"); return DSM_ERR_ARG; }
    c->alpha = alpha; c->delta = delta; c->epsilon = epsilon;
    return DSM_OK;
}

// ---------------------------------------------------------------- RNG
static void mt_seed_host(uint32_t *st, unsigned long seed)
{
    if (seed == 0) seed = 4357;              // gsl_rng_set default for mt19937
    st[0] = (uint32_t)(seed & 0xffffffffUL);
    for (int i = 1; i < 624; ++i) st[i] = 1812433253u * (st[i - 1] ^ (st[i - 1] >> 30)) + (uint32_t)i;
    st[624] = 624;                           // position: refill on first use
}

static int seed_mt(dsm_ctx *c, unsigned long seed)
{
    uint32_t st[625];
    mt_seed_host(st, seed);
    HIP_TRY(hipStreamSynchronize(c->stream_rng));
    HIP_TRY(hipMemcpyAsync(c->mt_state, st, sizeof st, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mt_seeded = true;
    return DSM_OK;
}

extern "C" int dsm_ctx_seed(dsm_ctx *c, unsigned long mt_seed, uint64_t ctr_seed)
{
    if (!c) return DSM_ERR_ARG;
    BIND(c);
    c->ctr_seed = ctr_seed;
    c->iter_ctr = 0;
    return seed_mt(c, mt_seed);
}

// the two words besides (tau, gamma, eta, MT19937 state) that place a chain in its counter-based streams: the stream key and the
// number of iterations drawn so far.  With them a chain restored into a fresh context continues bit for bit (checkpoint / resume:
// SURVEY sec. 5; the reference's own hook, Output_Results.output_Pickled_haploSNP, is dead code).
// the screening state of the tau sweep (kernels_gibbs.hip: finalize_body): sweeps still to run without the fp32 screening pass, one word per
// launch parity.  Which steps are screened can decide a draw inside a ~1e-13 near-tie, so a checkpoint carries the words.
extern "C" int dsm_ctx_get_screen_state(dsm_ctx *c, uint32_t *out2)
{
    if (!c || !out2) { dsm_set_error("get_screen_state: null argument"); return DSM_ERR_ARG; }
    BIND(c);
    HIP_TRY(hipMemcpyAsync(out2, c->screen_ctl, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}
extern "C" int dsm_ctx_set_screen_state(dsm_ctx *c, const uint32_t *in2)
{
    if (!c || !in2) { dsm_set_error("set_screen_state: null argument"); return DSM_ERR_ARG; }
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->screen_ctl, in2, 2 * sizeof(uint32_t), hipMemcpyHostToDevice));
    return DSM_OK;
}

extern "C" int dsm_ctx_get_counters(dsm_ctx *c, uint64_t *ctr_seed, uint32_t *iter_ctr)
{
    if (!c || !ctr_seed || !iter_ctr) { dsm_set_error("get_counters: null argument"); return DSM_ERR_ARG; }
    *ctr_seed = c->ctr_seed; *iter_ctr = c->iter_ctr;
    return DSM_OK;
}
extern "C" int dsm_ctx_set_counters(dsm_ctx *c, uint64_t ctr_seed, uint32_t iter_ctr)
{
    if (!c) { dsm_set_error("set_counters: null context"); return DSM_ERR_ARG; }
    c->ctr_seed = ctr_seed; c->iter_ctr = iter_ctr;
    return DSM_OK;
}

extern "C" int dsm_mt_seed_state(unsigned long seed, uint32_t *state625)
{
    if (!state625) return DSM_ERR_ARG;
    mt_seed_host(state625, seed);
    return DSM_OK;
}

extern "C" int dsm_ctx_get_mt_state(dsm_ctx *c, uint32_t *state625)
{
    if (!c || !state625) return DSM_ERR_ARG;
    if (!c->mt_seeded) { dsm_set_error("tau RNG not seeded"); return DSM_ERR_STATE; }
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream_rng));
    HIP_TRY(hipMemcpyAsync(state625, c->mt_state, 625 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_set_mt_state(dsm_ctx *c, const uint32_t *state625)
{
    if (!c || !state625 || state625[624] > 624) { dsm_set_error("set_mt_state: bad state"); return DSM_ERR_ARG; }
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream_rng));
    HIP_TRY(hipMemcpyAsync(c->mt_state, state625, 625 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mt_seeded = true;
    return DSM_OK;
}

extern "C" int dsm_ctx_debug_mt_fill(dsm_ctx *c, size_t n, uint32_t *out)
{
    if (!c || (!out && n)) { dsm_set_error("debug_mt_fill: bad arguments"); return DSM_ERR_ARG; }
    if (!c->mt_seeded) { dsm_set_error("tau RNG not seeded"); return DSM_ERR_STATE; }
    if (n == 0) return DSM_OK;
    BIND(c);
    DevBuf<uint32_t> d;
    DSM_TRY(d.alloc(n));
    HIP_TRY(hipStreamSynchronize(c->stream_rng));
    DSM_TRY(k_mt_fill(c, d, n, c->stream));
    HIP_TRY(hipMemcpyAsync(out, d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_set_tau_rng(dsm_ctx *c, int mode)
{
    if (!c || (mode != DSM_RNG_MT19937 && mode != DSM_RNG_PHILOX)) { dsm_set_error("bad rng mode"); return DSM_ERR_ARG; }
    c->tau_rng = mode;
    return DSM_OK;
}

// The MT19937 words of the tau sweeps of one call.  The stream is serial, but a call knows how many sweeps it will run
// (`per` words each), so the side stream generates them in CHUNKS of several sweeps, one chunk ahead of the reader, into two
// slots: one cross-stream event pair per chunk instead of per sweep (each pair costs a bubble of several microseconds
// between two launches of the main stream).  Chunks start small so that the first sweep is not kept waiting and grow
// by <= 1.5x, slower than the generator outruns the fastest reader (the 82 us tau-only sweeps of updateTau vs 50 us per fill).
struct SweepWords {
    dsm_ctx *c;
    int total;
    size_t per;                                         // words per sweep: c->u_cap = V*G, or V*F of a held sweep (the slots are sized for V*G)
    int filled = 0, nchunk = 0;
    int first[2] = {0, 0}, len[2] = {0, 0};             // sweeps held by each slot
    int max_len = 1;
    SweepWords(dsm_ctx *ctx, int n_sweeps, size_t words_per_sweep) : c(ctx), total(n_sweeps), per(words_per_sweep)
    {
        max_len = (int)std::max<size_t>(1, std::min<size_t>(DSM_U_CHUNK, c->u_chunk_words / std::max<size_t>(1, per)));
    }
    bool active() const { return c->tau_rng == DSM_RNG_MT19937; }
    int fill_next()
    {
        static const int grow[] = {1, 2, 3, 4, 6, 8};
        int want = grow[std::min(nchunk, 5)];
        want = std::min(std::min(want, max_len), total - filled);
        const int slot = nchunk & 1;
        uint32_t *buf = c->u_raw + (size_t)slot * c->u_chunk_words;
        HIP_TRY(hipStreamWaitEvent(c->stream_rng, c->ev_u_free[slot], 0));   // the last reader of this slot is done
        DSM_TRY(k_mt_fill(c, buf, (size_t)want * per, c->stream_rng));
        HIP_TRY(hipEventRecord(c->ev_u_ready[slot], c->stream_rng));
        first[slot] = filled; len[slot] = want;
        filled += want; ++nchunk;
        return DSM_OK;
    }
    // start generating before the main stream gets to the first sweep
    int prefetch()
    {
        if (!active() || filled > 0 || total < 1) return DSM_OK;
        if (!c->mt_seeded) { dsm_set_error("tau RNG not seeded: call dsm_ctx_seed / dsm_setRNG"); return DSM_ERR_STATE; }
        return fill_next();
    }
    // words of sweep `it` (sweeps must be asked for in order); makes the main stream wait for the chunk at its first sweep
    int acquire(int it, const uint32_t **u)
    {
        *u = nullptr;
        if (!active()) return DSM_OK;
        if (!c->mt_seeded) { dsm_set_error("tau RNG not seeded: call dsm_ctx_seed / dsm_setRNG"); return DSM_ERR_STATE; }
        if (it >= filled) DSM_TRY(fill_next());
        int slot = (it >= first[0] && it < first[0] + len[0] && len[0]) ? 0 : 1;
        if (!(it >= first[slot] && it < first[slot] + len[slot])) { dsm_set_error("sweep words asked out of order"); return DSM_ERR_STATE; }
        if (it == first[slot]) {
            if (filled < total) DSM_TRY(fill_next());            // keep one chunk ahead (into the other slot)
            HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_u_ready[slot], 0));
        }
        *u = c->u_raw + (size_t)slot * c->u_chunk_words + (size_t)(it - first[slot]) * per;
        return DSM_OK;
    }
    int release(int it)
    {
        if (!active()) return DSM_OK;
        for (int slot = 0; slot < 2; ++slot)
            if (len[slot] && it == first[slot] + len[slot] - 1) HIP_TRY(hipEventRecord(c->ev_u_free[slot], c->stream));
        return DSM_OK;
    }
};

// ---------------------------------------------------------------- single steps
// One sweep of the resident state with the resident gamma / eta over haplotypes 0 .. G - n_held - 1: the full sweep (n_held = 0, the
// only one with logp_out) or the held sweep of DESIGN.md sec. 8e, which consumes V F words of the MT19937 stream instead of V G.
static int sample_tau_once(dsm_ctx *c, int n_held, int *nchange, double *logp_out)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (n_held < 0 || n_held > c->G) { dsm_set_error("sample_tau_held: n_held = %d outside 0..%d", n_held, c->G); return DSM_ERR_ARG; }
    if (n_held == c->G) { c->iter_ctr++; if (nchange) *nchange = 0; return DSM_OK; }      // a sweep over no haplotype
    BIND(c);
    DevBuf<double> d_logp;
    const size_t nl = (size_t)c->V * c->G * 4;
    if (logp_out) DSM_TRY(d_logp.alloc(nl));
    const uint32_t *u = nullptr;
    SweepWords words(c, 1, n_held ? (size_t)c->V * (c->G - n_held) : c->u_cap);
    HIP_TRY(hipMemsetAsync(c->nchange, 0, sizeof(int), c->stream));
    DSM_TRY(words.acquire(0, &u));
    DSM_TRY(n_held ? k_held_sweep(c, n_held, c->gamma, c->eta, c->iter_ctr++, u)
               : k_tau_sweep(c, 1, c->gamma, c->eta, c->eta, nullptr, d_logp, c->iter_ctr++, nullptr, u));
    DSM_TRY(words.release(0));
    int n = 0;
    HIP_TRY(hipMemcpyAsync(&n, c->nchange, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (logp_out) HIP_TRY(hipMemcpyAsync(logp_out, d_logp, nl * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->nchange, 0, sizeof(int), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nchange) *nchange = n;
    return DSM_OK;
}

extern "C" int dsm_ctx_sample_tau(dsm_ctx *c, int *nchange, double *logp_out) { return sample_tau_once(c, 0, nchange, logp_out); }
extern "C" int dsm_ctx_sample_tau_held(dsm_ctx *c, int n_held, int *nchange) { return sample_tau_once(c, n_held, nchange, nullptr); }

// ---- pair moves of the main chain (kernels_pairtau.hip)
extern "C" int dsm_ctx_set_pair_moves(dsm_ctx *c, int every)
{
    if (!c) { dsm_set_error("set_pair_moves: null context"); return DSM_ERR_ARG; }
    if (every < 0) { dsm_set_error("set_pair_moves: every = %d is negative", every); return DSM_ERR_ARG; }
    c->pair_every = every;
    return DSM_OK;
}
extern "C" int dsm_ctx_get_pair_moves(dsm_ctx *c, int *every)
{
    if (!c || !every) { dsm_set_error("get_pair_moves: null argument"); return DSM_ERR_ARG; }
    *every = c->pair_every;
    return DSM_OK;
}
// one pair pass on the resident state with the resident gamma / eta, keyed by `iter`: neither the MT19937 stream nor the iteration
// counter moves
extern "C" int dsm_ctx_sample_tau_pairs(dsm_ctx *c, uint32_t iter, int *nchange)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    BIND(c);
    HIP_TRY(hipMemsetAsync(c->nchange, 0, sizeof(int), c->stream));
    DSM_TRY(k_pair_sweep(c, c->gamma, c->eta, iter));
    int n = 0;
    HIP_TRY(hipMemcpyAsync(&n, c->nchange, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->nchange, 0, sizeof(int), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nchange) *nchange = n;
    return DSM_OK;
}

extern "C" int dsm_ctx_sample_stats(dsm_ctx *c, uint32_t iter, uint64_t *sum_mu, uint64_t *esum)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    BIND(c);
    const size_t sg = (size_t)c->S * c->G;
    HIP_TRY(hipMemsetAsync(c->sum_mu, 0, sg * sizeof(unsigned long long), c->stream));
    DSM_TRY(stats_ensure_ntab(c));
    DSM_TRY(esum_reset(c));
    // (the launch of stats_big_kernel left out where the context says so: stage 2 then draws the deferred items, the same sums)
    DSM_TRY(k_stats(c, iter, !(stats_big_optional(c) && !stats_big_wanted(c))));
    DSM_TRY(k_esum_fold(c));
    if (sum_mu) HIP_TRY(hipMemcpyAsync(sum_mu, c->sum_mu, sg * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (esum) HIP_TRY(hipMemcpyAsync(esum, c->esum, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->sum_mu, 0, sg * sizeof(unsigned long long), c->stream));
    DSM_TRY(esum_reset(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_stats_spec(dsm_ctx *c)
{
    if (!c || c->G < 1) { dsm_set_error("stats_spec: no chain state"); return DSM_ERR_STATE; }
    return stats_spec(c);
}

extern "C" int dsm_ctx_force_stats_spec(dsm_ctx *c, int spec)
{
    if (!c || spec < 0 || spec > 4) { dsm_set_error("force_stats_spec: 0 (rule), 1, 2, 3 or 4"); return DSM_ERR_ARG; }
    c->force_stats_spec = spec;
    return DSM_OK;
}

extern "C" int dsm_ctx_debug_stage1(dsm_ctx *c, uint32_t iter, uint32_t *ntab, uint64_t *esum)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (stats_spec(c) < 2) { dsm_set_error("debug_stage1: the aggregated specification does not apply to this shape (force it with dsm_ctx_force_stats_spec)"); return DSM_ERR_UNSUPPORTED; }
    BIND(c);
    DSM_TRY(esum_reset(c));
    DSM_TRY(k_stats_stage1(c, iter));
    DSM_TRY(k_esum_fold(c));
    const size_t NH = (size_t)1 << c->G, S = (size_t)c->S;
    const size_t ld = (size_t)c->ntab_ld;
    std::vector<uint32_t> t((size_t)c->ntab_rep * NH * ld);
    HIP_TRY(hipMemcpyAsync(t.data(), c->ntab, t.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (esum) HIP_TRY(hipMemcpyAsync(esum, c->esum, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->ntab, 0, t.size() * sizeof(uint32_t), c->stream));
    DSM_TRY(esum_reset(c));
    HIP_TRY(hipMemsetAsync(c->big_count, 0, DSM_BIG_NT * DSM_BIG_NL * DSM_BIG_STRIDE * sizeof(uint32_t), c->stream));     // (the running count of non-empty lists with them)
    c->big_seen = 0; c->big_hot = true;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ntab)
        for (size_t h = 0; h < NH; ++h)
            for (size_t s = 0; s < S; ++s) {                                       // device [rep][H][S] -> [S][H], copies summed
                uint32_t v = 0;
                for (int r = 0; r < c->ntab_rep; ++r) v += t[((size_t)r * NH + ((h * DSM_NTAB_HMUL + (s >> 4) * DSM_NTAB_SWZ) & (NH - 1))) * ld + s];
                ntab[s * NH + h] = v;
            }
    return DSM_OK;
}

extern "C" int dsm_ctx_debug_binom(dsm_ctx *c, int kind, uint32_t n, const double *w4, uint64_t seed, int nsamp, uint32_t *out, int spec)
{
    if (!c || !w4 || !out || nsamp < 1 || kind < 0 || kind > 2 || spec < 2 || spec > 3) { dsm_set_error("debug_binom: bad arguments"); return DSM_ERR_ARG; }
    BIND(c);
    const size_t len = (size_t)nsamp * (kind == 2 ? 4 : 1);
    DevBuf<uint32_t> d;
    DSM_TRY(d.alloc(len));
    DSM_TRY(k_binom_test(c, kind, n, w4, seed, nsamp, d, spec));
    HIP_TRY(hipMemcpyAsync(out, d, len * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_draw_gamma_eta(dsm_ctx *c, uint32_t iter, const uint64_t *sum_mu, const uint64_t *esum,
                                      double *gamma_out, double *eta_out)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (!sum_mu || !esum) { dsm_set_error("draw_gamma_eta: null sums"); return DSM_ERR_ARG; }
    BIND(c);
    const size_t sg = (size_t)c->S * c->G;
    DevBuf<double> d_g, d_e;
    DSM_TRY(d_g.alloc(sg));
    DSM_TRY(d_e.alloc(16));
    HIP_TRY(hipMemcpyAsync(c->sum_mu, sum_mu, sg * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->esum, esum, 16 * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    DSM_TRY(k_dirichlet(c, iter, d_g, nullptr, d_e, nullptr, c->prior, -1, 0, nullptr));
    if (gamma_out) HIP_TRY(hipMemcpyAsync(gamma_out, d_g, sg * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (eta_out) HIP_TRY(hipMemcpyAsync(eta_out, d_e, 16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// ll / lp of (resident tau, gamma, eta) -> scalars[0..1]; star untouched unless it<0
static int eval_state(dsm_ctx *c, const double *gamma, const double *eta, uint64_t *trace_slot, int star_mode)
{
    int nb = 0;
    DSM_TRY(k_prior(c, gamma, eta, c->prior));
    DSM_TRY(k_tau_sweep(c, 2, gamma, eta, eta, trace_slot, nullptr, 0, &nb, nullptr));
    return k_finalize(c, nb, -1, star_mode, c->prior, gamma, eta);
}

extern "C" int dsm_ctx_loglik(dsm_ctx *c, double *ll, double *lp)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    BIND(c);
    double sc[2];
    DSM_TRY(eval_state(c, c->gamma, c->eta, nullptr, 2));     // star_mode 2: MAP record untouched
    HIP_TRY(hipMemcpyAsync(sc, c->scalars, sizeof sc, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ll) *ll = sc[0];
    if (lp) *lp = sc[1];
    return DSM_OK;
}

// ---------------------------------------------------------------- update loops
int alloc_traces(dsm_ctx *c, int n)
{
    // buffers are kept across update() calls and only grown (hipMalloc/hipFree cost milliseconds)
    const size_t sg = (size_t)c->S * c->G;
    if (n > c->trace_cap || !c->tau_trace) {
        free_traces(c);
        // room for at least 512 iterations while the tau trace stays below 1 GB: a driver that calls update() with a
        // growing iteration count (burn-in 5, then 20, ...) does not pay hipFree + hipMalloc (~1 ms) inside every call
        const int want = n;
        if (n < 512 && (size_t)513 * c->V * sizeof(uint64_t) <= ((size_t)1 << 30)) n = 512;
        DSM_TRY(dev_alloc(&c->tau_trace, (size_t)(n + 1) * c->V));
        DSM_TRY(dev_alloc(&c->ll_trace, (size_t)n));
        DSM_TRY(dev_alloc(&c->lp_trace, (size_t)n));
        DSM_TRY(dev_alloc(&c->nchange_trace, (size_t)n));
        DSM_TRY(dev_alloc(&c->gamma_trace, (size_t)n * sg));
        DSM_TRY(dev_alloc(&c->eta_trace, (size_t)n * 16));
        c->trace_cap = n;
        n = want;
    }
    c->n_trace = n;
    c->tau_fixed_trace = false;             // (the fixed-tau chain sets it after this call)
    return DSM_OK;
}

// ---------------------------------------------------------------- chains of one call
// What the launchers read to batch (dsm_host.h: LAUNCH_OR_COLLECT); written only by Chains::launch.
thread_local BatchCtl g_batch;

// The chains of one update call: one context on its own (the dsm_ctx_* entry points: plain launches), or K contexts of one shape
// (dsm_batch_*: one launch per kernel for all of them, chain = blockIdx.y), each moved onto the leader's streams with timing off for
// the duration of the call.  The destructor drains the leader's streams and puts every moved context back, on every return path.
struct Chains {
    dsm_ctx *const *c;
    int K;
    bool batched;
    struct Home { hipStream_t stream, stream_rng; bool timing; int nmft_fused; };
    std::vector<Home> home;                 // the moved chains' own settings
    dsm_ctx *lead() const { return c[0]; }
    ~Chains()
    {
        if (home.empty()) return;
        (void)hipStreamSynchronize(lead()->stream);
        (void)hipStreamSynchronize(lead()->stream_rng);
        for (size_t k = 0; k < home.size(); ++k) {
            c[k]->stream = home[k].stream; c[k]->stream_rng = home[k].stream_rng; c[k]->timing = home[k].timing; c[k]->nmft_fused = home[k].nmft_fused;
        }
    }
    // Checks the chains (state: a chain state is needed; fits(lead, c, k): the caller's own checks of chain k) and, batched, moves them
    // onto the leader's streams; nmft: with the leader's launch form of the NMF update.
    template <class Fits> int open(bool state, bool nmft, Fits fits)
    {
        if (!c || K < 1 || K > DSM_MAX_BATCH) { dsm_set_error("batch of %d chains (1..%d)", K, DSM_MAX_BATCH); return DSM_ERR_ARG; }
        for (int k = 0; k < K; ++k) {
            DSM_TRY(dsm_ctx_need(c[k], true, state));
            const dsm_ctx *a = c[0], *b = c[k];
            if (b->device != a->device || b->V != a->V || b->S != a->S) { dsm_set_error("batch: chain %d differs from chain 0 in device or shape", k); return DSM_ERR_ARG; }
            DSM_TRY(fits(a, b, k));
            for (int j = 0; j < k; ++j) if (c[j] == b) { dsm_set_error("batch: chain %d listed twice", k); return DSM_ERR_ARG; }
        }
        BIND(lead());
        for (int k = 0; batched && k < K; ++k) {
            HIP_TRY(hipStreamSynchronize(c[k]->stream));
            HIP_TRY(hipStreamSynchronize(c[k]->stream_rng));
            home.push_back(Home{c[k]->stream, c[k]->stream_rng, c[k]->timing, c[k]->nmft_fused});
            c[k]->stream = lead()->stream; c[k]->stream_rng = lead()->stream_rng; c[k]->timing = false;
            if (nmft) c[k]->nmft_fused = home[0].nmft_fused;
        }
        return DSM_OK;
    }
    // f(chain, k) chain by chain, each launch its own
    template <class F> int each(F f) const
    {
        for (int k = 0; k < K; ++k) DSM_TRY(f(c[k], k));
        return DSM_OK;
    }
    // f(chain, k) for every chain; batched, what each launcher f calls collects from the chains goes out as one launch
    template <class F> int launch(F f) const
    {
        int r = DSM_OK;
        for (int k = 0; k < K && r == DSM_OK; ++k) {
            if (batched) g_batch = BatchCtl{K, k};
            r = f(c[k], k);
        }
        g_batch = BatchCtl{};
        return r;
    }
};

// the chains of a Gibbs or update_tau batch also share G and the tau RNG
static int same_G_and_rng(const dsm_ctx *a, const dsm_ctx *b, int k)
{
    if (b->G != a->G || b->tau_rng != a->tau_rng) { dsm_set_error("batch: chain %d differs from chain 0 in shape or tau RNG", k); return DSM_ERR_ARG; }
    return DSM_OK;
}

// the Dirichlet log-prior terms of iteration it (two slots, by parity)
static double *prior_slot(dsm_ctx *c, int it) { return c->prior + (it & 1) * (DSM_MAX_S + 4); }

// The tau step of a Gibbs iteration: the LAST n_held haplotypes are held.  0 = the full chain (the sweep and the likelihood of the new
// state are one launch: k_tau_sweep mode 3); 0 < n_held < G = the partly held chain (k_held_sweep, V F words of the
// MT19937 stream per sweep, then the likelihood-only pass, k_tau_sweep mode 2, which also stores tau); n_held = G = tau fixed
// (HaploSNP_Sampler.py:409-428, update_fixed_tau; sec. 8c: no sweep, no word generated or consumed, the likelihood-only pass, tau stored
// once -- dsm_host.h: tau_fixed_trace).  fix_eta (n_held > 0 only): the E sums and the eta draw are still made, but the chain's eta, the
// trace rows, the prior terms, the sweep and the likelihood all stay at the matrix the call came in with.
struct TauStep { int n_held = 0; bool fix_eta = false; };

// The Gibbs loop of one chain (unbatched) or of K chains of one shape sharing every launch of the iteration.  A chain ends in the same
// state either way: the mu/E specification is the chain's own (round 5; the per-read pass of small or shallow tables and of G > 16 is
// launched chain by chain, everything else is shared).  Per iteration: the mu/E pass at (tau, gamma, eta), the Dirichlet launch (gamma_new,
// eta_new, traces, prior terms; it finalizes the previous iteration), the tau step.
static int gibbs_update(dsm_ctx *const *ctxs, int K, bool batched, int n_iter, TauStep step = TauStep{})
{
    if (n_iter < 0) { dsm_set_error("n_iter < 0"); return DSM_ERR_ARG; }
    if (batched && step.n_held) { dsm_set_error("batch: no held haplotypes (the held sweep has no batched form)"); return DSM_ERR_UNSUPPORTED; }
    Chains ch{ctxs, K, batched};
    DSM_TRY(ch.open(true, false, [batched](const dsm_ctx *a, const dsm_ctx *b, int k) -> int {
        DSM_TRY(same_G_and_rng(a, b, k));
        if (batched && b->pair_every > 0) {
            dsm_set_error("batch: chain %d has pair moves on (dsm_ctx_set_pair_moves: every = %d); the pair pass has no batched form", k, b->pair_every);
            return DSM_ERR_UNSUPPORTED;
        }
        // one specification per batch (the launches are shared): chains of one shape on one table have the same by rule
        if (stats_spec(b) == stats_spec(a)) return DSM_OK;
        dsm_set_error("batch: chain %d runs mu/E specification %d, chain 0 specification %d (different tables or different dsm_ctx_force_stats_spec)", k, stats_spec(b), stats_spec(a));
        return DSM_ERR_ARG;
    }));
    dsm_ctx *const lead = ch.lead();
    const bool full = step.n_held == 0, fixed = step.n_held == lead->G, fix_eta = step.fix_eta && !full;
    // pair moves belong to the full chain run alone; the fixed-tau chain has no tau step and ignores the setting
    if (!full && !fixed && lead->pair_every > 0) {
        dsm_set_error("gibbs_update_held_tau: pair moves are on (dsm_ctx_set_pair_moves: every = %d); the pair pass has no held form", lead->pair_every);
        return DSM_ERR_UNSUPPORTED;
    }
    const uint32_t pair_E = (full && !batched && lead->G > 1) ? (uint32_t)lead->pair_every : 0u;
    const int spec = stats_spec(lead);
    // sampleMu (:341): spec v2 = stage 1, then stage 2 inside the Dirichlet launch; spec v1 = the per-read pass
    const bool agg = spec >= 2;
    const bool fuse_s2 = agg && lead->G < 10;           // many subsets per sample: stage 2 as its own 1024-thread launch
    const size_t sg = (size_t)lead->S * lead->G;
    // The launch of stats_big_kernel after stage 1 is a choice for the full chain whose Dirichlet launch runs stage 2 (it then draws what
    // the deferred lists hold itself).  Chains with G >= 10, specification 1 or 4, sharded chains and the held and fixed-tau chains keep
    // the launch unconditionally (kernels_stats.hip: stats_big_optional).  The choice is one of speed only; a batch launches if any
    // of its chains would.
    const bool big_opt = full && fuse_s2 && stats_big_optional(lead);
    auto big_wanted = [&]() { bool w = !big_opt; for (int k = 0; k < K; ++k) w = w || stats_big_wanted(ctxs[k]); return w; };
    bool launch_big = big_wanted();
    const bool big_auto = big_opt && !batched && stats_big_mode(lead) == -1;       // (not forced: the next look can change the choice)
    // the MT19937 words of the sweeps are generated on the side stream, chunks of sweeps ahead (never beyond the last sweep
    // of the call: the stream position must equal the reference's)
    std::vector<SweepWords> words;
    words.reserve(K);
    std::vector<int> nb_prev(K, 0);
    std::vector<uint32_t> ic(K);
    std::vector<const uint32_t *> u(K, nullptr);
    DevBuf<double> held;                               // fix_eta: the four prior terms of the held matrix
    DSM_TRY(ch.each([&](dsm_ctx *c, int) -> int {
        DSM_TRY(alloc_traces(c, n_iter));
        c->tau_fixed_trace = fixed;
        HIP_TRY(hipMemsetAsync(c->nchange, 0, sizeof(int), c->stream));
        if (!full) {
            HIP_TRY(hipMemsetAsync(c->sum_mu, 0, sg * sizeof(unsigned long long), c->stream));
            DSM_TRY(esum_reset(c));                         // Esum and every partial copy of it (a failed pass may have left counts there)
        }
        // entry state: ll, lp, storeStarState(0)  (HaploSNP_Sampler.py:336-338); tau -> slot 0 of the trace
        DSM_TRY(eval_state(c, c->gamma, c->eta, c->tau_trace, 1));
        DSM_TRY(stats_ensure_ntab(c));
        if (full && !batched) DSM_TRY(k_tau_neartie_hint(c));   // which instantiation of the full sweep this call runs (same draws either way)
        if (fix_eta && n_iter > 0) {
            DSM_TRY(held.alloc((size_t)c->S + 4));
            DSM_TRY(k_prior(c, c->gamma, c->eta, held));
            DSM_TRY(k_fixtau_fill_eta(c, c->eta, c->eta_trace, n_iter));
        }
        words.emplace_back(c, fixed ? 0 : n_iter, full ? c->u_cap : (size_t)c->V * (c->G - step.n_held));
        return DSM_OK;
    }));
    DSM_TRY(ch.launch([&](dsm_ctx *, int k) { return words[k].prefetch(); }));
    for (int it = 0; it < n_iter; ++it) {
        // (the abundances move during a burn-in: the choice of the full sweep's instantiation is looked at again now and then -- a stream
        // synchronisation and a 4-byte read-back every 64 iterations; the draws do not depend on it)
        // (the same look tells whether stage 1 still hands items over: a settled chain drops the launch of stats_big_kernel, at most 64 iterations late)
        if (full && !batched && it && (it & 63) == 0 && (lead->tau_neartie_mode == -1 || big_auto)) {
            DSM_TRY(k_tau_rare_count(lead, true)); DSM_TRY(k_tau_neartie_hint(lead));
            launch_big = big_wanted();
        }
        DSM_TRY(ch.launch([&](dsm_ctx *c, int k) { ic[k] = c->iter_ctr++; return agg ? k_stats_stage1(c, ic[k], launch_big) : k_stats_v1(c, ic[k]); }));
        if (agg && !fuse_s2) DSM_TRY(ch.launch([&](dsm_ctx *c, int k) { return k_stats_stage2(c, ic[k]); }));
        // sampleGamma (:342) + the eta draw (:347: eta depends only on the E sums) + traces; the same
        // launch finalizes iteration it-1 (ll, lp, MAP test :349-353) in one extra workgroup
        DSM_TRY(ch.launch([&](dsm_ctx *c, int k) {
            return k_dirichlet(c, ic[k], c->gamma, c->gamma_trace + (size_t)it * sg, c->eta_new, fix_eta ? nullptr : c->eta_trace + (size_t)it * 16,
                               prior_slot(c, it), it - 1, nb_prev[k], prior_slot(c, it - 1), fuse_s2 ? 1 : 0);
        }));
        // tau sweep with (gamma_new, eta_old) (:345); the full sweep's launch is also the log-likelihood of the new state with eta_new (:349)
        if (!fixed) {
            DSM_TRY(ch.launch([&](dsm_ctx *, int k) { return words[k].acquire(it, &u[k]); }));
            DSM_TRY(ch.launch([&](dsm_ctx *c, int k) {
                if (!full) return k_held_sweep(c, step.n_held, c->gamma, c->eta, ic[k], u[k]);
                return k_tau_sweep(c, 3, c->gamma, c->eta, c->eta_new, c->tau_trace + (size_t)(it + 1) * c->V, nullptr, ic[k], &nb_prev[k], u[k]);
            }));
            DSM_TRY(ch.each([&](dsm_ctx *, int k) { return words[k].release(it); }));
        }
        // a pair iteration: the pair pass with the (gamma_new, eta_old) the sweep conditioned on; the likelihood of the state it leaves
        // takes the likelihood-only pass below, which overwrites what the sweep's launch stored (tau's trace slot, the ll partials)
        const bool pair_it = pair_E && (ic[0] + 1u) % pair_E == 0;
        if (pair_it) DSM_TRY(k_pair_sweep(lead, lead->gamma, lead->eta, ic[0]));
        DSM_TRY(ch.each([&](dsm_ctx *c, int) -> int {
            if (fix_eta) HIP_TRY(hipMemcpyAsync(prior_slot(c, it) + c->S, held.p + c->S, 4 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            else std::swap(c->eta, c->eta_new);                          // eta_new becomes the chain's eta
            return DSM_OK;
        }));
        // held and fixed: the likelihood-only pass at (tau_new, gamma_new, eta_new); it stores tau_new where tau moves
        if (!full || pair_it)
            DSM_TRY(ch.each([&](dsm_ctx *c, int k) {
                return k_tau_sweep(c, 2, c->gamma, c->eta, c->eta, fixed ? nullptr : c->tau_trace + (size_t)(it + 1) * c->V, nullptr, 0, &nb_prev[k], nullptr);
            }));
    }
    // the last iteration's finalize launch of a chain run alone also counts the haplotypes that are rare in every sample -- what the next
    // call's choice of sweep instantiation goes by -- straight into the host's pinned word: it rides on this call's own launch and synchronisation
    const bool want_rare = !batched && n_iter > 0 && lead->tau_neartie_mode == -1;
    // ... and, for every chain whose launch of stats_big_kernel is a choice, the device's count of deferred lists found non-empty
    const bool want_big = big_opt && n_iter > 0;
    DSM_TRY(ch.each([&](dsm_ctx *c, int) -> int {
        if ((want_rare || want_big) && !c->h_rare) HIP_TRY(hipHostMalloc((void **)&c->h_rare, 2 * sizeof(int), hipHostMallocDefault));
        return DSM_OK;
    }));
    if (n_iter > 0)
        DSM_TRY(ch.each([&](dsm_ctx *c, int k) {
            return k_finalize(c, nb_prev[k], n_iter - 1, 0, prior_slot(c, n_iter - 1), c->gamma_trace + (size_t)(n_iter - 1) * sg,
                              c->eta_trace + (size_t)(n_iter - 1) * 16, 0, want_rare ? c->h_rare : nullptr, want_big ? c->h_rare + 1 : nullptr);
        }));
    HIP_TRY(hipStreamSynchronize(lead->stream));
    if (!full && !fixed) HIP_TRY(hipStreamSynchronize(lead->stream_rng));
    if (want_rare) lead->tau_rare_n = *lead->h_rare;
    if (want_big) DSM_TRY(ch.each([&](dsm_ctx *c, int) -> int { stats_big_take(c, (uint32_t)c->h_rare[1]); return DSM_OK; }));
    return DSM_OK;
}

extern "C" int dsm_ctx_gibbs_update(dsm_ctx *c, int n_iter) { return gibbs_update(&c, 1, false, n_iter); }

// K chains of one shape (same device, V, S, G, tau RNG), one launch per kernel of the iteration for all of them: on tables that leave
// most of the GPU idle -- a few hundred to a few thousand positions, the usual DESMAN input -- the replicate chains of a G value
// (scripts/runDesman.sh:15-21) then cost little more than one.  Every chain ends in the state dsm_ctx_gibbs_update leaves it in.
extern "C" int dsm_batch_gibbs_update(dsm_ctx *const *ctxs, int K, int n_iter) { return gibbs_update(ctxs, K, true, n_iter); }

// ONE chain sharded over several GPUs by positions (last row: for chains < GPUs).  This context holds positions
// v_offset .. v_offset + V of a table of v_total; gamma / eta are replicated.  Per iteration the shards exchange, through
// `exchange` (the caller's all-reduce: RCCL via torch.distributed in desman_amd/vshard.py), the subset table of the mu/E pass
// (uint32 [rep][2^G][S], summed: stage 2 and the gamma / eta draws then run replicated and bit-identical on every shard)
// and an 18-double vector {log-likelihood and changed pairs of the previous sweep, Esum}.  Counter-based streams are keyed by
// GLOBAL cell / position indices, so the chain does not depend on how it is sharded: every shard's tau equals the slice of the
// unsharded chain's, gamma / eta / traces equal it bit for bit (ll, lp to rounding: sums of shard sums).  Requires the
// aggregated mu/E pass and counter-based tau uniforms (dsm_ctx_set_tau_rng(DSM_RNG_PHILOX): the MT19937 stream is serial).
// exchange(user, tab, n_tab, vec, n_vec) is called with this context's stream drained; it must return (0 = ok) only after
// the reduced values are in place.  n_tab = 0: only the vector is exchanged.
struct dsm_comm;
int comm_enqueue_exchange(dsm_comm *m, uint32_t *tab, size_t n_tab, double *vec, size_t n_vec, hipStream_t stream);   // comm.hip
int comm_device(const dsm_comm *m);

// the loop of both forms: exchange != null -- the caller's all-reduce, called with the stream drained; comm != null -- RCCL
// all-reduces enqueued on the chain's stream by the library (no host synchronisation inside the loop)
// (not run through gibbs_update: its exchanges sit between stage 1 and stage 2 and around every finalize -- hooks there, no code saved)
static int gibbs_update_sharded(dsm_ctx *c, int n_iter, int v_offset, int v_total, dsm_exchange_fn exchange, void *user, dsm_comm *comm)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (c->pair_every > 0) {
        dsm_set_error("gibbs_update_sharded: pair moves are on (dsm_ctx_set_pair_moves: every = %d); the pair pass has no sharded form", c->pair_every);
        return DSM_ERR_UNSUPPORTED;
    }
    c->tau_neartie_on = false;                           // (a sharded chain runs the sweep's plain instantiation)
    if (n_iter < 0 || (!exchange && !comm) || v_offset < 0 || v_total < v_offset + c->V) { dsm_set_error("gibbs_update_sharded: bad arguments"); return DSM_ERR_ARG; }
    if (comm && comm_device(comm) != c->device) { dsm_set_error("gibbs_update_sharded: the communicator lives on device %d, the context on %d", comm_device(comm), c->device); return DSM_ERR_ARG; }
    if (c->tau_rng != DSM_RNG_PHILOX) { dsm_set_error("gibbs_update_sharded: needs counter-based tau uniforms (DSM_RNG_PHILOX)"); return DSM_ERR_STATE; }
    BIND(c);
    const int keep_force = c->force_stats_spec;
    if (c->force_stats_spec < 2) c->force_stats_spec = DSM_STATS_AGG;          // the aggregated pass whatever the shard's size
    struct Guard { dsm_ctx *c; int f; ~Guard() { c->shard_on = false; c->force_stats_spec = f; } } guard{c, keep_force};
    if (stats_spec(c) < 2) { dsm_set_error("gibbs_update_sharded: the aggregated mu/E pass does not apply to this shape (G <= 16)"); return DSM_ERR_UNSUPPORTED; }
    if (!c->shard_vec) DSM_TRY(dev_alloc(&c->shard_vec, (size_t)18));
    // shard_on before anything sizes the subset table: its layout (copies, row stride) must be the same on every rank -- it is
    // derived from v_total, S and G, never from this shard's own V (kernels_stats.hip: stats_ntab_rep)
    c->shard_on = true; c->shard_voff = v_offset; c->shard_vtot = v_total;
    DSM_TRY(alloc_traces(c, n_iter));
    const size_t sg = (size_t)c->S * c->G;
    HIP_TRY(hipMemsetAsync(c->nchange, 0, sizeof(int), c->stream));
    DSM_TRY(esum_reset(c));
    auto swap_vec = [&](uint32_t *tab, size_t n_tab) -> int {
        if (comm) return comm_enqueue_exchange(comm, tab, n_tab, c->shard_vec, (size_t)18, c->stream);
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (exchange(user, tab, n_tab, c->shard_vec, (size_t)18) != 0) { dsm_set_error("gibbs_update_sharded: the exchange callback failed"); return DSM_ERR_STATE; }
        return DSM_OK;
    };
    // entry state: ll, lp of the WHOLE table, storeStarState(0)
    {
        int nb = 0;
        DSM_TRY(k_prior(c, c->gamma, c->eta, c->prior));
        DSM_TRY(k_tau_sweep(c, 2, c->gamma, c->eta, c->eta, c->tau_trace, nullptr, 0, &nb, nullptr));
        DSM_TRY(k_shard_pack(c, nb));
        DSM_TRY(swap_vec(nullptr, 0));
        DSM_TRY(k_finalize(c, nb, -1, 1, c->prior, c->gamma, c->eta));
        DSM_TRY(esum_reset(c));
    }
    DSM_TRY(stats_ensure_ntab(c));
    const bool fuse_s2 = c->G < 10;
    int nb_prev = 0;
    for (int it = 0; it < n_iter; ++it) {
        const uint32_t ic = c->iter_ctr++;
        DSM_TRY(k_stats_stage1(c, ic));                                   // this shard's cells -> its subset table and Esum
        DSM_TRY(k_shard_pack(c, nb_prev));                                // + ll / nchange of the previous sweep
        DSM_TRY(swap_vec(c->ntab, c->ntab_len));
        DSM_TRY(k_shard_unpack(c));
        if (!fuse_s2) DSM_TRY(k_stats_stage2(c, ic));
        DSM_TRY(k_dirichlet(c, ic, c->gamma, c->gamma_trace + (size_t)it * sg, c->eta_new, c->eta_trace + (size_t)it * 16,
                        prior_slot(c, it), it - 1, nb_prev, prior_slot(c, it - 1), fuse_s2 ? 1 : 0));
        DSM_TRY(k_tau_sweep(c, 3, c->gamma, c->eta, c->eta_new, c->tau_trace + (size_t)(it + 1) * c->V, nullptr, ic, &nb_prev, nullptr));
        std::swap(c->eta, c->eta_new);
    }
    if (n_iter > 0) {
        DSM_TRY(k_shard_pack(c, nb_prev));
        DSM_TRY(swap_vec(nullptr, 0));
        DSM_TRY(k_finalize(c, nb_prev, n_iter - 1, 0, prior_slot(c, n_iter - 1), c->gamma_trace + (size_t)(n_iter - 1) * sg,
                       c->eta_trace + (size_t)(n_iter - 1) * 16));
        DSM_TRY(esum_reset(c));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_gibbs_update_sharded(dsm_ctx *c, int n_iter, int v_offset, int v_total, dsm_exchange_fn exchange, void *user)
{
    if (!exchange) { dsm_set_error("gibbs_update_sharded: no exchange callback"); return DSM_ERR_ARG; }
    return gibbs_update_sharded(c, n_iter, v_offset, v_total, exchange, user, nullptr);
}

// the same with the exchange done by the library over its own RCCL communicator (comm.hip): no host synchronisation per iteration
extern "C" int dsm_ctx_gibbs_update_sharded_comm(dsm_ctx *c, int n_iter, int v_offset, int v_total, dsm_comm *comm)
{
    if (!comm) { dsm_set_error("gibbs_update_sharded_comm: no communicator"); return DSM_ERR_ARG; }
    return gibbs_update_sharded(c, n_iter, v_offset, v_total, nullptr, nullptr, comm);
}

// raw device <-> host copies of the exchange buffers (for callers that reduce on the host, e.g. the two-shards-on-one-GPU test)
extern "C" int dsm_device_read(int device, const void *dev, void *host, size_t bytes)
{
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return DSM_OK;
}
extern "C" int dsm_device_write(int device, void *dev, const void *host, size_t bytes)
{
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
    return DSM_OK;
}

// one chain's inputs of an update_tau call: the stored (gamma, eta) pairs in, the entry state and the log-priors of every pair
static int tau_inputs(dsm_ctx *c, int n_iter, const double *gamma_store, const double *eta_store)
{
    const size_t sg = (size_t)c->S * c->G;
    if (n_iter > c->in_cap || !c->gamma_in) {            // grow-only, like the traces
        DSM_TRY(dev_alloc(&c->gamma_in, (size_t)n_iter * sg));
        DSM_TRY(dev_alloc(&c->eta_in, (size_t)n_iter * 16));
        DSM_TRY(dev_alloc(&c->prior_all, (size_t)n_iter * (c->S + 4)));
        c->in_cap = n_iter;
    }
    HIP_TRY(hipMemcpyAsync(c->gamma_in, gamma_store, (size_t)n_iter * sg * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->eta_in, eta_store, (size_t)n_iter * 16 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->gamma_trace, c->gamma_in, (size_t)n_iter * sg * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->eta_trace, c->eta_in, (size_t)n_iter * 16 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->nchange, 0, sizeof(int), c->stream));
    // entry: lp with (gamma_store[0], eta_store[0])  (HaploSNP_Sampler.py:386-389)
    DSM_TRY(eval_state(c, c->gamma_in, c->eta_in, c->tau_trace, 1));
    // the Dirichlet log-priors of all stored (gamma, eta) pairs in one launch instead of one per sweep
    DSM_TRY(k_prior_batch(c, c->gamma_in, c->eta_in, n_iter, c->prior_all));
    // sweep it writes parity it & 1 of (ll_partial, nchange); its finalize (ll / lp / MAP test / traces) rides as one
    // extra workgroup in the launch of sweep it + 1, which writes the other parity: one launch per sweep
    HIP_TRY(hipMemsetAsync(c->nchange, 0, 2 * sizeof(int), c->stream));
    return DSM_OK;
}

// updateTau (the -r path) of one chain or of K chains of one shape sharing the launch of every sweep.  gamma_stores[k] [n][S][G],
// eta_stores[k] [n][4][4]: chain k's traces.
static int update_tau(dsm_ctx *const *ctxs, int K, bool batched, int n_iter, const double *const *gamma_stores, const double *const *eta_stores)
{
    if (n_iter < 1 || !gamma_stores || !eta_stores) { dsm_set_error("update_tau: bad arguments"); return DSM_ERR_ARG; }
    Chains ch{ctxs, K, batched};
    DSM_TRY(ch.open(true, false, [&](const dsm_ctx *a, const dsm_ctx *b, int k) {
        if (!gamma_stores[k] || !eta_stores[k]) { dsm_set_error("update_tau: bad arguments"); return DSM_ERR_ARG; }
        return same_G_and_rng(a, b, k);
    }));
    const size_t sg = (size_t)ch.lead()->S * ch.lead()->G;
    std::vector<SweepWords> words;
    words.reserve(K);
    DSM_TRY(ch.each([&](dsm_ctx *c, int) -> int { DSM_TRY(alloc_traces(c, n_iter)); words.emplace_back(c, n_iter, c->u_cap); return DSM_OK; }));
    DSM_TRY(ch.launch([&](dsm_ctx *, int k) { return words[k].prefetch(); }));          // (generating while the inputs go in)
    DSM_TRY(ch.each([&](dsm_ctx *c, int k) { return tau_inputs(c, n_iter, gamma_stores[k], eta_stores[k]); }));
    std::vector<int> nb_prev(K, 0);
    std::vector<const uint32_t *> u(K, nullptr);
    for (int it = 0; it < n_iter; ++it) {
        DSM_TRY(ch.launch([&](dsm_ctx *, int k) { return words[k].acquire(it, &u[k]); }));
        DSM_TRY(ch.launch([&](dsm_ctx *c, int k) -> int {
            const uint32_t ic = c->iter_ctr++;
            const double *g = c->gamma_in + (size_t)it * sg, *e = c->eta_in + (size_t)it * 16;
            TauFinalRider rider;
            if (it > 0) {
                rider.nblocks = nb_prev[k]; rider.it = it - 1; rider.prior = c->prior_all + (size_t)(it - 1) * (c->S + 4);
                rider.gamma_src = c->gamma_in + (size_t)(it - 1) * sg; rider.eta_src = c->eta_in + (size_t)(it - 1) * 16;
            }
            return k_tau_sweep(c, 3, g, e, e, c->tau_trace + (size_t)(it + 1) * c->V, nullptr, ic, &nb_prev[k], u[k], it & 1,
                               it > 0 ? &rider : nullptr);                                              // :392-393
        }));
        DSM_TRY(ch.each([&](dsm_ctx *, int k) { return words[k].release(it); }));
    }
    DSM_TRY(ch.each([&](dsm_ctx *c, int k) {
        return k_finalize(c, nb_prev[k], n_iter - 1, 0, c->prior_all + (size_t)(n_iter - 1) * (c->S + 4),
                          c->gamma_in + (size_t)(n_iter - 1) * sg, c->eta_in + (size_t)(n_iter - 1) * 16, (n_iter - 1) & 1);
    }));
    HIP_TRY(hipStreamSynchronize(ch.lead()->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_update_tau(dsm_ctx *c, int n_iter, const double *gamma_store, const double *eta_store) { return update_tau(&c, 1, false, n_iter, &gamma_store, &eta_store); }

extern "C" int dsm_batch_update_tau(dsm_ctx *const *ctxs, int K, int n_iter, const double *const *gamma_stores, const double *const *eta_stores)
{
    return update_tau(ctxs, K, true, n_iter, gamma_stores, eta_stores);
}

// ---------------------------------------------------------------- the chain with tau held (HaploSNP_Sampler.py:409-428, update_fixed_tau)
// The distinct packed tau words of the resident state in ascending order, and the row of each position's word.  overflow: a pooled
// cell, or the four pooled cells of one (word, sample) together -- the depth dsm_ctx_set_counts bounds --, would pass INT32_MAX.
struct FixtauWords { std::vector<uint64_t> words; std::vector<int32_t> row; bool overflow = false; };

static int fixtau_words(dsm_ctx *c, FixtauWords *p)
{
    const int V = c->V, S = c->S;
    std::vector<uint64_t> t((size_t)V);
    HIP_TRY(hipMemcpyAsync(t.data(), c->tau, (size_t)V * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    p->words = t;
    std::sort(p->words.begin(), p->words.end());
    p->words.erase(std::unique(p->words.begin(), p->words.end()), p->words.end());
    p->row.resize((size_t)V);
    for (int v = 0; v < V; ++v) p->row[v] = (int32_t)(std::lower_bound(p->words.begin(), p->words.end(), t[v]) - p->words.begin());
    p->overflow = false;
    if (c->max_depth <= (uint64_t)INT32_MAX) return DSM_OK;        // a sample's reads over ALL positions fit: so does every pooled cell
    std::vector<int32_t> cnt((size_t)V * S * 4);
    HIP_TRY(hipMemcpyAsync(cnt.data(), c->cnt_vs, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int64_t> dep(p->words.size() * (size_t)S, 0);
    for (int v = 0; v < V && !p->overflow; ++v)
        for (int s = 0; s < S; ++s) {
            const int32_t *x = cnt.data() + ((size_t)v * S + s) * 4;
            int64_t &d = dep[(size_t)p->row[v] * S + s];
            d += (int64_t)x[0] + x[1] + x[2] + x[3];
            if (d > (int64_t)INT32_MAX) { p->overflow = true; break; }
        }
    return DSM_OK;
}

// pooled [W][S][4] on the device: zeroed, then fixtau_pool_kernel
static int fixtau_pool_counts(dsm_ctx *c, const FixtauWords &p, DevBuf<int32_t> &d_pooled)
{
    const size_t np = p.words.size() * (size_t)c->S * 4;
    DevBuf<int32_t> d_row;
    DSM_TRY(d_row.alloc((size_t)c->V));
    DSM_TRY(d_pooled.alloc(np));
    HIP_TRY(hipMemcpyAsync(d_row, p.row.data(), (size_t)c->V * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_pooled, 0, np * sizeof(int32_t), c->stream));
    DSM_TRY(k_fixtau_pool(c, d_row, d_pooled));
    HIP_TRY(hipStreamSynchronize(c->stream));                   // (d_row is released on return)
    return DSM_OK;
}

// The scratch chain of the pooled form: a context of W positions -- the pooled counts, the W words -- with the caller's gamma, eta, priors,
// stream key, iteration counter and mu/E choice.  It is loaded through dsm_ctx_set_counts / dsm_ctx_set_state, so it IS the chain a caller
// would set up on the pooled table (the test contract), its data constant included.
static int fixtau_enter(dsm_ctx *c, const FixtauWords &p, dsm_ctx **child_out)
{
    const int W = (int)p.words.size(), S = c->S, G = c->G;
    DevBuf<int32_t> d_pooled;
    DSM_TRY(fixtau_pool_counts(c, p, d_pooled));
    const size_t np = (size_t)W * S * 4;
    std::vector<int32_t> h32(np);
    std::vector<double> gamma((size_t)S * G), eta(16);
    HIP_TRY(hipMemcpyAsync(h32.data(), d_pooled, np * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(gamma.data(), c->gamma, gamma.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(eta.data(), c->eta, 16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int64_t> h64(h32.begin(), h32.end());
    std::vector<int64_t> onehot((size_t)W * G * 4, 0);
    for (int w = 0; w < W; ++w)
        for (int g = 0; g < G; ++g) onehot[((size_t)w * G + g) * 4 + ((p.words[w] >> (2 * g)) & 3)] = 1;
    if (!c->fixtau_child) DSM_TRY(dsm_ctx_create(&c->fixtau_child, c->device));
    dsm_ctx *k = c->fixtau_child;
    DSM_TRY(dsm_ctx_set_counts(k, h64.data(), W, S));
    DSM_TRY(dsm_ctx_set_priors(k, c->alpha, c->delta, c->epsilon));
    DSM_TRY(dsm_ctx_set_state(k, onehot.data(), gamma.data(), eta.data(), G));
    k->ctr_seed = c->ctr_seed; k->iter_ctr = c->iter_ctr;
    k->force_stats_spec = c->force_stats_spec; k->tau_neartie_mode = c->tau_neartie_mode; k->tau_screen = c->tau_screen;
    *child_out = k;
    return DSM_OK;
}

extern "C" int dsm_ctx_gibbs_update_fixed_tau(dsm_ctx *c, int n_iter, int fix_eta, int pool)
{
    if (n_iter < 0) { dsm_set_error("n_iter < 0"); return DSM_ERR_ARG; }
    if (pool < -1 || pool > 1) { dsm_set_error("gibbs_update_fixed_tau: pool -1 (auto), 0 or 1"); return DSM_ERR_ARG; }
    DSM_TRY(dsm_ctx_need(c, true, true));
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream_rng));
    bool pooled = false;
    FixtauWords p;
    if (pool != 0) {
        DSM_TRY(fixtau_words(c, &p));
        if (p.overflow && pool == 1) { dsm_set_error("gibbs_update_fixed_tau: a pooled count would pass 2^31-1 (run with pool = 0 or -1)"); return DSM_ERR_UNSUPPORTED; }
        // auto: pooling is one pass over the table, less than one iteration's mu/E pass, so any reduction counts as worth it (not measured where it stops paying: DESIGN.md sec. 8c)
        pooled = !p.overflow && (pool == 1 || (int)p.words.size() < c->V);
    }
    if (!pooled) return gibbs_update(&c, 1, false, n_iter, TauStep{c->G, fix_eta != 0});
    dsm_ctx *k = nullptr;
    DSM_TRY(fixtau_enter(c, p, &k));
    DSM_TRY(gibbs_update(&k, 1, false, n_iter, TauStep{k->G, fix_eta != 0}));      // (returns with the child's stream drained)
    // back to the caller: gamma, eta, traces, MAP record, iteration counter; its counts and tau were only read
    const size_t sg = (size_t)c->S * c->G, n = (size_t)n_iter;
    DSM_TRY(alloc_traces(c, n_iter));
    c->tau_fixed_trace = true;
    auto d2d = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream) : hipSuccess; };
    HIP_TRY(d2d(c->tau_trace, c->tau, (size_t)c->V * sizeof(uint64_t)));
    HIP_TRY(d2d(c->gamma, k->gamma, sg * sizeof(double)));
    HIP_TRY(d2d(c->eta, k->eta, 16 * sizeof(double)));
    HIP_TRY(d2d(c->gamma_trace, k->gamma_trace, n * sg * sizeof(double)));
    HIP_TRY(d2d(c->eta_trace, k->eta_trace, n * 16 * sizeof(double)));
    HIP_TRY(d2d(c->ll_trace, k->ll_trace, n * sizeof(double)));
    HIP_TRY(d2d(c->lp_trace, k->lp_trace, n * sizeof(double)));
    HIP_TRY(d2d(c->nchange_trace, k->nchange_trace, n * sizeof(int)));
    HIP_TRY(d2d(c->star, k->star, 2 * sizeof(double)));
    HIP_TRY(d2d(c->gamma_star, k->gamma_star, sg * sizeof(double)));
    HIP_TRY(d2d(c->eta_star, k->eta_star, 16 * sizeof(double)));
    HIP_TRY(d2d(c->scalars, k->scalars, 2 * sizeof(double)));
    // the multinomial coefficients of the caller's table minus the pooled table's: every reported ll / lp is the caller's table's
    DSM_TRY(k_fixtau_add_const(c, n_iter, c->ll_const - k->ll_const));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->iter_ctr = k->iter_ctr;
    c->tau_rare_n = k->tau_rare_n;
    return DSM_OK;
}

// ---------------------------------------------------------------- the chain with the LAST n_held haplotypes held
extern "C" int dsm_ctx_gibbs_update_held_tau(dsm_ctx *c, int n_iter, int n_held, int fix_eta)
{
    if (n_iter < 0) { dsm_set_error("n_iter < 0"); return DSM_ERR_ARG; }
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (n_held < 0 || n_held > c->G) { dsm_set_error("gibbs_update_held_tau: n_held = %d outside 0..%d", n_held, c->G); return DSM_ERR_ARG; }
    if (n_held == 0) return dsm_ctx_gibbs_update(c, n_iter);
    if (n_held == c->G) return dsm_ctx_gibbs_update_fixed_tau(c, n_iter, fix_eta, 0);
    BIND(c);
    if (c->tau_rng == DSM_RNG_MT19937 && n_iter > 0 && !c->mt_seeded) { dsm_set_error("tau RNG not seeded: call dsm_ctx_seed / dsm_setRNG"); return DSM_ERR_STATE; }
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream_rng));
    return gibbs_update(&c, 1, false, n_iter, TauStep{n_held, fix_eta != 0});
}

// test hook: the pooled table the call above would run on for the resident state -- *W words, pooled [W][S][4] (room for [V][S][4]),
// words [W] ascending (room for V), row [V].  Any pointer may be null.
extern "C" int dsm_ctx_debug_fixtau_pool(dsm_ctx *c, int *W, int32_t *pooled, uint64_t *words, int32_t *row)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    FixtauWords p;
    DSM_TRY(fixtau_words(c, &p));
    if (p.overflow) { dsm_set_error("debug_fixtau_pool: a pooled count would pass 2^31-1"); return DSM_ERR_UNSUPPORTED; }
    if (W) *W = (int)p.words.size();
    if (words) memcpy(words, p.words.data(), p.words.size() * sizeof(uint64_t));
    if (row) memcpy(row, p.row.data(), p.row.size() * sizeof(int32_t));
    if (pooled) {
        DevBuf<int32_t> d;
        DSM_TRY(fixtau_pool_counts(c, p, d));
        HIP_TRY(hipMemcpy(pooled, d, p.words.size() * (size_t)c->S * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return DSM_OK;
}

// test hook: dsm_ctx_sample_stats on the pooled state of the resident one (the caller's state and counters are untouched)
extern "C" int dsm_ctx_debug_fixtau_sample_stats(dsm_ctx *c, uint32_t iter, uint64_t *sum_mu, uint64_t *esum)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    FixtauWords p;
    DSM_TRY(fixtau_words(c, &p));
    if (p.overflow) { dsm_set_error("debug_fixtau_sample_stats: a pooled count would pass 2^31-1"); return DSM_ERR_UNSUPPORTED; }
    dsm_ctx *k = nullptr;
    DSM_TRY(fixtau_enter(c, p, &k));
    return dsm_ctx_sample_stats(k, iter, sum_mu, esum);
}

extern "C" int dsm_release_device_caches(void)
{
    // what the library keeps per process and device beyond the life of a context: the MT19937 jump tables (2 x 50 MB per device, built by the
    // first long fill).  No context may be running a fill while this is called.
    mt_jump_release();
    return DSM_OK;
}

extern "C" int dsm_ctx_debug_log2f(dsm_ctx *c, const float *in, float *out, size_t n)
{
    if (!c || !in || !out) { dsm_set_error("debug_log2f: bad arguments"); return DSM_ERR_ARG; }
    if (n == 0) return DSM_OK;
    BIND(c);
    DevBuf<float> d_in, d_out;
    DSM_TRY(d_in.alloc(n)); DSM_TRY(d_out.alloc(n));
    HIP_TRY(hipMemcpyAsync(d_in, in, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    DSM_TRY(k_log2f_test(c, d_in, d_out, n));
    HIP_TRY(hipMemcpyAsync(out, d_out, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// workgroups of one tau sweep: launched, and resident at once on this device (occupancy x compute units)
extern "C" int dsm_ctx_tau_launch_info(dsm_ctx *c, int *launched, int *resident)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (!launched || !resident) { dsm_set_error("tau_launch_info: null argument"); return DSM_ERR_ARG; }
    BIND(c);
    return tau_launch_info(c, launched, resident);
}

// 0: dsm_nmft_factorize never takes the persistent one-launch path; 1 / -1: wherever the table fits (the default)
extern "C" int dsm_ctx_set_nmft_persist(dsm_ctx *c, int mode)
{
    if (!c || mode < -1 || mode > 1) { dsm_set_error("set_nmft_persist: mode -1, 0 or 1"); return DSM_ERR_ARG; }
    c->nmft_persist = mode;
    return DSM_OK;
}

// Which form of the reduce + gamma/control step of an NMFT update runs (kernels_nmft.hip: k_nmft_gamma): -1 = by the number of
// workgroup partials (the default), 0 = reduction and control as two launches, 1 = the fused launch.  Same factors bit for bit.
extern "C" int dsm_ctx_set_nmft_fused(dsm_ctx *c, int mode)
{
    if (!c || mode < -1 || mode > 3 || mode == 2) { dsm_set_error("set_nmft_fused: mode -1, 0, 1 or 3"); return DSM_ERR_ARG; }
    c->nmft_fused = mode;
    return DSM_OK;
}

// A/B switch for tests and measurements: with on = 0 every sweep step is evaluated in fp64 (the same draws except in near-ties:
// the two modes evaluate the current base's log-probability along different FMA chains, a flip needs u within ~1e-13 of a CDF edge)
extern "C" int dsm_ctx_set_tau_neartie(dsm_ctx *c, int mode)
{
    if (!c || mode < -1 || mode > 1) { dsm_set_error("set_tau_neartie: -1 (by the abundances), 0 or 1"); return DSM_ERR_ARG; }
    c->tau_neartie_mode = mode;
    return DSM_OK;
}

// Whether a Gibbs iteration launches stats_big_kernel between stage 1 and the Dirichlet launch, where that is a choice (kernels_stats.hip:
// stats_big_optional): -1 = while stage 1 was last seen handing items over, 0 = never (the Dirichlet launch draws them), 1 = always.
// Same draws bit for bit.
extern "C" int dsm_ctx_set_big_launch(dsm_ctx *c, int mode)
{
    if (!c || mode < -1 || mode > 1) { dsm_set_error("set_big_launch: -1 (while the deferred lists are in use), 0 or 1"); return DSM_ERR_ARG; }
    c->big_launch_mode = mode;
    return DSM_OK;
}

// test hook: how many of the deferred lists' counters are non-zero now (0 between passes), and the running count of lists found non-empty
extern "C" int dsm_ctx_debug_big_lists(dsm_ctx *c, int *nonzero, uint32_t *seen)
{
    if (!c) { dsm_set_error("debug_big_lists: null context"); return DSM_ERR_ARG; }
    if (nonzero) *nonzero = 0;
    if (seen) *seen = 0;
    if (!c->big_count) return DSM_OK;
    BIND(c);
    std::vector<uint32_t> w(DSM_BIG_NT * DSM_BIG_NL * DSM_BIG_STRIDE);
    HIP_TRY(hipMemcpyAsync(w.data(), c->big_count, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int nz = 0;
    for (int i = 0; i < DSM_BIG_NT * DSM_BIG_NL; ++i) nz += w[(size_t)i * DSM_BIG_STRIDE] != 0u;
    nz += w[DSM_BIG_W_ARRIVE] != 0u;                      // (the arrival word and the tickets are zero between launches too)
    for (int i = 0; i < DSM_BIG_NT * DSM_BIG_NL; ++i) nz += w[(size_t)i * DSM_BIG_STRIDE + DSM_BIG_W_TICKET] != 0u;
    if (nonzero) *nonzero = nz;
    if (seen) *seen = w[DSM_BIG_W_SEEN];
    return DSM_OK;
}

extern "C" int dsm_ctx_set_tau_screen(dsm_ctx *c, int on)
{
    if (!c) { dsm_set_error("set_tau_screen: null context"); return DSM_ERR_ARG; }
    c->tau_screen = on != 0;
    return DSM_OK;
}

// Evidence for the screening pass of the tau sweep: wavefront-steps run, and wavefront-steps the fp32 screen did not decide
// (evaluated in fp64), summed by every finalize step over the sweeps of the full iterations and of updateTau.  mode 1 = read
// and zero, 0 = read.
extern "C" int dsm_ctx_sweep_stats(dsm_ctx *c, uint64_t *steps, uint64_t *exact_steps, int mode)
{
    if (!c || mode < 0 || mode > 1) { dsm_set_error("sweep_stats: bad arguments"); return DSM_ERR_ARG; }
    BIND(c);
    unsigned long long h[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h, c->sweep_stats, sizeof h, hipMemcpyDeviceToHost, c->stream));
    if (mode == 1) HIP_TRY(hipMemsetAsync(c->sweep_stats, 0, sizeof h, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (steps) *steps = h[0];
    if (exact_steps) *exact_steps = h[1];
    return DSM_OK;
}

extern "C" int dsm_ctx_get_trace(dsm_ctx *c, double *ll, double *lp, int32_t *nchange, double *gamma_store, double *eta_store)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    BIND(c);
    const size_t n = (size_t)c->n_trace, sg = (size_t)c->S * c->G;
    if (n == 0) return DSM_OK;
    if (ll) HIP_TRY(hipMemcpyAsync(ll, c->ll_trace, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (lp) HIP_TRY(hipMemcpyAsync(lp, c->lp_trace, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (nchange) HIP_TRY(hipMemcpyAsync(nchange, c->nchange_trace, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (gamma_store) HIP_TRY(hipMemcpyAsync(gamma_store, c->gamma_trace, n * sg * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (eta_store) HIP_TRY(hipMemcpyAsync(eta_store, c->eta_trace, n * 16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_get_star(dsm_ctx *c, int64_t *tau_star, double *gamma_star, double *eta_star, double *lp_star, int *iter_star)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (!c->tau_trace) { dsm_set_error("get_star: no update has run"); return DSM_ERR_STATE; }
    BIND(c);
    double st[2];
    HIP_TRY(hipMemcpyAsync(st, c->star, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int slot = (int)st[1];
    if (tau_star) DSM_TRY(fetch_tau(c, trace_tau_slot(c, slot), tau_star));
    if (gamma_star) HIP_TRY(hipMemcpyAsync(gamma_star, c->gamma_star, (size_t)c->S * c->G * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (eta_star) HIP_TRY(hipMemcpyAsync(eta_star, c->eta_star, 16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (lp_star) *lp_star = st[0];
    if (iter_star) *iter_star = slot > 0 ? slot - 1 : 0;      // storeStarState(iter), entry state = 0
    return DSM_OK;
}

extern "C" int dsm_ctx_get_tau_sum(dsm_ctx *c, int64_t *tau_sum)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (!c->tau_trace || !tau_sum) { dsm_set_error("get_tau_sum: no update has run"); return DSM_ERR_STATE; }
    BIND(c);
    const size_t nt = (size_t)c->V * c->G * 4;
    if (c->tau_fixed_trace) {                 // every stored iteration holds the tau of slot 0
        DSM_TRY(fetch_tau(c, c->tau_trace, tau_sum));
        for (size_t i = 0; i < nt; ++i) tau_sum[i] *= c->n_trace;
        return DSM_OK;
    }
    DevBuf<int64_t> d;
    DSM_TRY(d.alloc(nt));
    DSM_TRY(k_tau_sum(c, c->tau_trace, c->n_trace, d));
    HIP_TRY(hipMemcpyAsync(tau_sum, d, nt * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_ctx_get_tau_at(dsm_ctx *c, int it, int64_t *tau)
{
    DSM_TRY(dsm_ctx_need(c, true, true));
    if (!c->tau_trace || !tau || it < -1 || it >= c->n_trace) { dsm_set_error("get_tau_at: bad iteration"); return DSM_ERR_ARG; }
    BIND(c);
    return fetch_tau(c, trace_tau_slot(c, it + 1), tau);
}

// ---------------------------------------------------------------- NMFT
extern "C" int dsm_nmft_set(dsm_ctx *c, const double *tau, const double *gamma, int G)
{
    DSM_TRY(dsm_ctx_need(c, true, false));
    if (!tau || !gamma || G < 1 || G > DSM_MAX_G) { dsm_set_error("nmft_set: bad arguments"); return DSM_ERR_ARG; }
    BIND(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int V = c->V, S = c->S;
    if (!c->F) { DSM_TRY(dev_alloc(&c->F, (size_t)V * 4 * S)); DSM_TRY(k_nmft_freq(c)); }
    c->nG = G;
    c->nmft_blocks = nmft_grid(c);
    DSM_TRY(dev_alloc(&c->ntau, (size_t)V * 4 * G));
    dev_free(&c->ntau2);                                  // sized by the previous G: factorize_tau's fused pass makes it again on first use
    DSM_TRY(dev_alloc(&c->ngam, (size_t)G * S));
    DSM_TRY(dev_alloc(&c->ngam_raw, (size_t)G * S));
    DSM_TRY(dev_alloc(&c->ngam2, (size_t)G * S));            // the other parity's buffers of the update kernel's own gamma step
    DSM_TRY(dev_alloc(&c->ngam_raw2, (size_t)G * S));
    DSM_TRY(dev_alloc(&c->npart, (size_t)std::max(c->nmft_blocks, std::max(nmft_wide_grid(c), nmft_use_mfma(c) ? std::max(nmft_mfma_grid(c, false), nmft_mfma_grid(c, true)) : 0)) * ((size_t)G * S + G + 1)));
    DSM_TRY(dev_alloc(&c->nstat, (size_t)G * S + 2 * G + 16));
    // reference layout tau[v + a*V][g] -> device layout [v][a][g]
    std::vector<double> t((size_t)V * 4 * G);
    for (int a = 0; a < 4; ++a)
        for (int v = 0; v < V; ++v)
            memcpy(&t[((size_t)v * 4 + a) * G], &tau[((size_t)a * V + v) * G], sizeof(double) * G);
    HIP_TRY(hipMemcpyAsync(c->ntau, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ngam, gamma, (size_t)G * S * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ngam_raw, gamma, (size_t)G * S * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_nmft_get(dsm_ctx *c, double *tau, double *gamma)
{
    DSM_TRY(dsm_ctx_need(c, true, false));
    if (!c->ntau) { dsm_set_error("nmft_get: call dsm_nmft_set first"); return DSM_ERR_STATE; }
    BIND(c);
    const int V = c->V, S = c->S, G = c->nG;
    if (tau) {
        std::vector<double> t((size_t)V * 4 * G);
        HIP_TRY(hipMemcpyAsync(t.data(), c->ntau, t.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int a = 0; a < 4; ++a)
            for (int v = 0; v < V; ++v)
                memcpy(&tau[((size_t)a * V + v) * G], &t[((size_t)v * 4 + a) * G], sizeof(double) * G);
    }
    if (gamma) HIP_TRY(hipMemcpyAsync(gamma, c->ngam, (size_t)G * S * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// nstat control words (after the G*S + 2G reduced statistics):
//   [0] div of the current state  [1] previous div  [2] done flag  [3] updates run  [4] it at stop
//   [10] the fused pass of factorize_tau left the current rows in ntau2  [11] the update kernel's own gamma step left gamma in ngam2
static double *nmft_ctl(dsm_ctx *c) { return c->nstat + (size_t)c->nG * c->S + 2 * c->nG; }

// One chain's part of a factorize call (dsm_nmft_factorize, dsm_batch_nmft_factorize): its start, its control words as last read back,
// its end.  The destructor takes over which buffer of each pair the update loop left current -- pointer swaps, no copies -- and clears
// what the update kernels read only during the call, on every return path.
struct NmftRun {
    dsm_ctx *c = nullptr;
    DevBuf<double> trace;                  // objective after every update
    double h[12] = {};
    bool fusedfix = false;                  // gamma fixed on the matrix-core kernel: ntau / ntau2 alternate
    bool swap_tau = false, swap_gam = false;    // set by the update loops that alternate a pair (the persistent launch keeps its own)
    ~NmftRun()
    {
        if (!c) return;
        if (swap_tau && h[10] != 0.0) std::swap(c->ntau, c->ntau2);
        if (swap_gam && h[11] != 0.0) { std::swap(c->ngam, c->ngam2); std::swap(c->ngam_raw, c->ngam_raw2); }
        c->ndiv_trace = nullptr; c->nmft_fix_gamma = 0;
    }
    int begin(dsm_ctx *ctx, int max_iter, int fix_gamma)
    {
        c = ctx;
        DSM_TRY(trace.alloc((size_t)max_iter + 1));
        HIP_TRY(hipMemsetAsync(nmft_ctl(c), 0, 16 * sizeof(double), c->stream));
        c->ndiv_trace = trace;
        // gamma fixed: the update kernels leave out what only a gamma update reads (kernels_nmft.hip), and on the matrix-core kernel an
        // update is ONE fused pass (objective of the current rows + candidate rows of the next update into the second buffer, accepted or
        // not by the control step that follows: NmftMfmaParams.fix_gamma == 2)
        fusedfix = fix_gamma && nmft_use_mfma(c);
        c->nmft_fix_gamma = fusedfix ? 2 : fix_gamma ? 1 : 0;
        if (fusedfix && !c->ntau2) DSM_TRY(dev_alloc(&c->ntau2, (size_t)c->V * 4 * c->nG));
        // factorize applies _adjustment once before the first objective (Init_NMFT.py:102)
        if (!fix_gamma) DSM_TRY(k_nmft_clamp(c));
        return DSM_OK;
    }
    int read_ctl() { HIP_TRY(hipMemcpyAsync(h, nmft_ctl(c), sizeof h, hipMemcpyDeviceToHost, c->stream)); return DSM_OK; }
    // updates run and the objective trace, from the control words read back after the last launch (the copy is enqueued)
    int finish(int *n_done, double *div_trace)
    {
        const int done = (int)h[3];
        if (n_done) *n_done = done;
        if (div_trace) HIP_TRY(hipMemcpyAsync(div_trace, trace, ((size_t)done + 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        return DSM_OK;
    }
};

extern "C" int dsm_nmft_factorize(dsm_ctx *c, int max_iter, double min_change, int fix_gamma, int *n_done, double *div_trace)
{
    DSM_TRY(dsm_ctx_need(c, true, false));
    if (!c->ntau) { dsm_set_error("nmft_factorize: call dsm_nmft_set first"); return DSM_ERR_STATE; }
    if (max_iter < 0) { dsm_set_error("max_iter < 0"); return DSM_ERR_ARG; }
    BIND(c);
    NmftRun run;
    DSM_TRY(run.begin(c, max_iter, fix_gamma));
    const int adjust = fix_gamma ? 0 : 1;
    const bool fusedfix = run.fusedfix;
    const int BATCH = 64;
    {
        // tables whose quads of variants are all resident at once: the whole loop as ONE persistent launch (kernels_nmft.hip)
        int used = 0;
        DSM_TRY(k_nmft_persist(c, max_iter, min_change, fix_gamma, adjust, &used));
        if (used) {
            DSM_TRY(run.read_ctl());
            HIP_TRY(hipStreamSynchronize(c->stream));
            DSM_TRY(run.finish(n_done, div_trace));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return DSM_OK;
        }
    }
    const bool wave = nmft_use_wave(c);
    // one-pass path: statistics of the initial state, then every update launch also produces the
    // statistics of the next iteration; two-pass path (large S*G): pass A + pass B per iteration
    if (wave && !fusedfix) DSM_TRY(k_nmft_wave(c, adjust, 0));
    // One iteration = the same 2-3 launches every time (the iteration index and the stop flag live in
    // device memory), so BATCH iterations can be captured once into a hipGraph and replayed.  Measured on
    // MI355X / ROCm 7.2: a replayed kernel node costs ~10 us, more than a stream-ordered launch (V=10k: 70 vs
    // 40 us per iteration; V=1k: 48 vs 25), so a single chain runs eagerly.  Replay pays when several chains
    // share the GPU from different host threads -- the `-r 1000` sweeps every shipped workflow runs -- because
    // it takes the host (and the runtime's launch lock) out of the loop: 35-chain sweep at V=1000, 4 chains at a
    // time: 4.2 s eager -> 2.2 s replayed.  desman_amd.chains opts in through DESMAN_HIP_NMFT_GRAPH=1.
    // (Timing mode records events per launch -> eager.)
    const bool gstep = wave && !fusedfix && nmft_gstep_applies(c, fix_gamma);
    run.swap_tau = fusedfix;                 // an odd number of accepted candidates: the current rows are in ntau2
    run.swap_gam = gstep;                    // an odd number of gamma steps: the current gamma is in ngam2
    auto enqueue_iteration = [&](int n) -> int {                                     // n = launch number of this call (parity slot)
        if (fusedfix) {                                                              // the pass first: its objective is what the control step tests
            DSM_TRY(k_nmft_wave(c, adjust, 1));
            return k_nmft_gamma(c, max_iter, min_change, fix_gamma, adjust, n & 1);
        }
        if (!wave) DSM_TRY(k_nmft_pass_a(c));
        if (gstep) {
            // large tables on the matrix-core kernel (round 6): the reduction, then the update kernel, which begins with the gamma / control
            // step itself (NmftMfmaParams.gstep) -- two launches per update instead of three
            DSM_TRY(k_nmft_reduce(c));
            c->nmft_gstep = 1; c->nmft_gstep_parity = n & 1; c->nmft_gstep_max_iter = max_iter; c->nmft_gstep_min_change = min_change;
            const int rc = k_nmft_wave(c, adjust, 1);
            c->nmft_gstep = 0;
            return rc;
        }
        // the control kernel decides ON THE DEVICE whether this update runs at all (Init_NMFT.py:106)
        DSM_TRY(k_nmft_gamma(c, max_iter, min_change, fix_gamma, adjust, n & 1));       // also records div_trace[it]
        DSM_TRY(wave ? k_nmft_wave(c, adjust, 1) : k_nmft_pass_b(c, adjust));           // exits at once when stopped
        return DSM_OK;
    };
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    struct GraphGuard { hipGraph_t &g; hipGraphExec_t &e; ~GraphGuard() { if (e) (void)hipGraphExecDestroy(e); if (g) (void)hipGraphDestroy(g); } } gg{graph, gexec};
    const char *genv = getenv("DESMAN_HIP_NMFT_GRAPH");
    const bool use_graph = genv && genv[0] == '1' && !c->timing && max_iter >= BATCH && (size_t)c->V * c->S <= 131072;
    if (use_graph) {
        HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        int rc = DSM_OK;
        for (int k = 0; k < BATCH && rc == DSM_OK; ++k) rc = enqueue_iteration(k);      // BATCH is even: node k keeps its parity in every replay
        hipError_t e = hipStreamEndCapture(c->stream, &graph);
        if (rc != DSM_OK) return rc;
        HIP_TRY(e);
        HIP_TRY(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
    }
    // iterations 0..max_iter inclusive evaluate the objective; the last one can only stop
    for (int launched = 0; launched <= max_iter;) {
        if (use_graph) { HIP_TRY(hipGraphLaunch(gexec, c->stream)); launched += BATCH; }
        else { for (int k = 0; k < BATCH && launched <= max_iter; ++k, ++launched) DSM_TRY(enqueue_iteration(launched)); }
        DSM_TRY(run.read_ctl());
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (run.h[2] != 0.0) break;
    }
    DSM_TRY(run.finish(n_done, div_trace));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

// Init_NMFT.factorize / factorize_tau of K chains of one shape at once: every update is one launch of each of its three
// kernels for all of them (chain = blockIdx.y).  The stop test is per chain, on the device; a chain that has stopped costs
// nothing but its workgroups' first instruction.  Matrix-core path only (S <= 128, G <= 16).  n_done [K];
// div_traces [K][max_iter + 1] or null.
extern "C" int dsm_batch_nmft_factorize(dsm_ctx *const *ctxs, int K, int max_iter, double min_change, int fix_gamma,
                                        int *n_done, double *div_traces)
{
    if (max_iter < 0) { dsm_set_error("max_iter < 0"); return DSM_ERR_ARG; }
    // (Round 6, VERDICT r5 item 6 -- measured, not kept: every chain of a batch of small tables running its own persistent launch from a host
    // thread of its own, as many at once as the persistent path's gate admits (four of V = 1000, S = 64).  4.4 us per chain-update at 8 x
    // (1000, 64, 5) and 8 x COG0015 against 2.9-3.0 for the batched three-launch loop below, which shares every launch among the K chains:
    // profiles/r06_batch_nmft.txt.  The batched loop already is what the item asked a batch-persistent kernel for.)
    NmftRun run[DSM_MAX_BATCH];             // (before the chains: their destructor drains the stream before the traces are freed)
    Chains ch{ctxs, K, true};
    DSM_TRY(ch.open(false, true, [](const dsm_ctx *a, const dsm_ctx *b, int k) {
        if (!b->ntau) { dsm_set_error("nmft_factorize: call dsm_nmft_set first (chain %d)", k); return DSM_ERR_STATE; }
        if (b->nG != a->nG) { dsm_set_error("batch: chain %d differs from chain 0 in device or shape", k); return DSM_ERR_ARG; }
        if (!nmft_use_mfma(b) && !nmft_use_wide(b)) { dsm_set_error("batch: the matrix-core NMFT kernels do not apply to this shape (S <= 512, G <= 16)"); return DSM_ERR_UNSUPPORTED; }
        return DSM_OK;
    }));
    const int adjust = fix_gamma ? 0 : 1;
    DSM_TRY(ch.each([&](dsm_ctx *c, int k) { return run[k].begin(c, max_iter, fix_gamma); }));
    // gamma fixed: the fused pass where the shape has one (S <= 128), else the two-half form of nmft_split_kernel without gamma numerators
    const bool fused = run[0].fusedfix;
    for (int k = 0; k < K; ++k) run[k].swap_tau = fused;
    if (!fused) DSM_TRY(ch.launch([&](dsm_ctx *c, int) { return k_nmft_wave(c, adjust, 0); }));
    const int BATCH = 64;
    for (int launched = 0; launched <= max_iter;) {
        for (int i = 0; i < BATCH && launched <= max_iter; ++i, ++launched) {
            if (fused) DSM_TRY(ch.launch([&](dsm_ctx *c, int) { return k_nmft_wave(c, adjust, 1); }));     // the fused pass first: its objective is what the control step tests
            DSM_TRY(ch.launch([&](dsm_ctx *c, int) { return k_nmft_gamma(c, max_iter, min_change, fix_gamma, adjust, launched & 1); }));
            if (!fused) DSM_TRY(ch.launch([&](dsm_ctx *c, int) { return k_nmft_wave(c, adjust, 1); }));
        }
        DSM_TRY(ch.each([&](dsm_ctx *, int k) { return run[k].read_ctl(); }));
        HIP_TRY(hipStreamSynchronize(ch.lead()->stream));
        bool all = true;
        for (int k = 0; k < K; ++k) all = all && run[k].h[2] != 0.0;
        if (all) break;
    }
    DSM_TRY(ch.each([&](dsm_ctx *, int k) {
        return run[k].finish(n_done ? n_done + k : nullptr, div_traces ? div_traces + (size_t)k * ((size_t)max_iter + 1) : nullptr);
    }));
    HIP_TRY(hipStreamSynchronize(ch.lead()->stream));
    return DSM_OK;
}

// test hook (read only): the kernel family and instantiation dsm_nmft_factorize takes for this context as it is set up now
extern "C" int dsm_nmft_debug_path(dsm_ctx *c, int fix_gamma, int *out)
{
    DSM_TRY(dsm_ctx_need(c, true, false));
    if (!out) { dsm_set_error("nmft_debug_path: out is null"); return DSM_ERR_ARG; }
    if (!c->ntau) { dsm_set_error("nmft_debug_path: call dsm_nmft_set first"); return DSM_ERR_STATE; }
    BIND(c);
    return nmft_debug_path(c, fix_gamma, out);
}

extern "C" int dsm_nmft_objective(dsm_ctx *c, double *div)
{
    DSM_TRY(dsm_ctx_need(c, true, false));
    if (!c->ntau || !div) { dsm_set_error("nmft_objective: call dsm_nmft_set first"); return DSM_ERR_STATE; }
    BIND(c);
    HIP_TRY(hipMemsetAsync(nmft_ctl(c), 0, 16 * sizeof(double), c->stream));
    DSM_TRY(nmft_use_wave(c) ? k_nmft_wave(c, 0, 0) : k_nmft_pass_a(c));
    DSM_TRY(k_nmft_gamma(c, 0, 0.0, 1, 0, 0));     // max_iter = 0: reduce + record div only
    HIP_TRY(hipMemcpyAsync(div, nmft_ctl(c), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_nmft_get_tau(dsm_ctx *c, int64_t *tau_onehot)
{
    DSM_TRY(dsm_ctx_need(c, true, false));
    if (!c->ntau || !tau_onehot) { dsm_set_error("nmft_get_tau: call dsm_nmft_set first"); return DSM_ERR_STATE; }
    BIND(c);
    DevBuf<uint64_t> d_p;
    DSM_TRY(d_p.alloc((size_t)c->V));
    DSM_TRY(k_nmft_get_tau(c, d_p));
    const int Gs = c->G;
    c->G = c->nG;
    int r = fetch_tau(c, d_p, tau_onehot);
    c->G = Gs;
    return r;
}

// ---------------------------------------------------------------- legacy shim
// One process-global context + MT19937 stream, like `static gsl_rng *ptGSLRNG`
// (sampletau/c_sample_tau.c:24).  Not re-entrant (neither is the reference).
static dsm_ctx *g_legacy = nullptr;
static bool g_legacy_rng = false;
static std::mutex g_legacy_mu;
// the tensor resident in the shim's context: a module-swap user passes the same `variants` on every call
// (HaploSNP_Sampler.py:345), and re-uploading 20 MB costs more than the sweep.  The shim may skip the upload only if
// the tensor is provably the same: pointer, shape and a 64-bit hash of EVERY word (multi-threaded, ~0.3 ms for
// 20 MB) must match -- the pointers are borrowed, the caller may have rewritten the array in place.
static const int64_t *g_legacy_ptr = nullptr;
static int g_legacy_V = 0, g_legacy_S = 0;
static uint64_t g_legacy_hash = 0;

static uint64_t hash_words(const int64_t *p, size_t n)
{
    const unsigned nthr = (unsigned)std::max<size_t>(1, std::min<size_t>(8, n / 65536));
    std::vector<uint64_t> part(nthr, 0);
    auto work = [&](unsigned t) {
        const size_t lo = n * t / nthr, hi = n * (t + 1) / nthr;
        uint64_t h[4] = {0x243F6A8885A308D3ull, 0x13198A2E03707344ull, 0xA4093822299F31D0ull, 0x082EFA98EC4E6C89ull};
        size_t i = lo;
        for (; i + 4 <= hi; i += 4)
            for (int k = 0; k < 4; ++k) h[k] = (h[k] ^ (uint64_t)p[i + k]) * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
        for (; i < hi; ++i) h[0] = (h[0] ^ (uint64_t)p[i]) * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
        uint64_t r = 0;
        for (int k = 0; k < 4; ++k) r = (r ^ h[k]) * 0xD6E8FEB86659FD93ull + (r >> 29);
        part[t] = r;
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nthr; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    uint64_t r = n;
    for (unsigned t = 0; t < nthr; ++t) r = (r ^ part[t]) * 0xD6E8FEB86659FD93ull + (r >> 31);
    return r;
}

static int legacy_ctx()
{
    if (g_legacy) return DSM_OK;
    int dev = 0;
    const char *e = getenv("DESMAN_HIP_DEVICE");
    if (e) dev = atoi(e);
    return dsm_ctx_create(&g_legacy, dev);
}

extern "C" int dsm_initRNG(void)
{
    std::lock_guard<std::mutex> lk(g_legacy_mu);
    DSM_TRY(legacy_ctx());
    g_legacy_rng = true;
    return seed_mt(g_legacy, 0);          // gsl_rng_alloc: default seed
}

extern "C" int dsm_setRNG(unsigned long seed)
{
    std::lock_guard<std::mutex> lk(g_legacy_mu);
    if (!g_legacy || !g_legacy_rng) { dsm_set_error("setRNG before initRNG"); return DSM_ERR_STATE; }
    return seed_mt(g_legacy, seed);
}

extern "C" int dsm_freeRNG(void)
{
    std::lock_guard<std::mutex> lk(g_legacy_mu);
    g_legacy_rng = false;
    if (g_legacy) g_legacy->mt_seeded = false;
    return DSM_OK;
}

extern "C" int dsm_getRNG_state(uint32_t *state625)
{
    std::lock_guard<std::mutex> lk(g_legacy_mu);
    if (!g_legacy || !g_legacy_rng) { dsm_set_error("getRNG_state: RNG not initialised"); return DSM_ERR_STATE; }
    return dsm_ctx_get_mt_state(g_legacy, state625);
}

extern "C" int dsm_setRNG_state(const uint32_t *state625)
{
    std::lock_guard<std::mutex> lk(g_legacy_mu);
    if (!g_legacy || !g_legacy_rng) { dsm_set_error("setRNG_state: RNG not initialised"); return DSM_ERR_STATE; }
    return dsm_ctx_set_mt_state(g_legacy, state625);
}

extern "C" int dsm_sample_tau(int64_t *tau, const double *pi, const double *eta, const int64_t *variants, int nV, int nG, int nS)
{
    std::lock_guard<std::mutex> lk(g_legacy_mu);
    if (!tau || !pi || !eta || !variants || nV < 0 || nG < 1 || nS < 1) { dsm_set_error("sample_tau: bad arguments"); return DSM_ERR_ARG; }
    if (nV == 0) return 0;
    if (!g_legacy || !g_legacy_rng) { dsm_set_error("sample_tau: RNG not initialised (initRNG/setRNG)"); return DSM_ERR_STATE; }
    dsm_ctx *c = g_legacy;
    c->tau_rng = DSM_RNG_MT19937;
    const uint64_t hsh = hash_words(variants, (size_t)nV * nS * 4);
    if (!(c->cnt_vs && variants == g_legacy_ptr && nV == g_legacy_V && nS == g_legacy_S && hsh == g_legacy_hash)) {
        g_legacy_ptr = nullptr;
        DSM_TRY(dsm_ctx_set_counts(c, variants, nV, nS));
        g_legacy_ptr = variants; g_legacy_V = nV; g_legacy_S = nS; g_legacy_hash = hsh;
    }
    DSM_TRY(dsm_ctx_set_state(c, tau, pi, eta, nG));
    int n = 0;
    DSM_TRY(dsm_ctx_sample_tau(c, &n, nullptr));
    DSM_TRY(dsm_ctx_get_state(c, tau, nullptr, nullptr));
    return n;
}

// ---------------------------------------------------------------- reference-named aliases
// The four symbols sampletau/sampletau.pyx:10-16 declares (`cdef extern from "c_sample_tau.h"`), with the
// reference's own prototypes (c_sample_tau.c:26,36,42,95: `long` = int64 on LP64), so the unmodified .pyx links
// against this library with only a `libraries=` change in setup.py.  The reference has no
// error channel (malloc failure -> message + exit(1), c_sample_tau.c:200-203): errors are reported on stderr;
// c_sample_tau then returns -1 (the reference's callers add the return value to a change counter).
static void alias_report(const char *fn, int rc)
{
    if (rc < 0) fprintf(stderr, "desman_hip: %s failed (%d): %s\n", fn, rc, dsm_last_error());
}
extern "C" void c_initRNG(void) { alias_report("c_initRNG", dsm_initRNG()); }
extern "C" void c_setRNG(unsigned long seed) { alias_report("c_setRNG", dsm_setRNG(seed)); }
extern "C" void c_freeRNG(void) { alias_report("c_freeRNG", dsm_freeRNG()); }
extern "C" int c_sample_tau(long *tau, double *pi, double *eta, long *variants, int nV, int nG, int nS)
{
    static_assert(sizeof(long) == sizeof(int64_t), "LP64 expected");
    const int rc = dsm_sample_tau(reinterpret_cast<int64_t *>(tau), pi, eta, reinterpret_cast<const int64_t *>(variants), nV, nG, nS);
    alias_report("c_sample_tau", rc);
    return rc < 0 ? -1 : rc;
}
