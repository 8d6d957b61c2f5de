// dsm_host_util.h -- the host scaffolding of an entry point (internal): early return, device buffers, device and context selection, the
// input rules the tools share, the staging of a count chunk, the LDS gate, the debug knobs.  Plain functions and one class template; a
// function whose message names the tool takes it as `who`.  A new tool starts from these, not from a copy of another tool's host half.
#pragma once
#include <math.h>

#include <vector>

#include "dsm_host.h"
#include "log_table.h"

#define DSM_TRY(x) do { int _r = (x); if (_r != DSM_OK) return _r; } while (0)
#define BIND(c) HIP_TRY(hipSetDevice((c)->device))

// *p freed, then room for n (at least one) elements; *p is null after a failure
template <typename T>
static inline int dev_alloc(T **p, size_t n)
{
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e != hipSuccess) { *p = nullptr; dsm_set_error("hipMalloc(%zu B) failed: %s", n * sizeof(T), hipGetErrorString(e)); return DSM_ERR_NOMEM; }
    return DSM_OK;
}

// device buffer released on every exit path (error returns included)
template <typename T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) { return dev_alloc(&p, n); }
    operator T *() const { return p; }
};

// the device of a call that has no context
static inline int dsm_bind_device(int device)
{
    const int nd = dsm_device_count();
    if (nd <= 0) { dsm_set_error("no HIP device visible"); return DSM_ERR_NODEVICE; }
    if (device < 0 || device >= nd) { dsm_set_error("device %d out of range (0..%d)", device, nd - 1); return DSM_ERR_ARG; }
    HIP_TRY(hipSetDevice(device));
    return DSM_OK;
}

// what a call needs of its context: the count tensor, the chain state
static inline int dsm_ctx_need(dsm_ctx *c, bool counts, bool state)
{
    if (!c) { dsm_set_error("null context"); return DSM_ERR_ARG; }
    if (counts && !c->cnt_vs) { dsm_set_error("no count tensor: call dsm_ctx_set_counts first"); return DSM_ERR_STATE; }
    if (state && !c->have_state) { dsm_set_error("no chain state: call dsm_ctx_set_state first"); return DSM_ERR_STATE; }
    return DSM_OK;
}

// the opening of a tool's context form: a context with counts, its device current
static inline int dsm_ctx_enter(dsm_ctx *c, bool sync)
{
    DSM_TRY(dsm_ctx_need(c, true, false));
    HIP_TRY(hipSetDevice(c->device));
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));      // the tools read the resident tensors from the default stream
    return DSM_OK;
}

// the count rules of dsm_ctx_set_counts on a caller's table [cells][S][4]: no negative count, no cell and no depth above 2^31 - 1 reads
static inline int dsm_check_counts(const char *who, const int64_t *counts, size_t cells, int S)
{
    for (size_t i = 0; i < cells * (size_t)S; ++i) {
        int64_t tot = 0;
        for (int b = 0; b < 4; ++b) {
            const int64_t x = counts[i * 4 + b];
            if (x < 0 || x > 2147483647ll) { dsm_set_error("%s: count %lld at position %zu, sample %zu", who, (long long)x, i / S, i % S); return DSM_ERR_ARG; }
            tot += x;
        }
        if (tot > 2147483647ll) { dsm_set_error("%s: depth above 2^31-1 at position %zu, sample %zu", who, i / S, i % S); return DSM_ERR_ARG; }
    }
    return DSM_OK;
}

static inline int dsm_check_eta(const char *who, const double *eta)
{
    for (int i = 0; i < 16; ++i)
        if (!(eta[i] >= 0.0) || !std::isfinite(eta[i])) { dsm_set_error("%s: eta[%d] is negative or not finite", who, i); return DSM_ERR_ARG; }
    return DSM_OK;
}

static inline int dsm_check_gamma(const char *who, const double *gamma, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!(gamma[i] >= 0.0) || !std::isfinite(gamma[i])) { dsm_set_error("%s: gamma[%zu] is negative or not finite", who, i); return DSM_ERR_ARG; }
    return DSM_OK;
}

// `words` checked counts of the caller's int64 table as int32 in d_x, through x32.  A null stream: one blocking copy; otherwise a copy
// on the stream and the wait for it (x32 is refilled for the next chunk)
static inline int dsm_stage_counts(const int64_t *src, size_t words, int32_t *d_x, std::vector<int32_t> &x32, hipStream_t stream)
{
    x32.resize(words);
    for (size_t i = 0; i < words; ++i) x32[i] = (int32_t)src[i];
    if (!stream) HIP_TRY(hipMemcpy(d_x, x32.data(), words * sizeof(int32_t), hipMemcpyHostToDevice));
    else {
        HIP_TRY(hipMemcpyAsync(d_x, x32.data(), words * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    return DSM_OK;
}

// the table of dsm_log (log_table.h) for a call that has no context: d_ltab [256][2]
static inline int dsm_upload_log_table(double *d_ltab)
{
    HIP_TRY(hipMemcpy(d_ltab, dsm_log_table_host, sizeof dsm_log_table_host, hipMemcpyHostToDevice));
    return DSM_OK;
}

// a kernel launched with `lds` bytes of dynamic LDS: more than the 160 KB of a compute unit cannot run, more than 48 KB has to be asked for
static inline int dsm_allow_lds(const void *fn, size_t lds, const char *who)
{
    if (lds > 160 * 1024) { dsm_set_error("%s: %zu B of LDS", who, lds); return DSM_ERR_UNSUPPORTED; }
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return DSM_OK;
}

// a debug knob: 0 = the default, a positive value replaces it
static inline int dsm_set_knob(int *knob, long long value, const char *who, const char *what)
{
    if (value < 0) { dsm_set_error("%s: %s %lld", who, what, value); return DSM_ERR_ARG; }
    *knob = (int)value;
    return DSM_OK;
}
