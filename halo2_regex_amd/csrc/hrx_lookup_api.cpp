// hrx_lookup_api.cpp — hrx_lookup_words_per_string / hrx_lookup_layout / hrx_lookup_counts_device / _device_planes / _host / hrx_ctx_lookup_group
// (include/hrx.h LOOKUP COUNTS): how often a string's advice rows hit each row of the circuit's three fixed lookup tables per def.  The rule is
// hrx_lookup.hpp's, the kernel hrx_kernel_lookup.hip, the host form hrx_lookup_host.cpp.  The image is the context's: built from the rows
// RegexTableConfig::load assigns (table_transition_rows / table_endpoint_rows — never from a walk table) at the context's first lookup call, under its
// lock, and for a device call uploaded then; after that a device call is one launch and nothing else.  DESIGN.md §18.
#include "hrx_ctx.hpp"
#include "hrx_kernel.hpp"
#include "hrx_lookup.hpp"

namespace hrx {
void lookup_counts_host(const LookupArgs &a, unsigned threads);      // hrx_lookup_host.cpp
}
using namespace hrx;

// the run of one string: per def (offset of trans[], T_d, E_d), and W
static size_t lookup_run_of(const DefsSet &s, size_t def, size_t *off, size_t *n_tr, size_t *n_ep) {
    size_t w = 0;
    for (size_t d = 0; d < s.defs.size(); ++d) {
        const size_t t = table_transition_rows(s, d, nullptr, 0), e = table_endpoint_rows(s, d, nullptr, 0);
        if (d == def) { *off = w; *n_tr = t; *n_ep = e; }
        w += t + 2 * e;
    }
    return (w + 3) & ~(size_t)3;
}

// the argument rules the forms share: check_rows' (hrx_rows_api.cpp) for the rows (no masked rows), hrx_fr_columns_device's for the window, the outputs'
static int check_lookup_args(const hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records,
                             const uint32_t *const *planes, size_t n_planes, size_t rec_pitch, size_t B, size_t M, size_t b_begin, size_t b_count,
                             uint32_t *counts, uint32_t *misses, bool device, LookupArgs &a) {
    if (!counts) return fail(HRX_ERR_ARG, "NULL buffer");
    if (b_begin > B || b_count > B - b_begin) return fail(HRX_ERR_ARG, "string range outside the batch");
    if (((uintptr_t)counts & 15) || ((uintptr_t)misses & 3)) return fail(HRX_ERR_ARG, "counts must be 16-byte aligned, misses 4-byte");
    a = LookupArgs{};
    if (int rc = check_rows(ctx, layout, chars, stride, lens, records, planes, n_planes, rec_pitch, nullptr, 0, B, M, device, a)) return rc;
    a.b_begin = (uint32_t)b_begin; a.b_count = (uint32_t)b_count;
    a.counts = counts; a.misses = misses;
    return HRX_OK;
}

static int lookup_image_host(hrx_ctx *ctx) { return ctx_image_host(ctx, ctx->lookup_img, build_lookup_image, "lookup counts"); }
static int lookup_image_device(hrx_ctx *ctx, void *stream) { return ctx_image_device(ctx, ctx->lookup_img, build_lookup_image, "lookup counts", stream); }

static int lookup_device_any(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records,
                             const uint32_t *const *planes, size_t n_planes, size_t rec_pitch, size_t B, size_t M, size_t b_begin, size_t b_count,
                             uint32_t *counts, uint32_t *misses, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    LookupArgs a;
    if (int rc = check_lookup_args(ctx, layout, chars, stride, lens, records, planes, n_planes, rec_pitch, B, M, b_begin, b_count, counts, misses, true, a)) return rc;
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    if (int rc = lookup_image_device(ctx, stream)) return rc;
    a.image = (const uint32_t *)ctx->lookup_img.dev.p;
    a.W = lookup_words(ctx->lookup_img.host.data(), a.D);
    const LookupPlan p = plan_lookup(a.W, b_count, ctx->num_cus);
    a.G = p.G; a.pass_words = p.pass_words; a.passes = p.passes;
    if ((b_count + p.G - 1) / p.G > 0x7fffffffull) return fail(HRX_ERR_ARG, "more groups of strings than a launch has workgroups: use a smaller window");
    HIP_TRY(launch_lookup_counts(a, p.lds_bytes, (hipStream_t)stream));
    return HRX_OK;
}

extern "C" {

size_t hrx_lookup_words_per_string(const hrx_defs *defs) {
    if (!defs || defs->s.defs.empty()) return 0;
    size_t off, t, e;
    return lookup_run_of(defs->s, 0, &off, &t, &e);
}

int hrx_lookup_layout(const hrx_defs *defs, size_t def, size_t *trans_off, size_t *trans_rows, size_t *start_off, size_t *end_off, size_t *endpoint_rows) {
    if (!defs || !trans_off || !trans_rows || !start_off || !end_off || !endpoint_rows) return fail(HRX_ERR_ARG, "NULL argument");
    if (def >= defs->s.defs.size()) return fail(HRX_ERR_ARG, "def out of range");
    size_t off = 0, t = 0, e = 0;
    lookup_run_of(defs->s, def, &off, &t, &e);
    *trans_off = off; *trans_rows = t; *start_off = off + t; *end_off = off + t + e; *endpoint_rows = e;
    return HRX_OK;
}

int hrx_ctx_lookup_group(hrx_ctx *ctx, size_t b_count, size_t *group, size_t *passes) {
    if (!ctx || !group || !passes) return fail(HRX_ERR_ARG, "NULL argument");
    size_t off, t, e;
    const LookupPlan p = plan_lookup(lookup_run_of(ctx->s, 0, &off, &t, &e), b_count, ctx->num_cus);
    *group = p.G; *passes = p.passes;
    return HRX_OK;
}

int hrx_lookup_counts_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                             size_t B, size_t M, size_t b_begin, size_t b_count, uint32_t *counts, uint32_t *misses, void *stream) {
    return lookup_device_any(ctx, layout, chars, stride, lens, records, nullptr, 0, rec_pitch, B, M, b_begin, b_count, counts, misses, stream);
}

int hrx_lookup_counts_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *const *record_planes,
                                    size_t n_planes, size_t B, size_t M, size_t b_begin, size_t b_count, uint32_t *counts, uint32_t *misses, void *stream) {
    if (!record_planes) return fail(HRX_ERR_ARG, "NULL buffer");
    return lookup_device_any(ctx, layout, chars, stride, lens, nullptr, record_planes, n_planes, 0, B, M, b_begin, b_count, counts, misses, stream);
}

int hrx_lookup_counts_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                           size_t B, size_t M, size_t b_begin, size_t b_count, uint32_t *counts, uint32_t *misses) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    LookupArgs a;
    if (int rc = check_lookup_args(ctx, layout, chars, stride, lens, records, nullptr, 0, rec_pitch, B, M, b_begin, b_count, counts, misses, false, a)) return rc;
    unsigned threads;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int rc = lookup_image_host(ctx)) return rc;
        threads = ctx->host_threads > 0 ? (unsigned)ctx->host_threads : 0u;
    }
    a.image = ctx->lookup_img.host.data();       // (never rebuilt once it is there)
    a.W = lookup_words(a.image, a.D);
    lookup_counts_host(a, threads);
    return HRX_OK;
}

}  // extern "C"
