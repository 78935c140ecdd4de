// hrx_lookup_api.cpp — hrx_lookup_words_per_string / hrx_lookup_layout / hrx_lookup_counts_device / _device_planes / _host / hrx_ctx_lookup_group
// (include/hrx.h LOOKUP COUNTS): how often a string's advice rows hit each row of the circuit's three fixed lookup tables per def.  The rule is
// hrx_lookup.hpp's, the kernel hrx_kernel_lookup.hip, the host form hrx_lookup_host.cpp.  The image is the context's: built from the rows
// RegexTableConfig::load assigns (table_transition_rows / table_endpoint_rows — never from a walk table) at the context's first lookup call, under its
// lock, and for a device call uploaded then; after that a device call is one launch and nothing else.  DESIGN.md §18.
#include "hrx_ctx.hpp"
#include "hrx_kernel.hpp"
#include "hrx_lookup.hpp"      // hrx_lookup_run.hpp: the run's layout

namespace hrx {
void lookup_counts_host(const LookupArgs &a, unsigned threads);      // hrx_lookup_host.cpp
}
using namespace hrx;

// the argument rules the forms share: check_rows' (hrx_rows_api.cpp) for the rows (no masked rows), check_window's, the outputs'
static int check_lookup_args(const hrx_ctx *ctx, const RowsCall &c, size_t b_begin, size_t b_count, uint32_t *counts, uint32_t *misses, bool device,
                             LookupArgs &a) {
    if (!counts) return fail(HRX_ERR_ARG, "NULL buffer");
    if (int rc = check_window(c.B, b_begin, b_count)) return rc;
    if (((uintptr_t)counts & 15) || ((uintptr_t)misses & 3)) return fail(HRX_ERR_ARG, "counts must be 16-byte aligned, misses 4-byte");
    a = LookupArgs{};
    if (int rc = check_rows(ctx, c, device, a)) return rc;
    a.b_begin = (uint32_t)b_begin; a.b_count = (uint32_t)b_count;
    a.counts = counts; a.misses = misses;
    return HRX_OK;
}

static int lookup_image_host(hrx_ctx *ctx) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ctx_image_host(ctx, ctx->lookup_img, build_lookup_image, "lookup counts");
}
static int lookup_image_device(hrx_ctx *ctx, void *stream) { return ctx_image_device(ctx, ctx->lookup_img, build_lookup_image, "lookup counts", stream); }

static int lookup_device_any(hrx_ctx *ctx, const RowsCall &c, size_t b_begin, size_t b_count, uint32_t *counts, uint32_t *misses, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    LookupArgs a;
    if (int rc = check_lookup_args(ctx, c, b_begin, b_count, counts, misses, true, a)) return rc;
    if (int rc = check_has_device(ctx)) return rc;
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
    LookupRun run;
    return defs && defs_lookup_run(defs->s, run) ? run.W : 0;
}

int hrx_lookup_layout(const hrx_defs *defs, size_t def, size_t *trans_off, size_t *trans_rows, size_t *start_off, size_t *end_off, size_t *endpoint_rows) {
    if (!defs || !trans_off || !trans_rows || !start_off || !end_off || !endpoint_rows) return fail(HRX_ERR_ARG, "NULL argument");
    if (def >= defs->s.defs.size()) return fail(HRX_ERR_ARG, "def out of range");
    LookupRun run;
    if (!defs_lookup_run(defs->s, run)) return fail(HRX_ERR_ARG, "lookup layout: more defs than HRX_MAX_DEFS, or more bins than a u32 run indexes");
    const PermuteCol tr = lookup_run_col(run, 3 * (uint32_t)def), st = lookup_run_col(run, 3 * (uint32_t)def + 1), en = lookup_run_col(run, 3 * (uint32_t)def + 2);
    *trans_off = tr.off; *trans_rows = tr.T; *start_off = st.off; *end_off = en.off; *endpoint_rows = en.T;
    return HRX_OK;
}

int hrx_ctx_lookup_group(hrx_ctx *ctx, size_t b_count, size_t *group, size_t *passes) {
    if (!ctx || !group || !passes) return fail(HRX_ERR_ARG, "NULL argument");
    LookupRun run;
    if (!defs_lookup_run(ctx->s, run)) return fail(HRX_ERR_ARG, "lookup group: more defs than HRX_MAX_DEFS, or more bins than a u32 run indexes");
    const LookupPlan p = plan_lookup(run.W, b_count, ctx->num_cus);
    *group = p.G; *passes = p.passes;
    return HRX_OK;
}

int hrx_lookup_counts_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                             size_t B, size_t M, size_t b_begin, size_t b_count, uint32_t *counts, uint32_t *misses, void *stream) {
    return lookup_device_any(ctx, RowsCall{layout, chars, stride, lens, records, nullptr, 0, rec_pitch, nullptr, 0, B, M}, b_begin, b_count, counts, misses, stream);
}

int hrx_lookup_counts_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *const *record_planes,
                                    size_t n_planes, size_t B, size_t M, size_t b_begin, size_t b_count, uint32_t *counts, uint32_t *misses, void *stream) {
    if (!record_planes) return fail(HRX_ERR_ARG, "NULL buffer");
    return lookup_device_any(ctx, RowsCall{layout, chars, stride, lens, nullptr, record_planes, n_planes, 0, nullptr, 0, B, M}, b_begin, b_count, counts, misses, stream);
}

int hrx_lookup_counts_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                           size_t B, size_t M, size_t b_begin, size_t b_count, uint32_t *counts, uint32_t *misses) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    LookupArgs a;
    const RowsCall c{layout, chars, stride, lens, records, nullptr, 0, rec_pitch, nullptr, 0, B, M};
    if (int rc = check_lookup_args(ctx, c, b_begin, b_count, counts, misses, false, a)) return rc;
    if (int rc = lookup_image_host(ctx)) return rc;
    a.image = ctx->lookup_img.host.data();       // (never rebuilt once it is there)
    a.W = lookup_words(a.image, a.D);
    lookup_counts_host(a, ctx_host_threads(ctx));
    return HRX_OK;
}

}  // extern "C"
