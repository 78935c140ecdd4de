// hrx_verify_api.cpp — hrx_verify_rows_device / hrx_verify_rows_device_planes / hrx_verify_rows_host (include/hrx.h VERIFY): do these witness rows satisfy
// the circuit?  The rules are hrx_verify.hpp's, the kernel is hrx_kernel_verify.hip, the host form hrx_verify_host.cpp.  The check tables are the context's:
// built from the rows RegexTableConfig::load assigns (table_transition_rows / table_endpoint_rows — never from a walk table) at the context's first verify
// call, under its lock, and for a device call uploaded then; after that a device call is one launch and nothing else.  DESIGN.md §17.
// The chunked forms (hrx_verify_rows_chunked_device / _planes / _host, hrx_verify_chunked_workspace_bytes, hrx_ctx_verify_chunk_rows) take
// the same arguments through the same checks, a chunk size (0: plan_verify_chunk_rows of hrx_plan.cpp) and a workspace for the chunks' summaries; a device
// call is two launches and nothing else.
#include "hrx_ctx.hpp"
#include "hrx_kernel.hpp"
#include "hrx_plan.hpp"
#include "hrx_verify.hpp"

namespace hrx {
void verify_rows_host(const VerifyArgs &a, unsigned threads);      // hrx_verify_host.cpp
void verify_rows_chunked_host(const VerifyArgs &a, uint32_t chunk_rows, uint32_t *summaries, unsigned threads);
}
using namespace hrx;
static_assert(kVfyFirstState == HRX_VERIFY_FIRST_STATE && kVfyEnable == HRX_VERIFY_ENABLE && kVfyTransition == HRX_VERIFY_TRANSITION &&
                  kVfyStartLookup == HRX_VERIFY_START_LOOKUP && kVfyEndLookup == HRX_VERIFY_END_LOOKUP && kVfyAccept == HRX_VERIFY_ACCEPT &&
                  kVfyFlags == HRX_VERIFY_FLAGS && kVfyPadding == HRX_VERIFY_PADDING && kVfyMask == HRX_VERIFY_MASK && kVfyRowShift == HRX_VERIFY_ROW_SHIFT,
              "hrx_verify.hpp and include/hrx.h");

// the argument rules the forms share: check_rows' (hrx_rows_api.cpp) for the rows, and the verdict's; fills `a` but image
static int check_verify_args(const hrx_ctx *ctx, const RowsCall &c, uint64_t *verdict, bool device, VerifyArgs &a) {
    if (!c.masked || !verdict) return fail(HRX_ERR_ARG, "NULL buffer");
    if ((uintptr_t)verdict & 7) return fail(HRX_ERR_ARG, "verdict must be 8-byte aligned");
    a = VerifyArgs{};
    if (int rc = check_rows(ctx, c, device, a)) return rc;
    a.verdict = verdict;
    return HRX_OK;
}

static int verify_image_host(hrx_ctx *ctx) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ctx_image_host(ctx, ctx->verify_img, build_verify_image, "verify");
}
static int verify_image_device(hrx_ctx *ctx, void *stream) { return ctx_image_device(ctx, ctx->verify_img, build_verify_image, "verify", stream); }

static int verify_device_any(hrx_ctx *ctx, const RowsCall &c, uint64_t *verdict, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (c.B == 0) return HRX_OK;
    VerifyArgs a;
    if (int rc = check_verify_args(ctx, c, verdict, true, a)) return rc;
    if (int rc = check_has_device(ctx)) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    if (int rc = verify_image_device(ctx, stream)) return rc;
    a.image = (const uint32_t *)ctx->verify_img.dev.p;
    HIP_TRY(launch_verify_rows(a, (hipStream_t)stream));
    return HRX_OK;
}

// chunk_rows as the chunked entry points take it: 0 = the context's pick; otherwise a multiple of kVfyChunkAlign, cut to one chunk where it reaches M
static int resolve_chunk_rows(const hrx_ctx *ctx, size_t B, size_t M, size_t chunk_rows, uint32_t &out) {
    if (chunk_rows == 0) chunk_rows = plan_verify_chunk_rows(B, M, ctx->num_cus);
    if (chunk_rows % kVfyChunkAlign) return fail(HRX_ERR_ARG, "chunk_rows must be 0 or a multiple of 32");
    const size_t one = (M + kVfyChunkAlign - 1) / kVfyChunkAlign * kVfyChunkAlign;
    out = (uint32_t)std::min(chunk_rows, one);
    return HRX_OK;
}

static int verify_chunked_device_any(hrx_ctx *ctx, const RowsCall &c, size_t chunk_rows, void *workspace, size_t workspace_bytes, uint64_t *verdict,
                                     void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    const size_t B = c.B, M = c.M;
    if (B == 0) return HRX_OK;
    VerifyChunkArgs ca{};
    if (int rc = check_verify_args(ctx, c, verdict, true, ca.a)) return rc;
    if (int rc = resolve_chunk_rows(ctx, B, M, chunk_rows, ca.chunk_rows)) return rc;
    ca.K = verify_chunk_count(ca.a.M, ca.chunk_rows);
    if (!workspace || ((uintptr_t)workspace & 15)) return fail(HRX_ERR_ARG, "workspace must be 16-byte aligned and not NULL");
    if (workspace_bytes < verify_chunked_workspace_bytes(B, M, ca.chunk_rows))
        return fail(HRX_ERR_ARG, "workspace smaller than hrx_verify_chunked_workspace_bytes(B, M, chunk_rows)");
    if ((B + 63) / 64 * (size_t)ca.K > 0x7fffffffull) return fail(HRX_ERR_ARG, "more (64 strings, chunk) pairs than a launch has workgroups: use larger chunks");
    ca.summaries = (uint32_t *)workspace;
    if (int rc = check_has_device(ctx)) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    if (int rc = verify_image_device(ctx, stream)) return rc;
    ca.a.image = (const uint32_t *)ctx->verify_img.dev.p;
    HIP_TRY(launch_verify_chunked(ca, (hipStream_t)stream));
    return HRX_OK;
}

extern "C" {

int hrx_verify_rows_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                           const uint16_t *masked, size_t msk_pitch, size_t B, size_t M, uint64_t *verdict, void *stream) {
    return verify_device_any(ctx, RowsCall{layout, chars, stride, lens, records, nullptr, 0, rec_pitch, masked, msk_pitch, B, M}, verdict, stream);
}

int hrx_verify_rows_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *const *record_planes,
                                  size_t n_planes, const uint16_t *masked, size_t B, size_t M, uint64_t *verdict, void *stream) {
    if (!record_planes) return fail(HRX_ERR_ARG, "NULL buffer");
    return verify_device_any(ctx, RowsCall{layout, chars, stride, lens, nullptr, record_planes, n_planes, 0, masked, 0, B, M}, verdict, stream);
}

int hrx_verify_rows_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                         const uint16_t *masked, size_t msk_pitch, size_t B, size_t M, uint64_t *verdict) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (B == 0) return HRX_OK;
    VerifyArgs a;
    const RowsCall c{layout, chars, stride, lens, records, nullptr, 0, rec_pitch, masked, msk_pitch, B, M};
    if (int rc = check_verify_args(ctx, c, verdict, false, a)) return rc;
    if (int rc = verify_image_host(ctx)) return rc;
    a.image = ctx->verify_img.host.data();       // (never rebuilt once it is there)
    verify_rows_host(a, ctx_host_threads(ctx));
    return HRX_OK;
}

size_t hrx_verify_chunked_workspace_bytes(size_t B, size_t M, size_t chunk_rows) { return verify_chunked_workspace_bytes(B, M, chunk_rows); }

size_t hrx_ctx_verify_chunk_rows(hrx_ctx *ctx, size_t B, size_t M) {
    if (!ctx) return 0;
    return plan_verify_chunk_rows(B, M, ctx->num_cus);
}

int hrx_verify_rows_chunked_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                                   const uint16_t *masked, size_t msk_pitch, size_t B, size_t M, size_t chunk_rows, void *workspace, size_t workspace_bytes,
                                   uint64_t *verdict, void *stream) {
    return verify_chunked_device_any(ctx, RowsCall{layout, chars, stride, lens, records, nullptr, 0, rec_pitch, masked, msk_pitch, B, M}, chunk_rows, workspace,
                                     workspace_bytes, verdict, stream);
}

int hrx_verify_rows_chunked_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *const *record_planes,
                                          size_t n_planes, const uint16_t *masked, size_t B, size_t M, size_t chunk_rows, void *workspace, size_t workspace_bytes,
                                          uint64_t *verdict, void *stream) {
    if (!record_planes) return fail(HRX_ERR_ARG, "NULL buffer");
    return verify_chunked_device_any(ctx, RowsCall{layout, chars, stride, lens, nullptr, record_planes, n_planes, 0, masked, 0, B, M}, chunk_rows, workspace,
                                     workspace_bytes, verdict, stream);
}

int hrx_verify_rows_chunked_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                                 const uint16_t *masked, size_t msk_pitch, size_t B, size_t M, size_t chunk_rows, uint64_t *verdict) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (B == 0) return HRX_OK;
    VerifyArgs a;
    const RowsCall c{layout, chars, stride, lens, records, nullptr, 0, rec_pitch, masked, msk_pitch, B, M};
    if (int rc = check_verify_args(ctx, c, verdict, false, a)) return rc;
    uint32_t C;
    if (int rc = resolve_chunk_rows(ctx, B, M, chunk_rows, C)) return rc;
    if (int rc = verify_image_host(ctx)) return rc;
    a.image = ctx->verify_img.host.data();
    std::vector<uint32_t> summaries;      // (the device form's workspace; here the call's own)
    try {
        summaries.resize(verify_chunked_workspace_bytes(B, M, C) / 4);
    } catch (const std::bad_alloc &) {
        return fail(HRX_ERR_BOUNDS, "verify: no memory for the chunk summaries: use larger chunks");
    }
    verify_rows_chunked_host(a, C, summaries.data(), ctx_host_threads(ctx));
    return HRX_OK;
}

}  // extern "C"
