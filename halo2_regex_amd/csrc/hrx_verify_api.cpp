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
static_assert(kVfyPmBlock == HRX_PM_BLOCK && kVfyMaxPlanes == kMaxDefsPerLaunch, "hrx_verify.hpp, include/hrx.h and hrx_kernel.hpp");
static_assert(kVfyFirstState == HRX_VERIFY_FIRST_STATE && kVfyEnable == HRX_VERIFY_ENABLE && kVfyTransition == HRX_VERIFY_TRANSITION &&
                  kVfyStartLookup == HRX_VERIFY_START_LOOKUP && kVfyEndLookup == HRX_VERIFY_END_LOOKUP && kVfyAccept == HRX_VERIFY_ACCEPT &&
                  kVfyFlags == HRX_VERIFY_FLAGS && kVfyPadding == HRX_VERIFY_PADDING && kVfyMask == HRX_VERIFY_MASK && kVfyRowShift == HRX_VERIFY_ROW_SHIFT,
              "hrx_verify.hpp and include/hrx.h");

// the context's check tables in host memory (the caller holds ctx->mu)
static int verify_image_ready(hrx_ctx *ctx) {
    if (!ctx->verify_image.empty()) return HRX_OK;
    const size_t D = ctx->s.defs.size();
    std::vector<std::vector<uint64_t>> tr(D), ep(D);
    std::vector<VerifyDefRows> rows(D);
    for (size_t d = 0; d < D; ++d) {
        tr[d].resize(4 * table_transition_rows(ctx->s, d, nullptr, 0));
        table_transition_rows(ctx->s, d, tr[d].data(), tr[d].size() / 4);
        ep[d].resize(3 * table_endpoint_rows(ctx->s, d, nullptr, 0));
        table_endpoint_rows(ctx->s, d, ep[d].data(), ep[d].size() / 3);
        const AllstrRegexDef &al = ctx->s.defs[d].allstr;
        rows[d] = VerifyDefRows{tr[d].data(), tr[d].size() / 4, ep[d].data(), ep[d].size() / 3, al.first_state_val, al.accepted_state_val};
    }
    std::vector<uint32_t> img;
    if (!build_verify_image(rows.data(), D, img)) return fail(HRX_ERR_BOUNDS, "verify: the config's table rows do not fit the checker's dense tables");
    ctx->verify_image = std::move(img);
    return HRX_OK;
}

// the argument rules the three forms share, in the order the errors are reported; fills `a` but image and verdict's meaning
static int check_verify_args(const hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records,
                             const uint32_t *const *planes, size_t n_planes, size_t rec_pitch, const uint16_t *masked, size_t msk_pitch, size_t B, size_t M,
                             uint64_t *verdict, bool device, VerifyArgs &a) {
    if (!chars || !lens || !masked || !verdict || (!records && !planes)) return fail(HRX_ERR_ARG, "NULL buffer");
    if (M == 0 || M > kVfyMaxRows || B > 0xffffffffull - 64) return fail(HRX_ERR_ARG, "shape out of range");
    if (layout != HRX_LAYOUT_STRING_MAJOR && layout != HRX_LAYOUT_POSITION_MAJOR && layout != (HRX_LAYOUT_POSITION_MAJOR | HRX_LAYOUT_INPUT_POSITION_MAJOR))
        return fail(HRX_ERR_ARG, "unknown layout");
    const bool pm = (layout & HRX_LAYOUT_POSITION_MAJOR) != 0;
    const size_t Dn = ctx->s.defs.size();
    if (planes) {
        if (!pm) return fail(HRX_ERR_ARG, "record planes are a position-major layout");
        if (!(n_planes == Dn || (Dn == 1 && n_planes == 2)) || n_planes > kVfyMaxPlanes)
            return fail(HRX_ERR_ARG, "record planes: one buffer per def (at most eight; one def: one buffer or two row stripes)");
        for (size_t d = 0; d < n_planes; ++d)
            if (!planes[d]) return fail(HRX_ERR_ARG, "NULL plane");
    }
    if (!rec_pitch) rec_pitch = M;
    if (!msk_pitch) msk_pitch = M;
    if (!pm && (rec_pitch < M || msk_pitch < M)) return fail(HRX_ERR_ARG, "pitches < M");
    if (((uintptr_t)verdict & 7) || ((uintptr_t)lens & 3)) return fail(HRX_ERR_ARG, "verdict must be 8-byte aligned, lens 4-byte");
    if (device) {     // the kernel reads 16-byte chunks, quads and octets: the alignment of the witness entry points that wrote the rows
        bool ok = !(stride & 15) && !((uintptr_t)chars & 15) && !((uintptr_t)records & 15) && !((uintptr_t)masked & 15);
        for (size_t d = 0; planes && d < n_planes; ++d) ok = ok && !((uintptr_t)planes[d] & 15);
        if (!ok) return fail(HRX_ERR_ARG, "chars, records, masked and every record plane must be 16-byte aligned, stride % 16 == 0");
    } else if (((uintptr_t)records & 3) || ((uintptr_t)masked & 1) || ((layout & HRX_LAYOUT_INPUT_POSITION_MAJOR) && (stride & 15))) {
        return fail(HRX_ERR_ARG, "records must be 4-byte aligned, masked 2-byte; position-major input: stride % 16 == 0");
    }
    a = VerifyArgs{};
    a.chars = chars; a.stride = stride; a.lens = lens; a.records = planes ? nullptr : records; a.masked = masked;
    for (size_t d = 0; planes && d < n_planes; ++d) a.planes[d] = planes[d];
    a.n_stripes = planes && n_planes == 2 * Dn ? 2u : 1u;
    a.B = (uint32_t)B; a.M = (uint32_t)M; a.D = (uint32_t)Dn; a.layout = (uint32_t)layout;
    a.rec_pitch = rec_pitch; a.msk_pitch = msk_pitch;
    a.verdict = verdict;
    return HRX_OK;
}

// the context's check tables on its device (the caller holds ctx->mu and has set the device).  First use: build and upload — an allocation and a
// blocking copy: not inside a stream capture
static int verify_tab_ready(hrx_ctx *ctx, void *stream) {
    if (ctx->verify_tab.p) return HRX_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing((hipStream_t)stream, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail(HRX_ERR_STATE, "verify: the context's check tables are built and uploaded at its first verify call, not inside a stream capture");
    if (int rc = verify_image_ready(ctx)) return rc;
    DevBuf tab;
    HIP_TRY(tab.reserve(ctx->verify_image.size() * 4));
    const hipError_t e = hipMemcpy(tab.p, ctx->verify_image.data(), ctx->verify_image.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        tab.release();
        return fail(HRX_ERR_HIP, std::string("verify: table upload: ") + hipGetErrorString(e));
    }
    ctx->verify_tab = tab;
    return HRX_OK;
}

static int verify_device_any(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records,
                             const uint32_t *const *planes, size_t n_planes, size_t rec_pitch, const uint16_t *masked, size_t msk_pitch, size_t B, size_t M,
                             uint64_t *verdict, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (B == 0) return HRX_OK;
    VerifyArgs a;
    if (int rc = check_verify_args(ctx, layout, chars, stride, lens, records, planes, n_planes, rec_pitch, masked, msk_pitch, B, M, verdict, true, a)) return rc;
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    if (int rc = verify_tab_ready(ctx, stream)) return rc;
    a.image = (const uint32_t *)ctx->verify_tab.p;
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

static int verify_chunked_device_any(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records,
                                     const uint32_t *const *planes, size_t n_planes, size_t rec_pitch, const uint16_t *masked, size_t msk_pitch, size_t B,
                                     size_t M, size_t chunk_rows, void *workspace, size_t workspace_bytes, uint64_t *verdict, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (B == 0) return HRX_OK;
    VerifyChunkArgs ca{};
    if (int rc = check_verify_args(ctx, layout, chars, stride, lens, records, planes, n_planes, rec_pitch, masked, msk_pitch, B, M, verdict, true, ca.a)) return rc;
    if (int rc = resolve_chunk_rows(ctx, B, M, chunk_rows, ca.chunk_rows)) return rc;
    ca.K = verify_chunk_count(ca.a.M, ca.chunk_rows);
    if (!workspace || ((uintptr_t)workspace & 15)) return fail(HRX_ERR_ARG, "workspace must be 16-byte aligned and not NULL");
    if (workspace_bytes < verify_chunked_workspace_bytes(B, M, ca.chunk_rows))
        return fail(HRX_ERR_ARG, "workspace smaller than hrx_verify_chunked_workspace_bytes(B, M, chunk_rows)");
    if ((B + 63) / 64 * (size_t)ca.K > 0x7fffffffull) return fail(HRX_ERR_ARG, "more (64 strings, chunk) pairs than a launch has workgroups: use larger chunks");
    ca.summaries = (uint32_t *)workspace;
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    if (int rc = verify_tab_ready(ctx, stream)) return rc;
    ca.a.image = (const uint32_t *)ctx->verify_tab.p;
    HIP_TRY(launch_verify_chunked(ca, (hipStream_t)stream));
    return HRX_OK;
}

extern "C" {

int hrx_verify_rows_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                           const uint16_t *masked, size_t msk_pitch, size_t B, size_t M, uint64_t *verdict, void *stream) {
    return verify_device_any(ctx, layout, chars, stride, lens, records, nullptr, 0, rec_pitch, masked, msk_pitch, B, M, verdict, stream);
}

int hrx_verify_rows_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *const *record_planes,
                                  size_t n_planes, const uint16_t *masked, size_t B, size_t M, uint64_t *verdict, void *stream) {
    if (!record_planes) return fail(HRX_ERR_ARG, "NULL buffer");
    return verify_device_any(ctx, layout, chars, stride, lens, nullptr, record_planes, n_planes, 0, masked, 0, B, M, verdict, stream);
}

int hrx_verify_rows_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                         const uint16_t *masked, size_t msk_pitch, size_t B, size_t M, uint64_t *verdict) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (B == 0) return HRX_OK;
    VerifyArgs a;
    if (int rc = check_verify_args(ctx, layout, chars, stride, lens, records, nullptr, 0, rec_pitch, masked, msk_pitch, B, M, verdict, false, a)) return rc;
    unsigned threads;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int rc = verify_image_ready(ctx)) return rc;
        threads = ctx->host_threads > 0 ? (unsigned)ctx->host_threads : 0u;
    }
    a.image = ctx->verify_image.data();       // (never rebuilt once it is there)
    verify_rows_host(a, threads);
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
    return verify_chunked_device_any(ctx, layout, chars, stride, lens, records, nullptr, 0, rec_pitch, masked, msk_pitch, B, M, chunk_rows, workspace,
                                     workspace_bytes, verdict, stream);
}

int hrx_verify_rows_chunked_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *const *record_planes,
                                          size_t n_planes, const uint16_t *masked, size_t B, size_t M, size_t chunk_rows, void *workspace, size_t workspace_bytes,
                                          uint64_t *verdict, void *stream) {
    if (!record_planes) return fail(HRX_ERR_ARG, "NULL buffer");
    return verify_chunked_device_any(ctx, layout, chars, stride, lens, nullptr, record_planes, n_planes, 0, masked, 0, B, M, chunk_rows, workspace, workspace_bytes,
                                     verdict, stream);
}

int hrx_verify_rows_chunked_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                                 const uint16_t *masked, size_t msk_pitch, size_t B, size_t M, size_t chunk_rows, uint64_t *verdict) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (B == 0) return HRX_OK;
    VerifyArgs a;
    if (int rc = check_verify_args(ctx, layout, chars, stride, lens, records, nullptr, 0, rec_pitch, masked, msk_pitch, B, M, verdict, false, a)) return rc;
    uint32_t C;
    if (int rc = resolve_chunk_rows(ctx, B, M, chunk_rows, C)) return rc;
    unsigned threads;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (int rc = verify_image_ready(ctx)) return rc;
        threads = ctx->host_threads > 0 ? (unsigned)ctx->host_threads : 0u;
    }
    a.image = ctx->verify_image.data();
    std::vector<uint32_t> summaries;      // (the device form's workspace; here the call's own)
    try {
        summaries.resize(verify_chunked_workspace_bytes(B, M, C) / 4);
    } catch (const std::bad_alloc &) {
        return fail(HRX_ERR_BOUNDS, "verify: no memory for the chunk summaries: use larger chunks");
    }
    verify_rows_chunked_host(a, C, summaries.data(), threads);
    return HRX_OK;
}

}  // extern "C"
