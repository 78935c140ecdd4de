// hrx_rows_api.cpp — what the entry points that READ witness rows share (hrx_verify_api.cpp, hrx_lookup_api.cpp, hrx_compress_api.cpp, the field cells of
// hrx_api.cpp): the argument rules of the row forms (hrx_rows.hpp) over a caller's RowsCall, a config's run of the lookup argument (hrx_lookup_run.hpp, for
// those three and hrx_permute_api.cpp), and a context's cached image of its circuit's table rows, in host memory and on its device.
#include "hrx_ctx.hpp"
#include "hrx_lookup_run.hpp"
#include "hrx_verify.hpp"      // VerifyDefRows

using namespace hrx;

int check_rows_layout(int layout) {
    if (!rows_layout_known(layout)) return fail(HRX_ERR_ARG, "unknown layout");
    return HRX_OK;
}

int check_rows_planes(const hrx_ctx *ctx, int layout, const uint32_t *const *planes, size_t n_planes) {
    const size_t Dn = ctx->s.defs.size();
    if (!(layout & HRX_LAYOUT_POSITION_MAJOR)) return fail(HRX_ERR_ARG, "record planes are a position-major layout");
    if (!planes || !(n_planes == Dn || (Dn == 1 && n_planes == 2)) || n_planes > kRowsMaxPlanes)
        return fail(HRX_ERR_ARG, "record planes: one buffer per def (at most eight; one def: one buffer or two row stripes)");
    for (size_t d = 0; d < n_planes; ++d)
        if (!planes[d]) return fail(HRX_ERR_ARG, "NULL plane");
    return HRX_OK;
}

int check_rows(const hrx_ctx *ctx, const RowsCall &c, bool device, RowsIn &a) {
    const size_t M = c.M, rec_pitch = c.rec_pitch ? c.rec_pitch : M, msk_pitch = c.msk_pitch ? c.msk_pitch : M;
    if (!c.chars || !c.lens || (!c.records && !c.planes)) return fail(HRX_ERR_ARG, "NULL buffer");
    if (M == 0 || M > kRowsMaxRows || c.B > 0xffffffffull - 64) return fail(HRX_ERR_ARG, "shape out of range");
    if (int rc = check_rows_layout(c.layout)) return rc;
    if (c.planes)
        if (int rc = check_rows_planes(ctx, c.layout, c.planes, c.n_planes)) return rc;
    if (!(c.layout & HRX_LAYOUT_POSITION_MAJOR) && (rec_pitch < M || msk_pitch < M)) return fail(HRX_ERR_ARG, "rec_pitch or msk_pitch < M");
    if ((uintptr_t)c.lens & 3) return fail(HRX_ERR_ARG, "lens must be 4-byte aligned");
    if (device) {     // the kernels read 16-byte chunks, quads and octets: the alignment of the witness entry points that wrote the rows
        bool ok = !(c.stride & 15) && !((uintptr_t)c.chars & 15) && !((uintptr_t)c.records & 15) && !((uintptr_t)c.masked & 15);
        for (size_t d = 0; c.planes && d < c.n_planes; ++d) ok = ok && !((uintptr_t)c.planes[d] & 15);
        if (!ok) return fail(HRX_ERR_ARG, "chars, records, masked and every record plane must be 16-byte aligned, stride % 16 == 0");
    } else if (((uintptr_t)c.records & 3) || ((uintptr_t)c.masked & 1) || ((c.layout & HRX_LAYOUT_INPUT_POSITION_MAJOR) && (c.stride & 15))) {
        return fail(HRX_ERR_ARG, "records must be 4-byte aligned, masked 2-byte; position-major input: stride % 16 == 0");
    }
    const size_t Dn = ctx->s.defs.size();
    a = RowsIn{};
    a.chars = c.chars; a.stride = c.stride; a.lens = c.lens; a.records = c.planes ? nullptr : c.records; a.masked = c.masked;
    for (size_t d = 0; c.planes && d < c.n_planes; ++d) a.planes[d] = c.planes[d];
    a.n_stripes = c.planes && c.n_planes == 2 * Dn ? 2u : 1u;
    a.B = (uint32_t)c.B; a.M = (uint32_t)M; a.D = (uint32_t)Dn; a.layout = (uint32_t)c.layout;
    a.rec_pitch = rec_pitch; a.msk_pitch = msk_pitch;
    return HRX_OK;
}

int check_window(size_t B, size_t b_begin, size_t b_count) {
    if (b_begin > B || b_count > B - b_begin) return fail(HRX_ERR_ARG, "string range outside the batch");
    return HRX_OK;
}

int check_has_device(const hrx_ctx *ctx) {
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    return HRX_OK;
}

unsigned ctx_host_threads(hrx_ctx *ctx) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ctx->host_threads > 0 ? (unsigned)ctx->host_threads : 0u;
}

bool defs_lookup_run(const DefsSet &s, LookupRun &run) {
    return lookup_run_fill(run, s.defs.size(), [&s](size_t d, size_t &t, size_t &e) {
        t = table_transition_rows(s, d, nullptr, 0);
        e = table_endpoint_rows(s, d, nullptr, 0);
    });
}

int ctx_image_host(hrx_ctx *ctx, CtxImage &im, CtxImageBuilder build, const char *noun) {
    if (!im.host.empty()) return HRX_OK;
    // the rows RegexTableConfig::load assigns, per def
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
    if (!build(rows.data(), D, img)) return fail(HRX_ERR_BOUNDS, std::string(noun) + ": the config's table rows do not fit the image's dense tables");
    im.host = std::move(img);
    return HRX_OK;
}

int ctx_image_device(hrx_ctx *ctx, CtxImage &im, CtxImageBuilder build, const char *noun, void *stream) {
    if (im.dev.p) return HRX_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing((hipStream_t)stream, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail(HRX_ERR_STATE, std::string(noun) + ": the context's image is built and uploaded at its first call, not inside a stream capture");
    if (int rc = ctx_image_host(ctx, im, build, noun)) return rc;
    DevBuf tab;
    HIP_TRY(tab.reserve(im.host.size() * 4));
    const hipError_t e = hipMemcpy(tab.p, im.host.data(), im.host.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        tab.release();
        return fail(HRX_ERR_HIP, std::string(noun) + ": image upload: " + hipGetErrorString(e));
    }
    im.dev = tab;
    return HRX_OK;
}
