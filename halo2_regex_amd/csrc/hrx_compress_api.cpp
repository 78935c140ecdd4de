// hrx_compress_api.cpp — hrx_lookup_num_columns / hrx_lookup_compress_inputs_device / _device_planes / _host / hrx_lookup_compress_table_device / _host /
// hrx_fr_mul (include/hrx.h LOOKUP COMPRESS): the lookup tuples of the witness rows and the rows of the fixed tables folded with a challenge into field
// cells.  The rule is hrx_compress.hpp's, the kernels hrx_kernel_compress.hip, the host forms hrx_compress_host.cpp.  The calls over rows read no image of
// the tables (a def's dummy state travels in the arguments): one launch from the first call on.  The table calls read the context's flat tuple array, built
// from the rows RegexTableConfig::load assigns at the context's first call of this kind, under its lock, and for a device call uploaded then — one run of
// hrx_lookup_run.hpp's layout.  DESIGN.md §20.
#include "hrx_compress.hpp"
#include "hrx_ctx.hpp"
#include "hrx_kernel.hpp"

namespace hrx {
void compress_inputs_host(const CompressArgs &a, unsigned threads);          // hrx_compress_host.cpp
void compress_table_host(const CompressTableArgs &a, unsigned threads);
}
using namespace hrx;

static int check_theta(const uint64_t *theta, size_t theta_stride, const uint64_t *cells, int flags) {
    if (!theta || !cells) return fail(HRX_ERR_ARG, "NULL buffer");
    if (theta_stride != 0 && theta_stride != 4) return fail(HRX_ERR_ARG, "theta_stride: 4 (one challenge per string or run) or 0 (one for the call)");
    if (((uintptr_t)cells & 15) || ((uintptr_t)theta & 7)) return fail(HRX_ERR_ARG, "cells must be 16-byte aligned, theta 8-byte");
    if (flags & ~HRX_FR_CANONICAL) return fail(HRX_ERR_ARG, "unknown flag bits");
    return HRX_OK;
}

// the argument rules the forms over rows share: check_rows' (hrx_rows_api.cpp) for the rows (no masked rows), check_window's
static int check_compress_args(const hrx_ctx *ctx, const RowsCall &c, size_t b_begin, size_t b_count, const uint64_t *theta, size_t theta_stride, uint64_t *cells,
                               int flags, bool device, CompressArgs &a) {
    if (int rc = check_theta(theta, theta_stride, cells, flags)) return rc;
    if (int rc = check_window(c.B, b_begin, b_count)) return rc;
    a = CompressArgs{};
    if (int rc = check_rows(ctx, c, device, a)) return rc;
    if (a.D > HRX_MAX_DEFS) return fail(HRX_ERR_ARG, "more defs than HRX_MAX_DEFS");
    for (uint32_t d = 0; d < a.D; ++d) {
        const uint64_t dummy = ctx->s.defs[d].allstr.largest_state_val + 1;      // table.rs:67
        if (dummy > 0xffffu) return fail(HRX_ERR_BOUNDS, "lookup compress: a dummy state beyond 16 bits");
        a.dummy[d] = (uint16_t)dummy;
    }
    a.b_begin = (uint32_t)b_begin; a.b_count = (uint32_t)b_count;
    a.theta = theta; a.theta_stride = (uint32_t)theta_stride; a.canonical = (flags & HRX_FR_CANONICAL) ? 1u : 0u;
    a.cells = cells; a.col_cells = (uint64_t)b_count * c.M;
    return HRX_OK;
}

static int compress_device_any(hrx_ctx *ctx, const RowsCall &c, size_t b_begin, size_t b_count, const uint64_t *theta, size_t theta_stride, uint64_t *cells,
                               int flags, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    CompressArgs a;
    if (int rc = check_compress_args(ctx, c, b_begin, b_count, theta, theta_stride, cells, flags, true, a)) return rc;
    if (int rc = check_has_device(ctx)) return rc;
    DeviceGuard guard;      // (stateless: no context scratch, no image, no lock)
    HIP_TRY(guard.set(ctx->device));
    const size_t M = c.M, tiles_of_string = (M + kCzRowsPerTile - 1) / kCzRowsPerTile;
    a.tiles = (uint32_t)std::min<size_t>(tiles_of_string, kCzMaxTiles);
    // one launch per 32768 strings (the grid's y dimension), as the field cells have it; every launch writes its slice of each column
    for (size_t done = 0; done < b_count; done += 32768) {
        const size_t nb = b_count - done < 32768 ? b_count - done : 32768;
        a.b_begin = (uint32_t)(b_begin + done); a.b_count = (uint32_t)nb;
        a.cells = cells + done * M * 4;
        a.theta = theta + done * theta_stride;
        HIP_TRY(launch_compress_inputs(a, (hipStream_t)stream));
    }
    return HRX_OK;
}

static int compress_image_host(hrx_ctx *ctx) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ctx_image_host(ctx, ctx->compress_img, build_compress_image, "lookup compress");
}
static int compress_image_device(hrx_ctx *ctx, void *stream) { return ctx_image_device(ctx, ctx->compress_img, build_compress_image, "lookup compress", stream); }

static int check_table_args(const uint64_t *theta, size_t theta_stride, size_t n_theta, uint64_t *cells, int flags, CompressTableArgs &a) {
    if (int rc = check_theta(theta, theta_stride, cells, flags)) return rc;
    if (n_theta > 0xffffu) return fail(HRX_ERR_ARG, "n_theta: at most 65535 runs a call");
    a = CompressTableArgs{};
    a.theta = theta; a.theta_stride = (uint32_t)theta_stride; a.n_theta = (uint32_t)n_theta; a.canonical = (flags & HRX_FR_CANONICAL) ? 1u : 0u;
    a.cells = cells;
    return HRX_OK;
}

extern "C" {

size_t hrx_lookup_num_columns(size_t D) { return 3 * D; }

void hrx_fr_mul(const uint64_t *a, const uint64_t *b, uint64_t *out) {
    if (!a || !b || !out) return;
    fr_store_cell(out, fr_mul(fr_load_cell(a), fr_load_cell(b)));
}

int hrx_lookup_compress_inputs_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                                      size_t B, size_t M, size_t b_begin, size_t b_count, const uint64_t *theta, size_t theta_stride, uint64_t *cells, int flags,
                                      void *stream) {
    return compress_device_any(ctx, RowsCall{layout, chars, stride, lens, records, nullptr, 0, rec_pitch, nullptr, 0, B, M}, b_begin, b_count, theta, theta_stride,
                               cells, flags, stream);
}

int hrx_lookup_compress_inputs_device_planes(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *const *record_planes,
                                             size_t n_planes, size_t B, size_t M, size_t b_begin, size_t b_count, const uint64_t *theta, size_t theta_stride,
                                             uint64_t *cells, int flags, void *stream) {
    if (!record_planes) return fail(HRX_ERR_ARG, "NULL buffer");
    return compress_device_any(ctx, RowsCall{layout, chars, stride, lens, nullptr, record_planes, n_planes, 0, nullptr, 0, B, M}, b_begin, b_count, theta,
                               theta_stride, cells, flags, stream);
}

int hrx_lookup_compress_inputs_host(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, const uint32_t *records, size_t rec_pitch,
                                    size_t B, size_t M, size_t b_begin, size_t b_count, const uint64_t *theta, size_t theta_stride, uint64_t *cells, int flags) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    CompressArgs a;
    const RowsCall c{layout, chars, stride, lens, records, nullptr, 0, rec_pitch, nullptr, 0, B, M};
    if (int rc = check_compress_args(ctx, c, b_begin, b_count, theta, theta_stride, cells, flags, false, a)) return rc;
    compress_inputs_host(a, ctx_host_threads(ctx));
    return HRX_OK;
}

int hrx_lookup_compress_table_device(hrx_ctx *ctx, const uint64_t *theta, size_t theta_stride, size_t n_theta, uint64_t *cells, int flags, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (n_theta == 0) return HRX_OK;
    CompressTableArgs a;
    if (int rc = check_table_args(theta, theta_stride, n_theta, cells, flags, a)) return rc;
    if (int rc = check_has_device(ctx)) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    if (int rc = compress_image_device(ctx, stream)) return rc;
    a.image = (const uint32_t *)ctx->compress_img.dev.p;
    a.W = (uint32_t)(ctx->compress_img.host.size() / 4);
    HIP_TRY(launch_compress_table(a, (hipStream_t)stream));
    return HRX_OK;
}

int hrx_lookup_compress_table_host(hrx_ctx *ctx, const uint64_t *theta, size_t theta_stride, size_t n_theta, uint64_t *cells, int flags) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (n_theta == 0) return HRX_OK;
    CompressTableArgs a;
    if (int rc = check_table_args(theta, theta_stride, n_theta, cells, flags, a)) return rc;
    if (int rc = compress_image_host(ctx)) return rc;
    a.image = ctx->compress_img.host.data();     // (never rebuilt once it is there)
    a.W = (uint32_t)(ctx->compress_img.host.size() / 4);
    compress_table_host(a, ctx_host_threads(ctx));
    return HRX_OK;
}

}  // extern "C"
