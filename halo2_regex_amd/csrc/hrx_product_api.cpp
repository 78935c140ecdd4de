// hrx_product_api.cpp — hrx_lookup_invert_table_device / _host / hrx_lookup_invert_workspace_bytes / hrx_lookup_product_device / _host /
// hrx_ctx_lookup_product_plan (include/hrx.h LOOKUP PRODUCT): the inverse tables 1 / (S + c) and the grand product Z of halo2's lookup argument.  The rule is
// hrx_product.hpp's, the kernels hrx_kernel_product.hip, the host forms hrx_product_host.cpp.  The calls read no image of the tables (the runs' layout is
// hrx_lookup_run.hpp's over the defs' row counts: defs_lookup_run of hrx_rows_api.cpp): the device forms are their launches from the first call on,
// stateless, no lock.  DESIGN.md §22.
#include "hrx_ctx.hpp"
#include "hrx_kernel.hpp"
#include "hrx_permute.hpp"     // kPmMaxRows: n_rows' bounds are LOOKUP PERMUTE's
#include "hrx_product.hpp"

namespace hrx {
void invert_table_host(const InvertArgs &a, unsigned threads);   // hrx_product_host.cpp
void product_host(const ProductArgs &a, unsigned threads);
}
using namespace hrx;

static const char *const kNoRun = "lookup product: more defs than HRX_MAX_DEFS, or more bins than a u32 run indexes";

// the words of a run that are bins: the last def's end
static uint32_t run_bins(const LookupRun &run) {
    const LookupRun::Def &R = run.def[run.D - 1u];
    return R.off + (uint32_t)lookup_run_def_words(R.n_tr, R.n_ep);
}

static int check_invert_args(const hrx_ctx *ctx, const uint64_t *table_cells, size_t n_runs, const uint64_t *shift, size_t shift_stride, uint64_t *inv_cells,
                             int flags, InvertArgs &a) {
    if (!table_cells || !shift || !inv_cells) return fail(HRX_ERR_ARG, "NULL buffer");
    if (shift_stride != 0 && shift_stride != 4) return fail(HRX_ERR_ARG, "shift_stride: 4 (one shift per run) or 0 (one for the call)");
    if (((uintptr_t)table_cells & 15) || ((uintptr_t)inv_cells & 15) || ((uintptr_t)shift & 7))
        return fail(HRX_ERR_ARG, "the table and the inverse cells must be 16-byte aligned, shift 8-byte");
    if (flags & ~HRX_FR_CANONICAL) return fail(HRX_ERR_ARG, "unknown flag bits");
    if (n_runs > 0x7fffffffull) return fail(HRX_ERR_ARG, "more runs than a call takes");
    LookupRun run;
    if (!defs_lookup_run(ctx->s, run) || run.D == 0) return fail(HRX_ERR_ARG, kNoRun);
    a = InvertArgs{};
    a.table = table_cells; a.shift = shift; a.shift_stride = (uint32_t)shift_stride; a.n_runs = (uint32_t)n_runs; a.W = run.W; a.bins = run_bins(run);
    a.canonical = (flags & HRX_FR_CANONICAL) ? 1u : 0u; a.inv = inv_cells;
    return HRX_OK;
}

// the argument rules both product forms share; fills `a`
static int check_product_args(const hrx_ctx *ctx, const uint32_t *lens, size_t M, size_t b_begin, size_t b_count, const uint64_t *in_cells, const uint32_t *a_idx,
                              const uint32_t *s_idx, size_t n_rows, size_t idx_pitch, const uint64_t *table_cells, const uint64_t *inv_beta,
                              const uint64_t *inv_gamma, size_t table_stride, const uint64_t *beta, const uint64_t *gamma, size_t challenge_stride, uint64_t *z,
                              size_t z_pitch, uint32_t *open, int flags, ProductArgs &a) {
    if (!lens || !in_cells || !a_idx || !s_idx || !table_cells || !inv_beta || !inv_gamma || !beta || !gamma || !z) return fail(HRX_ERR_ARG, "NULL buffer");
    if (((uintptr_t)in_cells & 15) || ((uintptr_t)a_idx & 15) || ((uintptr_t)s_idx & 15) || ((uintptr_t)table_cells & 15) || ((uintptr_t)inv_beta & 15) ||
        ((uintptr_t)inv_gamma & 15) || ((uintptr_t)z & 15) || ((uintptr_t)beta & 7) || ((uintptr_t)gamma & 7) || ((uintptr_t)lens & 3) || ((uintptr_t)open & 3))
        return fail(HRX_ERR_ARG, "the cells, the index columns and the tables must be 16-byte aligned, beta and gamma 8-byte, lens and open 4-byte");
    if (flags & ~HRX_FR_CANONICAL) return fail(HRX_ERR_ARG, "unknown flag bits");
    if (challenge_stride != 0 && challenge_stride != 4) return fail(HRX_ERR_ARG, "challenge_stride: 4 (beta and gamma per string) or 0 (one pair for the call)");
    a = ProductArgs{};
    LookupRun run;
    if (!defs_lookup_run(ctx->s, run) || run.D == 0) return fail(HRX_ERR_ARG, kNoRun);
    const size_t W = run.W, ncols = 3 * (size_t)run.D;
    for (uint32_t c = 0; c < ncols; ++c) a.col[c] = lookup_run_col(run, c);
    if (open && ncols > kPdMaxOpenCols) return fail(HRX_ERR_ARG, "open: a word has bits for 32 lookups (10 defs)");
    if (table_stride != 0 && table_stride != 4 * W) return fail(HRX_ERR_ARG, "table_stride: 4 W (one run per string) or 0 (one for the call)");
    if (n_rows < run.T_max || n_rows > kPmMaxRows) return fail(HRX_ERR_ARG, "n_rows: at least the rows of every table of the defs, at most 2^24");
    if (M == 0 || M > kPmMaxRows) return fail(HRX_ERR_ARG, "M: 1 .. 2^24");
    if (idx_pitch == 0) idx_pitch = (n_rows + 3) & ~(size_t)3;
    if (idx_pitch < n_rows || (idx_pitch & 3) || idx_pitch > 0xfffffffcull) return fail(HRX_ERR_ARG, "idx_pitch: a multiple of 4, at least n_rows (0: n_rows rounded up)");
    if (z_pitch == 0) z_pitch = (n_rows + 4) & ~(size_t)3;
    if (z_pitch <= n_rows || (z_pitch & 3) || z_pitch > 0xfffffffcull) return fail(HRX_ERR_ARG, "z_pitch: a multiple of 4 above n_rows (0: n_rows + 1 rounded up)");
    if (b_count > 0x7fffffffull || b_begin > 0xffffffffull - b_count) return fail(HRX_ERR_ARG, "more strings than a call takes: use a smaller window");
    if ((uint64_t)b_count * ncols > 0x7fffffffull) return fail(HRX_ERR_ARG, "more workgroups than a launch has: use a smaller window");
    a.lens = lens; a.M = (uint32_t)M; a.b_begin = (uint32_t)b_begin; a.b_count = (uint32_t)b_count; a.n_rows = (uint32_t)n_rows; a.idx_pitch = (uint32_t)idx_pitch;
    a.z_pitch = (uint32_t)z_pitch; a.W = (uint32_t)W; a.ncols = (uint32_t)ncols; a.canonical = (flags & HRX_FR_CANONICAL) ? 1u : 0u;
    a.in_cells = in_cells; a.a_idx = a_idx; a.s_idx = s_idx; a.table = table_cells; a.inv_beta = inv_beta; a.inv_gamma = inv_gamma;
    a.table_stride = (uint32_t)table_stride; a.beta = beta; a.gamma = gamma; a.challenge_stride = (uint32_t)challenge_stride; a.z = z; a.open = open;
    return HRX_OK;
}

extern "C" {

size_t hrx_lookup_invert_workspace_bytes(const hrx_defs *defs, size_t n_runs) {
    (void)defs; (void)n_runs;
    return 0;       // this build inverts a run inside one workgroup (kPdInvertLaunches == 1): no totals travel between launches
}

int hrx_lookup_invert_table_device(hrx_ctx *ctx, const uint64_t *table_cells, size_t n_runs, const uint64_t *shift, size_t shift_stride, uint64_t *inv_cells,
                                   int flags, void *workspace, size_t workspace_bytes, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (n_runs == 0) return HRX_OK;
    InvertArgs a;
    if (int rc = check_invert_args(ctx, table_cells, n_runs, shift, shift_stride, inv_cells, flags, a)) return rc;
    const size_t need = hrx_lookup_invert_workspace_bytes(nullptr, n_runs);
    if (((uintptr_t)workspace & 255) || (need && (!workspace || workspace_bytes < need)))
        return fail(HRX_ERR_ARG, "workspace: 256-byte aligned device memory of at least hrx_lookup_invert_workspace_bytes bytes");
    if (int rc = check_has_device(ctx)) return rc;
    DeviceGuard guard;      // (stateless: no context scratch, no image, no lock)
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_lookup_invert(a, (hipStream_t)stream));
    return HRX_OK;
}

int hrx_lookup_invert_table_host(hrx_ctx *ctx, const uint64_t *table_cells, size_t n_runs, const uint64_t *shift, size_t shift_stride, uint64_t *inv_cells,
                                 int flags) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (n_runs == 0) return HRX_OK;
    InvertArgs a;
    if (int rc = check_invert_args(ctx, table_cells, n_runs, shift, shift_stride, inv_cells, flags, a)) return rc;
    invert_table_host(a, ctx_host_threads(ctx));
    return HRX_OK;
}

int hrx_ctx_lookup_product_plan(hrx_ctx *ctx, size_t b_count, size_t n_rows, size_t *tile_rows, size_t *rows_per_lane) {
    (void)b_count; (void)n_rows;
    if (!ctx || !tile_rows || !rows_per_lane) return fail(HRX_ERR_ARG, "NULL argument");
    *tile_rows = kPdTileRows; *rows_per_lane = kPdRowsPerLane;
    return HRX_OK;
}

int hrx_lookup_product_device(hrx_ctx *ctx, const uint32_t *lens, size_t M, size_t b_begin, size_t b_count, const uint64_t *in_cells, const uint32_t *a_idx,
                              const uint32_t *s_idx, size_t n_rows, size_t idx_pitch, const uint64_t *table_cells, const uint64_t *inv_beta,
                              const uint64_t *inv_gamma, size_t table_stride, const uint64_t *beta, const uint64_t *gamma, size_t challenge_stride, uint64_t *z,
                              size_t z_pitch, uint32_t *open, int flags, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    ProductArgs a;
    if (int rc = check_product_args(ctx, lens, M, b_begin, b_count, in_cells, a_idx, s_idx, n_rows, idx_pitch, table_cells, inv_beta, inv_gamma, table_stride, beta,
                                    gamma, challenge_stride, z, z_pitch, open, flags, a))
        return rc;
    if (int rc = check_has_device(ctx)) return rc;
    DeviceGuard guard;      // (stateless: no context scratch, no image, no lock)
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_lookup_product(a, (hipStream_t)stream));
    return HRX_OK;
}

int hrx_lookup_product_host(hrx_ctx *ctx, const uint32_t *lens, size_t M, size_t b_begin, size_t b_count, const uint64_t *in_cells, const uint32_t *a_idx,
                            const uint32_t *s_idx, size_t n_rows, size_t idx_pitch, const uint64_t *table_cells, const uint64_t *inv_beta,
                            const uint64_t *inv_gamma, size_t table_stride, const uint64_t *beta, const uint64_t *gamma, size_t challenge_stride, uint64_t *z,
                            size_t z_pitch, uint32_t *open, int flags) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    ProductArgs a;
    if (int rc = check_product_args(ctx, lens, M, b_begin, b_count, in_cells, a_idx, s_idx, n_rows, idx_pitch, table_cells, inv_beta, inv_gamma, table_stride, beta,
                                    gamma, challenge_stride, z, z_pitch, open, flags, a))
        return rc;
    product_host(a, ctx_host_threads(ctx));
    return HRX_OK;
}

}  // extern "C"
