// hrx_permute_api.cpp — hrx_lookup_permute_device / _host / hrx_lookup_permute_workspace_bytes / hrx_ctx_lookup_permute_plan (include/hrx.h LOOKUP
// PERMUTE): the permuted columns A', S' of halo2's lookup argument out of the counts, as indices into a string's run and as cells of the compressed table.
// The rule is hrx_permute.hpp's, the kernels hrx_kernel_permute.hip, the host form hrx_permute_host.cpp.  The calls read no image of the tables (the runs'
// layout is hrx_lookup_run.hpp's over the defs' row counts: defs_lookup_run of hrx_rows_api.cpp): the device form is its launches from the first call on,
// stateless, no lock.  DESIGN.md §21.
#include "hrx_ctx.hpp"
#include "hrx_kernel.hpp"
#include "hrx_permute.hpp"

namespace hrx {
void permute_host(const PermuteArgs &a, unsigned threads);      // hrx_permute_host.cpp
}
using namespace hrx;

static const char *const kNoRun = "lookup permute: more defs than HRX_MAX_DEFS, or more bins than a u32 run indexes";

// the argument rules both forms share; fills `a` (but the plan and the workspace) and T_max
static int check_permute_args(const hrx_ctx *ctx, const uint32_t *counts, size_t b_count, size_t n_rows, size_t pitch, uint32_t *a_idx, uint32_t *s_idx,
                              const uint64_t *table_cells, size_t table_stride, uint64_t *a_cells, uint64_t *s_cells, uint32_t *overflow, PermuteArgs &a,
                              size_t &T_max) {
    if (!counts) return fail(HRX_ERR_ARG, "NULL buffer");
    if ((a_idx != nullptr) != (s_idx != nullptr)) return fail(HRX_ERR_ARG, "a_idx and s_idx: both or neither");
    if ((a_cells != nullptr) != (s_cells != nullptr) || (a_cells != nullptr) != (table_cells != nullptr))
        return fail(HRX_ERR_ARG, "table_cells, a_cells and s_cells: all three or none");
    if (!a_idx && !a_cells) return fail(HRX_ERR_ARG, "no output: the index pair, the cell pair or both");
    if (((uintptr_t)counts & 15) || ((uintptr_t)a_idx & 15) || ((uintptr_t)s_idx & 15) || ((uintptr_t)table_cells & 15) || ((uintptr_t)a_cells & 15) ||
        ((uintptr_t)s_cells & 15) || ((uintptr_t)overflow & 3))
        return fail(HRX_ERR_ARG, "counts, the index columns, the table and the cells must be 16-byte aligned, overflow 4-byte");
    a = PermuteArgs{};
    LookupRun run;
    if (!defs_lookup_run(ctx->s, run)) return fail(HRX_ERR_ARG, kNoRun);
    const size_t W = run.W, ncols = 3 * (size_t)run.D;
    T_max = run.T_max;
    for (uint32_t c = 0; c < ncols; ++c) a.col[c] = lookup_run_col(run, c);
    if (overflow && ncols > kPmMaxOverflowCols) return fail(HRX_ERR_ARG, "overflow: a word has bits for 32 lookups (10 defs)");
    if (table_cells && table_stride != 0 && table_stride != 4 * W) return fail(HRX_ERR_ARG, "table_stride: 4 W (one run per string) or 0 (one for the call)");
    if (n_rows < T_max || n_rows > kPmMaxRows) return fail(HRX_ERR_ARG, "n_rows: at least the rows of every table of the defs, at most 2^24");
    if (pitch == 0) pitch = (n_rows + 3) & ~(size_t)3;
    if (pitch < n_rows || (pitch & 3) || pitch > 0xfffffffcull) return fail(HRX_ERR_ARG, "pitch: a multiple of 4, at least n_rows (0: n_rows rounded up)");
    if (b_count > 0x7fffffffull) return fail(HRX_ERR_ARG, "more strings than a call takes: use a smaller window");
    a.counts = counts; a.b_count = (uint32_t)b_count; a.n_rows = (uint32_t)n_rows; a.pitch = (uint32_t)pitch; a.W = (uint32_t)W; a.ncols = (uint32_t)ncols;
    a.a_idx = a_idx; a.s_idx = s_idx; a.table = table_cells; a.table_stride = (uint32_t)table_stride; a.a_cells = a_cells; a.s_cells = s_cells;
    a.overflow = overflow;
    return HRX_OK;
}

extern "C" {

size_t hrx_lookup_permute_workspace_bytes(const hrx_defs *defs, size_t b_count, size_t n_rows) {
    if (!defs || defs->s.defs.empty()) return 0;
    LookupRun run;
    return defs_lookup_run(defs->s, run) ? plan_permute(run.T_max, run.W, 3 * (size_t)run.D, b_count, n_rows, 0).workspace_bytes : 0;
}

int hrx_ctx_lookup_permute_plan(hrx_ctx *ctx, size_t b_count, size_t n_rows, size_t *tile_rows, size_t *chunk_rows, size_t *group_rows, size_t *groups) {
    if (!ctx || !tile_rows || !chunk_rows || !group_rows || !groups) return fail(HRX_ERR_ARG, "NULL argument");
    LookupRun run;
    if (!defs_lookup_run(ctx->s, run)) return fail(HRX_ERR_ARG, kNoRun);
    const PermutePlan p = plan_permute(run.T_max, run.W, 3 * (size_t)run.D, b_count, n_rows, ctx->num_cus);
    *tile_rows = p.tile_rows; *chunk_rows = p.chunk_rows; *group_rows = p.group_rows; *groups = p.groups;
    return HRX_OK;
}

int hrx_lookup_permute_device(hrx_ctx *ctx, const uint32_t *counts, size_t b_count, size_t n_rows, size_t pitch, uint32_t *a_idx, uint32_t *s_idx,
                              const uint64_t *table_cells, size_t table_stride, uint64_t *a_cells, uint64_t *s_cells, uint32_t *overflow, void *workspace,
                              size_t workspace_bytes, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    PermuteArgs a;
    size_t T_max;
    if (int rc = check_permute_args(ctx, counts, b_count, n_rows, pitch, a_idx, s_idx, table_cells, table_stride, a_cells, s_cells, overflow, a, T_max)) return rc;
    const PermutePlan p = plan_permute(T_max, a.W, a.ncols, b_count, n_rows, ctx->num_cus);
    if (p.workspace_bytes) {
        if (!workspace || ((uintptr_t)workspace & 255) || workspace_bytes < p.workspace_bytes)
            return fail(HRX_ERR_ARG, "workspace: 256-byte aligned device memory of at least hrx_lookup_permute_workspace_bytes bytes");
        a.zrows = (uint32_t *)workspace;
    }
    if ((uint64_t)b_count * a.ncols * p.groups > 0x7fffffffull) return fail(HRX_ERR_ARG, "more workgroups than a launch has: use a smaller window");
    a.groups = p.groups; a.group_rows = p.group_rows;
    if (int rc = check_has_device(ctx)) return rc;
    DeviceGuard guard;      // (stateless: no context scratch, no image, no lock)
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_lookup_permute(a, (hipStream_t)stream));
    return HRX_OK;
}

int hrx_lookup_permute_host(hrx_ctx *ctx, const uint32_t *counts, size_t b_count, size_t n_rows, size_t pitch, uint32_t *a_idx, uint32_t *s_idx,
                            const uint64_t *table_cells, size_t table_stride, uint64_t *a_cells, uint64_t *s_cells, uint32_t *overflow) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    PermuteArgs a;
    size_t T_max;
    if (int rc = check_permute_args(ctx, counts, b_count, n_rows, pitch, a_idx, s_idx, table_cells, table_stride, a_cells, s_cells, overflow, a, T_max)) return rc;
    permute_host(a, ctx_host_threads(ctx));
    return HRX_OK;
}

}  // extern "C"
