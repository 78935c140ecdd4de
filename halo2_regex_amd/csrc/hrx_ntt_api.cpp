// hrx_ntt_api.cpp — hrx_fr_ntt_workspace_bytes / hrx_fr_ntt_prepare_device / hrx_fr_ntt_device / hrx_fr_ntt_host / hrx_ctx_fr_ntt_plan / hrx_fr_sub
// (include/hrx.h FR NTT): the transform of size 2^k over columns of bn256::Fr cells.  The rule is hrx_ntt.hpp's, the kernels hrx_kernel_ntt.hip, the host
// form hrx_ntt_host.cpp.  The calls read nothing of the context but its device: stateless, no lock, their launches from the first call on.  DESIGN.md §23.
#include "hrx_ctx.hpp"
#include "hrx_kernel.hpp"
#include "hrx_ntt.hpp"

namespace hrx {
void ntt_host(const NttArgs &a, unsigned threads);   // hrx_ntt_host.cpp
}
using namespace hrx;

// the argument rules both forms share; fills `a`
static int check_ntt_args(const uint64_t *in, size_t in_pitch, uint64_t *out, size_t out_pitch, size_t n_cols, unsigned k, size_t n_in, const uint64_t *shift,
                          int flags, NttArgs &a) {
    if (!in || !out) return fail(HRX_ERR_ARG, "NULL buffer");
    if (((uintptr_t)in & 15) || ((uintptr_t)out & 15) || ((uintptr_t)shift & 7)) return fail(HRX_ERR_ARG, "the cells must be 16-byte aligned, shift 8-byte");
    if (flags & ~(HRX_FR_CANONICAL | HRX_NTT_INVERSE)) return fail(HRX_ERR_ARG, "unknown flag bits");
    if (k < 1 || k > kNttMaxK) return fail(HRX_ERR_ARG, "k: 1 .. 24");
    const size_t n = (size_t)1 << k;
    if (n_in < 1 || n_in > n) return fail(HRX_ERR_ARG, "n_in: 1 .. 2^k");
    if ((in_pitch & 3) || in_pitch < n_in || in_pitch > 0xfffffffcull) return fail(HRX_ERR_ARG, "in_pitch: a multiple of 4 cells, at least n_in");
    if ((out_pitch & 3) || out_pitch < n || out_pitch > 0xfffffffcull) return fail(HRX_ERR_ARG, "out_pitch: a multiple of 4 cells, at least 2^k");
    // the permuting launch has the most workgroups: 2^(k - 8) a column
    if (n_cols > 0x7fffffffull || (k > 2u * kNttPermuteBits && n_cols > (0x7fffffffull >> (k - 2u * kNttPermuteBits))))
        return fail(HRX_ERR_ARG, "more workgroups than a launch has: transform fewer columns per call");
    if (n_cols > ((size_t)1 << 56) / (in_pitch > out_pitch ? in_pitch : out_pitch)) return fail(HRX_ERR_ARG, "columns x pitch: more bytes than an address has");
    if (!((const void *)in == (const void *)out && in_pitch == out_pitch)) {      // in place, or apart
        const uintptr_t i0 = (uintptr_t)in, i1 = i0 + ((n_cols - 1) * in_pitch + n_in) * 32u, o0 = (uintptr_t)out, o1 = o0 + ((n_cols - 1) * out_pitch + n) * 32u;
        if (i0 < o1 && o0 < i1) return fail(HRX_ERR_ARG, "in and out overlap: the same buffer with the same pitch (in place), or apart");
    }
    a = NttArgs{};
    a.in = in; a.out = out; a.in_pitch = in_pitch; a.out_pitch = out_pitch; a.n_cols = (uint32_t)n_cols; a.k = k; a.n_in = (uint32_t)n_in;
    a.inverse = (flags & HRX_NTT_INVERSE) ? 1u : 0u; a.canonical = (flags & HRX_FR_CANONICAL) ? 1u : 0u; a.shift = shift;
    return HRX_OK;
}

static int check_ntt_workspace(unsigned k, const void *workspace, size_t workspace_bytes) {
    if (k < 1 || k > kNttMaxK) return fail(HRX_ERR_ARG, "k: 1 .. 24");
    if (!workspace || ((uintptr_t)workspace & 255) || workspace_bytes < ntt_workspace_bytes(k))
        return fail(HRX_ERR_ARG, "workspace: 256-byte aligned device memory of at least hrx_fr_ntt_workspace_bytes(k) bytes");
    return HRX_OK;
}

extern "C" {

size_t hrx_fr_ntt_workspace_bytes(unsigned k) { return k >= 1 && k <= kNttMaxK ? ntt_workspace_bytes(k) : 0; }

int hrx_fr_ntt_prepare_device(hrx_ctx *ctx, unsigned k, void *workspace, size_t workspace_bytes, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (int rc = check_ntt_workspace(k, workspace, workspace_bytes)) return rc;
    if (int rc = check_has_device(ctx)) return rc;
    DeviceGuard guard;      // (stateless: no context scratch, no lock)
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_ntt_prepare(k, (uint32_t *)workspace, (hipStream_t)stream));
    return HRX_OK;
}

int hrx_fr_ntt_device(hrx_ctx *ctx, const uint64_t *in, size_t in_pitch, uint64_t *out, size_t out_pitch, size_t n_cols, unsigned k, size_t n_in,
                      const uint64_t *shift, int flags, const void *workspace, size_t workspace_bytes, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (n_cols == 0) return HRX_OK;
    NttArgs a;
    if (int rc = check_ntt_args(in, in_pitch, out, out_pitch, n_cols, k, n_in, shift, flags, a)) return rc;
    if (int rc = check_ntt_workspace(k, workspace, workspace_bytes)) return rc;
    if (int rc = check_has_device(ctx)) return rc;
    a.ws = (const uint32_t *)workspace;
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_ntt(a, ctx->device, (hipStream_t)stream));
    return HRX_OK;
}

int hrx_fr_ntt_host(hrx_ctx *ctx, const uint64_t *in, size_t in_pitch, uint64_t *out, size_t out_pitch, size_t n_cols, unsigned k, size_t n_in,
                    const uint64_t *shift, int flags) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (n_cols == 0) return HRX_OK;
    NttArgs a;
    if (int rc = check_ntt_args(in, in_pitch, out, out_pitch, n_cols, k, n_in, shift, flags, a)) return rc;
    ntt_host(a, ctx_host_threads(ctx));
    return HRX_OK;
}

int hrx_ctx_fr_ntt_plan(hrx_ctx *ctx, size_t n_cols, unsigned k, size_t *n_passes, size_t *pass_bits, size_t *cols_per_group) {
    (void)n_cols;
    if (!ctx || !n_passes || !pass_bits || !cols_per_group) return fail(HRX_ERR_ARG, "NULL argument");
    if (k < 1 || k > kNttMaxK) return fail(HRX_ERR_ARG, "k: 1 .. 24");
    const NttPlan p = ntt_plan(k);
    *n_passes = p.n_passes; *cols_per_group = p.cols_per_group;
    for (uint32_t j = 0; j < kNttMaxPasses; ++j) pass_bits[j] = p.pass_bits[j];
    return HRX_OK;
}

void hrx_fr_sub(const uint64_t *a, const uint64_t *b, uint64_t *out) {
    if (!a || !b || !out) return;
    fr_store_cell(out, fr_sub(fr_challenge(a), fr_challenge(b)));
}

}  // extern "C"
