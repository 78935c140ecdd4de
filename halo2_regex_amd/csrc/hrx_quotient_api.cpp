// hrx_quotient_api.cpp — hrx_fr_vanishing_inverse_device / _host / hrx_lookup_quotient_device / _host / hrx_ctx_lookup_quotient_plan (include/hrx.h LOOKUP
// QUOTIENT): the lookup argument's five constraints on the extended coset, folded into the quotient accumulator and divided by the vanishing polynomial.
// The rule is hrx_quotient.hpp's, the kernels hrx_kernel_quotient.hip, the host forms hrx_quotient_host.cpp.  The calls read nothing of the context but its
// device and its number of defs: stateless, no lock, their launches from the first call on.  DESIGN.md §24.
#include <initializer_list>

#include "hrx_ctx.hpp"
#include "hrx_kernel.hpp"
#include "hrx_lookup_run.hpp"  // LookupRun: the number of defs
#include "hrx_quotient.hpp"

namespace hrx {
void vanishing_inverse_host(const VanishArgs &a);                // hrx_quotient_host.cpp
void quotient_host(const QuotientArgs &a, unsigned threads);
}
using namespace hrx;

static int check_domain(unsigned k, unsigned ext_k) {
    if (k < 1 || ext_k <= k || ext_k - k > kQtMaxExtBits || ext_k > kNttMaxK) return fail(HRX_ERR_ARG, "k: at least 1; ext_k - k: 1 .. 6; ext_k: at most 24");
    return HRX_OK;
}

static int check_vanish_args(unsigned k, unsigned ext_k, const uint64_t *shift, uint64_t *t_inv, int flags, VanishArgs &a) {
    if (!t_inv) return fail(HRX_ERR_ARG, "NULL buffer");
    if (((uintptr_t)t_inv & 15) || ((uintptr_t)shift & 7)) return fail(HRX_ERR_ARG, "t_inv must be 16-byte aligned, shift 8-byte");
    if (flags & ~HRX_FR_CANONICAL) return fail(HRX_ERR_ARG, "unknown flag bits");
    if (int rc = check_domain(k, ext_k)) return rc;
    a = VanishArgs{shift, t_inv, k, ext_k, (flags & HRX_FR_CANONICAL) ? 1u : 0u};
    return HRX_OK;
}

// [p, p + cells x 32 bytes) and [q, ...) share a byte
static bool ranges_overlap(const void *p, size_t p_cells, const void *q, size_t q_cells) {
    const uintptr_t p0 = (uintptr_t)p, p1 = p0 + p_cells * 32u, q0 = (uintptr_t)q, q1 = q0 + q_cells * 32u;
    return p0 < q1 && q0 < p1;
}

// the argument rules both quotient forms share; fills `a`
static int check_quotient_args(const hrx_ctx *ctx, size_t b_count, unsigned k, unsigned ext_k, const uint64_t *a_ext, const uint64_t *ap_ext, const uint64_t *sp_ext,
                               const uint64_t *z_ext, size_t pitch, const uint64_t *s_ext, size_t s_pitch, size_t s_stride, const uint64_t *selectors,
                               size_t sel_pitch, const uint64_t *beta, const uint64_t *gamma, const uint64_t *y, size_t challenge_stride, const uint64_t *h_in,
                               uint64_t *h_out, size_t h_pitch, const uint64_t *t_inv, int flags, QuotientArgs &a) {
    if (!a_ext || !ap_ext || !sp_ext || !z_ext || !s_ext || !selectors || !beta || !gamma || !y || !h_out) return fail(HRX_ERR_ARG, "NULL buffer");
    if (flags & ~(HRX_FR_CANONICAL | HRX_QUOTIENT_DIVIDE)) return fail(HRX_ERR_ARG, "unknown flag bits");
    const bool divide = (flags & HRX_QUOTIENT_DIVIDE) != 0;
    if (divide && !t_inv) return fail(HRX_ERR_ARG, "HRX_QUOTIENT_DIVIDE needs t_inv");
    if (!divide) t_inv = nullptr;
    if (((uintptr_t)a_ext & 15) || ((uintptr_t)ap_ext & 15) || ((uintptr_t)sp_ext & 15) || ((uintptr_t)z_ext & 15) || ((uintptr_t)s_ext & 15) ||
        ((uintptr_t)selectors & 15) || ((uintptr_t)h_in & 15) || ((uintptr_t)h_out & 15) || ((uintptr_t)t_inv & 15) || ((uintptr_t)beta & 7) ||
        ((uintptr_t)gamma & 7) || ((uintptr_t)y & 7))
        return fail(HRX_ERR_ARG, "the cells must be 16-byte aligned, beta, gamma and y 8-byte");
    if (int rc = check_domain(k, ext_k)) return rc;
    if (s_stride != 0 && s_stride != 1) return fail(HRX_ERR_ARG, "s_stride: 1 (one table run per string) or 0 (one for the call)");
    if (challenge_stride != 0 && challenge_stride != 4) return fail(HRX_ERR_ARG, "challenge_stride: 4 (beta, gamma and y per string) or 0 (one set for the call)");
    const size_t N = (size_t)1 << ext_k;
    for (const size_t p : {pitch, s_pitch, sel_pitch, h_pitch})
        if ((p & 3) || p < N || p > 0xfffffffcull) return fail(HRX_ERR_ARG, "pitch, s_pitch, sel_pitch, h_pitch: multiples of 4 cells, at least 2^ext_k");
    LookupRun run;
    if (!defs_lookup_run(ctx->s, run) || run.D == 0) return fail(HRX_ERR_ARG, "lookup quotient: more defs than HRX_MAX_DEFS");
    const size_t ncols = 3 * (size_t)run.D, tiles = N > kQtTileCells ? N / kQtTileCells : 1;
    if (b_count > 0x7fffffffull / tiles) return fail(HRX_ERR_ARG, "more workgroups than a launch has: use a smaller window");
    if (ncols * b_count > ((size_t)1 << 56) / (pitch > s_pitch ? pitch : s_pitch)) return fail(HRX_ERR_ARG, "columns x pitch: more bytes than an address has");
    // h_out is the one buffer written: in place over h_in, apart from everything else read
    const size_t cells = (ncols * b_count - 1) * pitch + N, s_cells = (ncols * (s_stride ? b_count : 1) - 1) * s_pitch + N, h_cells = (b_count - 1) * h_pitch + N;
    if (h_in && h_in != h_out && ranges_overlap(h_out, h_cells, h_in, h_cells))
        return fail(HRX_ERR_ARG, "h_in and h_out overlap: the same buffer (in place), or apart");
    if (ranges_overlap(h_out, h_cells, a_ext, cells) || ranges_overlap(h_out, h_cells, ap_ext, cells) || ranges_overlap(h_out, h_cells, sp_ext, cells) ||
        ranges_overlap(h_out, h_cells, z_ext, cells) || ranges_overlap(h_out, h_cells, s_ext, s_cells) ||
        ranges_overlap(h_out, h_cells, selectors, 2 * sel_pitch + N) || (t_inv && ranges_overlap(h_out, h_cells, t_inv, (size_t)1 << (ext_k - k))))
        return fail(HRX_ERR_ARG, "h_out overlaps an input");
    a = QuotientArgs{};
    a.a_ext = a_ext; a.ap_ext = ap_ext; a.sp_ext = sp_ext; a.z_ext = z_ext; a.s_ext = s_ext; a.selectors = selectors; a.beta = beta; a.gamma = gamma; a.y = y;
    a.h_in = h_in; a.h_out = h_out; a.t_inv = t_inv; a.pitch = pitch; a.s_pitch = s_pitch; a.sel_pitch = sel_pitch; a.h_pitch = h_pitch;
    a.b_count = (uint32_t)b_count; a.ncols = (uint32_t)ncols; a.k = k; a.ext_k = ext_k; a.s_stride = (uint32_t)s_stride;
    a.challenge_stride = (uint32_t)challenge_stride; a.canonical = (flags & HRX_FR_CANONICAL) ? 1u : 0u; a.divide = divide ? 1u : 0u;
    return HRX_OK;
}

extern "C" {

int hrx_fr_vanishing_inverse_device(hrx_ctx *ctx, unsigned k, unsigned ext_k, const uint64_t *shift, uint64_t *t_inv, int flags, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    VanishArgs a;
    if (int rc = check_vanish_args(k, ext_k, shift, t_inv, flags, a)) return rc;
    if (int rc = check_has_device(ctx)) return rc;
    DeviceGuard guard;      // (stateless: no context scratch, no lock)
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_vanishing_inverse(a, (hipStream_t)stream));
    return HRX_OK;
}

int hrx_fr_vanishing_inverse_host(hrx_ctx *ctx, unsigned k, unsigned ext_k, const uint64_t *shift, uint64_t *t_inv, int flags) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    VanishArgs a;
    if (int rc = check_vanish_args(k, ext_k, shift, t_inv, flags, a)) return rc;
    vanishing_inverse_host(a);
    return HRX_OK;
}

int hrx_lookup_quotient_device(hrx_ctx *ctx, size_t b_count, unsigned k, unsigned ext_k, const uint64_t *a_ext, const uint64_t *ap_ext, const uint64_t *sp_ext,
                               const uint64_t *z_ext, size_t pitch, const uint64_t *s_ext, size_t s_pitch, size_t s_stride, const uint64_t *selectors,
                               size_t sel_pitch, const uint64_t *beta, const uint64_t *gamma, const uint64_t *y, size_t challenge_stride, const uint64_t *h_in,
                               uint64_t *h_out, size_t h_pitch, const uint64_t *t_inv, int flags, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    QuotientArgs a;
    if (int rc = check_quotient_args(ctx, b_count, k, ext_k, a_ext, ap_ext, sp_ext, z_ext, pitch, s_ext, s_pitch, s_stride, selectors, sel_pitch, beta, gamma, y,
                                     challenge_stride, h_in, h_out, h_pitch, t_inv, flags, a))
        return rc;
    if (int rc = check_has_device(ctx)) return rc;
    DeviceGuard guard;      // (stateless: no context scratch, no lock)
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_lookup_quotient(a, (hipStream_t)stream));
    return HRX_OK;
}

int hrx_lookup_quotient_host(hrx_ctx *ctx, size_t b_count, unsigned k, unsigned ext_k, const uint64_t *a_ext, const uint64_t *ap_ext, const uint64_t *sp_ext,
                             const uint64_t *z_ext, size_t pitch, const uint64_t *s_ext, size_t s_pitch, size_t s_stride, const uint64_t *selectors,
                             size_t sel_pitch, const uint64_t *beta, const uint64_t *gamma, const uint64_t *y, size_t challenge_stride, const uint64_t *h_in,
                             uint64_t *h_out, size_t h_pitch, const uint64_t *t_inv, int flags) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (b_count == 0) return HRX_OK;
    QuotientArgs a;
    if (int rc = check_quotient_args(ctx, b_count, k, ext_k, a_ext, ap_ext, sp_ext, z_ext, pitch, s_ext, s_pitch, s_stride, selectors, sel_pitch, beta, gamma, y,
                                     challenge_stride, h_in, h_out, h_pitch, t_inv, flags, a))
        return rc;
    quotient_host(a, ctx_host_threads(ctx));
    return HRX_OK;
}

int hrx_ctx_lookup_quotient_plan(hrx_ctx *ctx, size_t b_count, unsigned ext_k, size_t *tile_cells, size_t *cells_per_lane) {
    (void)b_count;
    if (!ctx || !tile_cells || !cells_per_lane) return fail(HRX_ERR_ARG, "NULL argument");
    if (ext_k < 2 || ext_k > kNttMaxK) return fail(HRX_ERR_ARG, "ext_k: 2 .. 24");
    *tile_cells = kQtTileCells; *cells_per_lane = kQtCellsPerLane;
    return HRX_OK;
}

}  // extern "C"
