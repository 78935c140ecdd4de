// hrx_route_api.cpp — hrx_route_workspace_bytes / hrx_route_device / hrx_route_host / hrx_gather_to_position_major_device (include/hrx.h ROUTE): the step
// between "screen" and "prove" — the strings a match call kept, sorted into the circuit sizes the caller has proving keys for, and each group staged as
// witness input.  The device entries check their arguments and enqueue their launches (hrx_kernel_route.hip: three; hrx_kernel_ragged.hip: one) on the
// caller's stream: they allocate nothing, touch no context scratch and do not synchronise (no lock either: nothing of the context but its device is
// read).  The host entry is hrx_route_host.cpp behind the same argument rules.  DESIGN.md §14.
#include "hrx_ctx.hpp"

namespace hrx {
void route_host(const RouteIn &in, uint32_t *order, uint64_t *bucket_offsets);      // hrx_route_host.cpp
}
using namespace hrx;
static_assert(kRouteMaxBuckets == HRX_MAX_BUCKETS, "hrx_route.hpp and include/hrx.h");

// the argument rules both forms of route share, in the order the errors are reported; fills `in`
static int check_route_args(const uint64_t *status, uint32_t require_accept, const uint32_t *lens, const uint64_t *offsets, size_t B, const uint32_t *bounds,
                            size_t n_buckets, const uint32_t *order, const uint64_t *bucket_offsets, RouteIn &in) {
    if ((lens != nullptr) == (offsets != nullptr)) return fail(HRX_ERR_ARG, "exactly one of lens and offsets");
    if (!route_bounds_valid(bounds, n_buckets))
        return fail(HRX_ERR_ARG, "bounds: 1..HRX_MAX_BUCKETS of them, strictly increasing, the last one <= 2^24");
    if (B > 0xffffffffull) return fail(HRX_ERR_ARG, "batch too large");
    if (!bucket_offsets || (B && !order)) return fail(HRX_ERR_ARG, "NULL output");
    if (((uintptr_t)status & 7) || ((uintptr_t)offsets & 7) || ((uintptr_t)bucket_offsets & 7) || ((uintptr_t)lens & 3) || ((uintptr_t)order & 3))
        return fail(HRX_ERR_ARG, "status, offsets and bucket_offsets must be 8-byte aligned, lens and order 4-byte");
    in = RouteIn{};
    in.status = status; in.require_accept = require_accept; in.lens = lens; in.offsets = offsets; in.B = B;
    in.bounds.n = (uint32_t)n_buckets;
    for (size_t j = 0; j < n_buckets; ++j) in.bounds.v[j] = bounds[j];
    return HRX_OK;
}

extern "C" {

size_t hrx_route_workspace_bytes(size_t B) { return route_workspace_bytes(B); }

int hrx_route_device(hrx_ctx *ctx, const uint64_t *status, uint32_t require_accept, const uint32_t *lens, const uint64_t *offsets, size_t B,
                     const uint32_t *bounds, size_t n_buckets, uint32_t *order, uint64_t *bucket_offsets, void *workspace, size_t workspace_bytes,
                     void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    RouteArgs a{};
    if (int rc = check_route_args(status, require_accept, lens, offsets, B, bounds, n_buckets, order, bucket_offsets, a.in)) return rc;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < route_workspace_bytes(B))
        return fail(HRX_ERR_ARG, "workspace: 8-byte aligned, at least hrx_route_workspace_bytes(B) bytes");
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    a.order = order; a.bucket_offsets = bucket_offsets; a.ws = (uint64_t *)workspace;
    DeviceGuard guard;      // (stateless: no context scratch, no lock)
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_route(a, (hipStream_t)stream));
    return HRX_OK;
}

int hrx_route_host(const uint64_t *status, uint32_t require_accept, const uint32_t *lens, const uint64_t *offsets, size_t B, const uint32_t *bounds,
                   size_t n_buckets, uint32_t *order, uint64_t *bucket_offsets) {
    RouteIn in;
    if (int rc = check_route_args(status, require_accept, lens, offsets, B, bounds, n_buckets, order, bucket_offsets, in)) return rc;
    route_host(in, order, bucket_offsets);
    return HRX_OK;
}

int hrx_gather_to_position_major_device(hrx_ctx *ctx, int layout, const uint8_t *src, size_t src_stride, const uint32_t *lens, const uint64_t *offsets,
                                        size_t B, const uint32_t *sel, size_t n_sel, size_t stride, uint8_t *chars_pm, uint32_t *lens_out, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    const bool ragged = layout == HRX_LAYOUT_INPUT_RAGGED;
    if (!ragged && layout != HRX_LAYOUT_STRING_MAJOR) return fail(HRX_ERR_ARG, "layout must be HRX_LAYOUT_STRING_MAJOR or HRX_LAYOUT_INPUT_RAGGED");
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    if (n_sel == 0) return HRX_OK;
    if (!sel || !chars_pm || !lens_out || (B && (!src || (ragged ? !offsets : !lens)))) return fail(HRX_ERR_ARG, "NULL buffer");
    if (B > 0xffffffffull || n_sel > 0xffffffffull - 64 || stride / 16 > 0xffffffffull) return fail(HRX_ERR_ARG, "shape out of range");
    if ((stride & 15) || stride < 16 || ((uintptr_t)src & 15) || ((uintptr_t)chars_pm & 15) || ((uintptr_t)sel & 3) || ((uintptr_t)lens_out & 3) ||
        (ragged ? ((uintptr_t)offsets & 7) != 0 : (((uintptr_t)lens & 3) || (src_stride & 15))))
        return fail(HRX_ERR_ARG, "src and chars_pm must be 16-byte aligned, offsets 8-byte, lens, sel and lens_out 4-byte, stride % 16 == 0, stride >= 16, "
                                 "string-major src_stride % 16 == 0");
    DeviceGuard guard;      // (stateless: no context scratch, no lock)
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_gather_to_position_major(src, src_stride, ragged ? nullptr : lens, ragged ? offsets : nullptr, B, sel, n_sel, stride, chars_pm, lens_out,
                                            (hipStream_t)stream));
    return HRX_OK;
}

}  // extern "C"
