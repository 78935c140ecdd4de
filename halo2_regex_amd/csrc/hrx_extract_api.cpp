// hrx_extract_api.cpp — hrx_extract_workspace_bytes / hrx_extract_spans_device / hrx_extract_spans_host (include/hrx.h EXTRACT): the runs a match call
// reported -> an Arrow list<large_binary> column of the revealed bytes plus its run words.  The device entry checks its arguments and enqueues the four
// launches of hrx_kernel_extract.hip on the caller's stream: it allocates nothing, touches no context scratch and does not synchronise (no lock either:
// nothing of the context but its device is read).  The host entry is hrx_extract_host.cpp behind the same argument rules.  DESIGN.md §13.
#include "hrx_ctx.hpp"

namespace hrx {
void extract_host(const ExtractIn &in, const hrx_extract_out &out, int threads);      // hrx_extract_host.cpp
}
using namespace hrx;

// the argument rules both forms share, in the order the errors are reported
static int check_extract_args(int layout, bool host, const uint8_t *src, size_t stride, const uint64_t *offsets, size_t B, const uint64_t *status,
                              const uint32_t *span_counts, const uint64_t *spans, size_t max_spans, const hrx_extract_out *out) {
    const bool ragged = layout == HRX_LAYOUT_INPUT_RAGGED, pm = layout == HRX_LAYOUT_INPUT_POSITION_MAJOR;
    if (host ? (layout != HRX_LAYOUT_STRING_MAJOR && !ragged) : (layout != HRX_LAYOUT_STRING_MAJOR && !ragged && !pm))
        return fail(HRX_ERR_ARG, host ? "layout must be HRX_LAYOUT_STRING_MAJOR or HRX_LAYOUT_INPUT_RAGGED"
                                      : "layout must be HRX_LAYOUT_STRING_MAJOR, HRX_LAYOUT_INPUT_POSITION_MAJOR or HRX_LAYOUT_INPUT_RAGGED");
    if (max_spans == 0 || max_spans > kMatchMaxSpans) return fail(HRX_ERR_ARG, "max_spans must be in 1..2^16");
    if (B > 0xffffffffull - 64) return fail(HRX_ERR_ARG, "batch too large");
    if (!out || !out->run_offsets || !out->byte_offsets || !out->totals || (out->runs_cap && !out->runs) || (out->values_cap && !out->values))
        return fail(HRX_ERR_ARG, "NULL output");
    if (B && (!src || !status || !span_counts || !spans || (ragged && !offsets))) return fail(HRX_ERR_ARG, "NULL buffer");
    if (((uintptr_t)out->run_offsets & 7) || ((uintptr_t)out->runs & 7) || ((uintptr_t)out->byte_offsets & 7) || ((uintptr_t)out->totals & 7) ||
        ((uintptr_t)status & 7) || ((uintptr_t)spans & 7) || ((uintptr_t)span_counts & 3) || (ragged && ((uintptr_t)offsets & 7)))
        return fail(HRX_ERR_ARG, "offsets, status, spans, run_offsets, runs, byte_offsets and totals must be 8-byte aligned, span_counts 4-byte");
    if (pm && (stride & 15)) return fail(HRX_ERR_ARG, "position-major input: stride % 16 == 0");
    if (!ragged && stride > (1u << 28)) return fail(HRX_ERR_ARG, "stride must be <= 2^28");
    return HRX_OK;
}

static ExtractIn extract_in(int layout, const uint8_t *src, size_t stride, const uint64_t *offsets, size_t B, const uint64_t *status,
                            const uint32_t *span_counts, const uint64_t *spans, size_t max_spans, uint32_t require_accept) {
    ExtractIn in{};
    in.layout = layout; in.src = src; in.stride = stride; in.offsets = offsets; in.B = B;
    in.status = status; in.span_counts = span_counts; in.spans = spans; in.max_spans = max_spans; in.require_accept = require_accept;
    return in;
}

extern "C" {

size_t hrx_extract_workspace_bytes(size_t B) { return extract_workspace_bytes(B); }

int hrx_extract_spans_device(hrx_ctx *ctx, int layout, const uint8_t *src, size_t stride, const uint64_t *offsets, size_t B,
                             const uint64_t *status, const uint32_t *span_counts, const uint64_t *spans, size_t max_spans,
                             uint32_t require_accept, const hrx_extract_out *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (int rc = check_extract_args(layout, false, src, stride, offsets, B, status, span_counts, spans, max_spans, out)) return rc;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < extract_workspace_bytes(B))
        return fail(HRX_ERR_ARG, "workspace: 8-byte aligned, at least hrx_extract_workspace_bytes(B) bytes");
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    ExtractArgs a{};
    a.in = extract_in(layout, src, stride, offsets, B, status, span_counts, spans, max_spans, require_accept);
    a.run_offsets = out->run_offsets; a.runs = out->runs; a.byte_offsets = out->byte_offsets; a.values = out->values; a.totals = out->totals;
    a.runs_cap = out->runs_cap; a.values_cap = out->values_cap;
    a.ws = (uint64_t *)workspace;
    DeviceGuard guard;      // (stateless: no context scratch, no lock)
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_extract(a, (hipStream_t)stream));
    return HRX_OK;
}

int hrx_extract_spans_host(int layout, const uint8_t *src, size_t stride, const uint64_t *offsets, size_t B, const uint64_t *status,
                           const uint32_t *span_counts, const uint64_t *spans, size_t max_spans, uint32_t require_accept,
                           const hrx_extract_out *out, int threads) {
    if (int rc = check_extract_args(layout, true, src, stride, offsets, B, status, span_counts, spans, max_spans, out)) return rc;
    int nt = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(nt, 1), B / 4096));      // a thread per 4096 strings at the most
    extract_host(extract_in(layout, src, stride, offsets, B, status, span_counts, spans, max_spans, require_accept), *out, nt);
    return HRX_OK;
}

}  // extern "C"
