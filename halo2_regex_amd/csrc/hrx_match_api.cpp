// hrx_match_api.cpp — hrx_match_batch_device / hrx_match_batch_host and their _ragged forms: the status word and the revealed runs of every string,
// without the witness rows (include/hrx.h MATCH, RAGGED).  The fused kernel where plan_match_launch allows it (hrx_kernel_match.hip padded,
// hrx_kernel_ragged.hip ragged), "via rows" otherwise: the position-major witness launch (launch_batch) slice by slice into context scratch, then
// the masked rows' runs.  The two input forms share the argument rules, the fused arguments, the via-rows driver (plan_via_rows, via_rows_scratch,
// match_via_rows: a form brings only the step that stages a slice's input) and the host entries' copy-out; they differ in the staging step and in
// how a host entry cuts its chunks.  DESIGN.md §11, §12.
// hrx_match_selected_device / _host (include/hrx.h SELECTED): the same two routes over an index array — the fused selected kernel, or via
// rows with an indexed staging step and a scan that scatters slot s of a slice to string sel[k0 + s]; the host entry packs the selected strings of a
// chunk back to back and runs the ragged chunk path on them.
#include "hrx_ctx.hpp"
#include "hrx_host_walk.hpp"
#include "hrx_lane.h"
#include "hrx_match_wide.h"

using namespace hrx;

// the argument rules both input forms share, in the order the errors are reported; the entry's own part: its input pointers (in_null), its
// 4- or 8-byte aligned one (in_misaligned) and the text of the alignment error
static int check_common_args(bool in_null, bool in_misaligned, const char *align_msg, size_t B, size_t M, const uint64_t *status,
                             const uint32_t *span_counts, const uint64_t *spans, size_t max_spans) {
    if (M == 0 || M > (1u << 24)) return fail(HRX_ERR_ARG, "max_chars_size must be in 1..2^24");
    if (B > 0xffffffffull - 64) return fail(HRX_ERR_ARG, "batch too large");
    if (max_spans > kMatchMaxSpans) return fail(HRX_ERR_ARG, "max_spans must be <= 2^16");
    if (B == 0) return HRX_OK;
    if (in_null || !status) return fail(HRX_ERR_ARG, "NULL buffer");
    if (max_spans == 0 && spans) return fail(HRX_ERR_ARG, "spans must be NULL when max_spans == 0");
    if (max_spans && (!spans || !span_counts)) return fail(HRX_ERR_ARG, "span_counts and spans are needed when max_spans > 0");
    if (((uintptr_t)status & 7) || ((uintptr_t)span_counts & 7) || ((uintptr_t)spans & 7) || in_misaligned) return fail(HRX_ERR_ARG, align_msg);
    return HRX_OK;
}
static int check_match_args(const uint8_t *chars, const uint32_t *lens, size_t B, size_t M, const uint64_t *status, const uint32_t *span_counts,
                            const uint64_t *spans, size_t max_spans) {
    return check_common_args(!chars || !lens, (uintptr_t)lens & 3, "status, span_counts and spans must be 8-byte aligned", B, M, status, span_counts, spans, max_spans);
}
// RAGGED input (include/hrx.h RAGGED; hrx_kernel_ragged.hip): string b is values + (offsets[b] - base), offsets[b + 1] - offsets[b] bytes
static int check_ragged_args(const uint8_t *values, const uint64_t *offsets, size_t B, size_t M, const uint64_t *status, const uint32_t *span_counts,
                             const uint64_t *spans, size_t max_spans) {
    return check_common_args(!values || !offsets, (uintptr_t)offsets & 7, "offsets, status, span_counts and spans must be 8-byte aligned", B, M, status, span_counts,
                             spans, max_spans);
}

// the planner's view of a context's config for the match entry points (describe and launch agree by construction)
static WitnessArgs match_args_of(const DefsSet &s, uint32_t dbg, int layout, size_t B, size_t M) {
    WitnessArgs a = witness_args_of(s, host_images(s));
    a.layout = (uint32_t)layout; a.B = (uint32_t)B; a.M = (uint32_t)M;
    if (!s.groups.empty()) a.D = 0u;     // (a multi-pass config always goes via rows)
    a.debug = dbg;
    return a;
}

// what a context's switches say about the match route: kDbgMatchViaRows, HRX_OPT_MATCH_FUSED_WIDE (none: the context-free describe)
struct MatchSwitches {
    bool via_rows, fused_wide;
};
static MatchSwitches switches_of(const hrx_ctx *ctx) { return MatchSwitches{ctx->match_via_rows, ctx->match_fused_wide}; }

// the one decision: the fused-wide walk where the option and plan_match_wide allow it, else plan_match_launch
static bool match_plan(const DefsSet &s, uint32_t dbg, const MatchSwitches &sw, int layout, size_t B, size_t M, int num_cus, MatchPlan &p) {
    if (plan_match_wide(s, dbg, sw.via_rows, sw.fused_wide, layout, B, M, num_cus, p)) return true;
    return plan_match_launch(match_args_of(s, dbg, layout, B, M), num_cus, sw.via_rows, p);
}

// the fused kernels' arguments but for the input (the entry's own: stride, lens, in_pm / offsets, base)
static MatchArgs fused_args(const hrx_ctx *ctx, const MatchPlan &p, const uint8_t *chars, size_t B, size_t M, uint64_t *status, uint32_t *span_counts,
                            uint64_t *spans, size_t max_spans) {
    MatchArgs m{};
    m.chars = chars; m.B = (uint32_t)B; m.M = (uint32_t)M; m.D = (uint32_t)ctx->s.defs.size(); m.max_spans = (uint32_t)max_spans;
    m.table_image = ctx->d_table; m.half_image = ctx->d_half; m.table_bytes = (uint32_t)p.lds_bytes;
    m.status = status; m.span_counts = span_counts; m.spans = spans;
    for (uint32_t d = 0; d < m.D; ++d) m.dc[d] = ctx->s.consts[d];
    return m;
}

// the fused-wide kernel's arguments (p.wide; hrx_match_wide.h)
static MatchWideArgs wide_args(const hrx_ctx *ctx, const MatchPlan &p, size_t B, size_t M, uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans) {
    MatchWideArgs w{};
    w.cw_image = (const uint8_t *)ctx->d_cw.p; w.image_bytes = (uint32_t)p.lds_bytes; w.cw_lut_off = ctx->s.cw_lut_off;
    w.B = (uint32_t)B; w.M = (uint32_t)M; w.D = (uint32_t)ctx->s.defs.size(); w.max_spans = (uint32_t)max_spans;
    w.status = status; w.span_counts = span_counts; w.spans = spans;
    for (uint32_t d = 0; d < w.D; ++d) w.dc[d] = ctx->s.cw_consts[d];
    return w;
}

// ---- "via rows".  Strings per slice: the witness rows of a slice, and `extra` staged bytes per string, fit the scratch; slices of more than one
// block are whole blocks.  0: not even one string's rows fit
static size_t via_rows_slice(size_t B, size_t M, size_t D, size_t extra) {
    const size_t per = ((M + 3) / 4) * 4 * D * 4 + ((M + 7) / 8) * 8 * 2 + extra;
    size_t n = kMatchScratchBytes / per;
    if (n == 0) return 0;
    if (n >= kPmBlock) n = n / kPmBlock * kPmBlock;
    return std::min(n, B);
}

// how a via-rows call cuts and stages its batch: the launch and the describe functions both read it here
struct ViaRows {
    size_t slice;       // strings per slice
    size_t stride;      // of the staged string-major input (ragged: round_up(M, 16); gather: the caller's)
    bool ragged;        // a staging kernel makes every slice (string-major input + lens, counted in the slice size): ragged_slice_kernel, or
    bool selected;      // selected_slice_kernel over either source, the slice's status words by slot in scratch and a scattering scan
    bool gather;        // slices inside a block of position-major input: pm_input_slice_kernel makes its strings string-major first
    int layout;         // of the witness launch
};
static ViaRows plan_via_rows(int layout, size_t stride, size_t B, size_t M, size_t D, bool selected = false) {
    ViaRows v{};
    v.selected = selected;
    v.ragged = layout == HRX_LAYOUT_INPUT_RAGGED || selected;
    v.stride = v.ragged ? (M + 15) & ~(size_t)15 : stride;
    v.slice = via_rows_slice(B, M, D, v.ragged ? v.stride + 4 : 0);
    const bool in_pm = layout == HRX_LAYOUT_INPUT_POSITION_MAJOR;
    v.gather = in_pm && v.slice < B && v.slice < kPmBlock;
    v.layout = HRX_LAYOUT_POSITION_MAJOR | (in_pm && !v.gather ? HRX_LAYOUT_INPUT_POSITION_MAJOR : 0);
    return v;
}

// The scratch of a via-rows call, ready for use on stream st.  It is this context's: allocated at first use (not inside a capture), and a launch on
// another stream first waits for the one that used it last (not possible inside a capture)
static int via_rows_scratch(hrx_ctx *ctx, const ViaRows &v, size_t M, hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(st, &cap));
    const bool capturing = cap != hipStreamCaptureStatusNone;
    if (v.slice == 0) return fail(HRX_ERR_BOUNDS, "match via rows: one string's witness rows exceed the 768 MiB scratch");
    const size_t D = ctx->s.defs.size(), noct = (M + 7) / 8, nquad = (M + 3) / 4;
    const size_t rec_bytes = nquad * 4 * D * 4 * v.slice, msk_bytes = noct * 8 * 2 * v.slice;
    const size_t chr_bytes = v.ragged || v.gather ? v.slice * v.stride : 0, len_bytes = v.ragged ? v.slice * 4 : 0;
    const size_t sta_bytes = v.selected ? v.slice * 8 : 0;
    if (rec_bytes > ctx->match_rec.cap || msk_bytes > ctx->match_msk.cap || chr_bytes > ctx->match_chars.cap || len_bytes > ctx->match_lens.cap ||
        sta_bytes > ctx->match_status.cap) {
        if (capturing) return fail(HRX_ERR_STATE, "match via rows: the context's scratch is allocated at first use, not inside a stream capture");
        HIP_TRY(hipDeviceSynchronize());     // (the buffers may be in use by earlier launches)
        HIP_TRY(ctx->match_rec.reserve(rec_bytes));
        HIP_TRY(ctx->match_msk.reserve(msk_bytes));
        HIP_TRY(ctx->match_chars.reserve(chr_bytes));
        HIP_TRY(ctx->match_lens.reserve(len_bytes));
        HIP_TRY(ctx->match_status.reserve(sta_bytes));
    }
    if (ctx->match_used && ctx->match_stream != st) {
        if (capturing) return fail(HRX_ERR_STATE, "match via rows: the scratch was last used on another stream");
        HIP_TRY(hipStreamSynchronize(ctx->match_stream));
    }
    ctx->match_used = true;
    ctx->match_stream = st;
    return HRX_OK;
}

// slice by slice: stage(b0, n, chars, lens) gives the input of strings [b0, b0 + n) as the witness launch reads it (v.layout, v.stride), then the
// position-major witness launch into the scratch and the runs of its masked rows.  scatter (a selected call: B slots, sel = the whole selection, the
// caller's outputs): the launch's status words go to scratch by slot and the scan writes slot b0 + s at index sel[b0 + s]
template <class Stage>
static int match_via_rows(hrx_ctx *ctx, const ViaRows &v, size_t B, size_t M, uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans,
                          hipStream_t st, const Stage &stage, const SpanScatter *scatter = nullptr) {
    if (int rc = via_rows_scratch(ctx, v, M, st)) return rc;      // first: it may allocate the buffers read below
    MatchArgs m{};
    m.M = (uint32_t)M; m.max_spans = (uint32_t)max_spans; m.masked = (const uint16_t *)ctx->match_msk.p;
    for (size_t b0 = 0; b0 < B; b0 += v.slice) {
        const size_t n = std::min(v.slice, B - b0);
        const uint8_t *c = nullptr;
        const uint32_t *lens = nullptr;
        if (int rc = stage(b0, n, c, lens)) return rc;
        uint64_t *const slice_status = scatter ? (uint64_t *)ctx->match_status.p : status + b0;
        if (int rc = launch_batch(ctx, c, v.stride, lens, n, M, (uint32_t *)ctx->match_rec.p, (uint16_t *)ctx->match_msk.p, slice_status, st, 0, 0, v.layout)) return rc;
        if (scatter) {
            m.B = (uint32_t)n; m.status = slice_status;
            SpanScatter o = *scatter;
            o.sel += b0;
            HIP_TRY(launch_spans_from_masked_selected(m, o, st));
        } else if (max_spans || span_counts) {
            m.B = (uint32_t)n; m.status = status + b0;
            m.span_counts = span_counts ? span_counts + b0 : nullptr; m.spans = spans ? spans + b0 * max_spans : nullptr;
            HIP_TRY(launch_spans_from_masked(m, st));
        }
    }
    return HRX_OK;
}

// the device part (device pointers; ctx->mu held, the device selected)
static int match_device_locked(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B, size_t M,
                               uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, hipStream_t st) {
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    if (layout != HRX_LAYOUT_STRING_MAJOR && layout != HRX_LAYOUT_INPUT_POSITION_MAJOR)
        return fail(HRX_ERR_ARG, "layout must be HRX_LAYOUT_STRING_MAJOR or HRX_LAYOUT_INPUT_POSITION_MAJOR");
    if ((stride & 15) || stride < 16 || ((uintptr_t)chars & 15))
        return fail(HRX_ERR_ARG, "chars must be 16-byte aligned with stride % 16 == 0 and stride >= 16");
    if (B == 0) return HRX_OK;
    MatchPlan p;
    if (!match_plan(ctx->s, ctx->debug, switches_of(ctx), layout, B, M, ctx->num_cus, p)) return fail(HRX_ERR_BOUNDS, "no match launch fits");
    if (p.wide) {
        HIP_TRY(launch_match_wide(wide_args(ctx, p, B, M, status, span_counts, spans, max_spans), SelectedSrc{chars, nullptr, lens, stride}, 0, nullptr, 0, p, ctx->num_cus, st));
        return HRX_OK;
    }
    if (p.fused) {
        MatchArgs m = fused_args(ctx, p, chars, B, M, status, span_counts, spans, max_spans);
        m.stride = stride; m.lens = lens; m.in_pm = layout == HRX_LAYOUT_INPUT_POSITION_MAJOR ? 1u : 0u;
        HIP_TRY(launch_match_lane(m, p, st));
        return HRX_OK;
    }
    const ViaRows v = plan_via_rows(layout, stride, B, M, ctx->s.defs.size());
    return match_via_rows(ctx, v, B, M, status, span_counts, spans, max_spans, st, [&](size_t b0, size_t n, const uint8_t *&c, const uint32_t *&l) -> int {
        c = chars + b0 * stride;      // (position-major input: whole blocks, b0 % kPmBlock == 0)
        l = lens + b0;
        if (v.gather) {
            HIP_TRY(launch_pm_input_slice(chars, stride, B, b0, n, (uint8_t *)ctx->match_chars.p, st));
            c = (const uint8_t *)ctx->match_chars.p;
        }
        return HRX_OK;
    });
}

// the device part of the ragged match (device pointers; ctx->mu held, the device selected)
static int match_ragged_device_locked(hrx_ctx *ctx, const uint8_t *values, const uint64_t *offsets, uint64_t base, size_t B, size_t M,
                                      uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, hipStream_t st) {
    if (B == 0) return HRX_OK;
    MatchPlan p;
    if (!match_plan(ctx->s, ctx->debug, switches_of(ctx), HRX_LAYOUT_STRING_MAJOR, B, M, ctx->num_cus, p)) return fail(HRX_ERR_BOUNDS, "no match launch fits");
    if (p.wide) {
        HIP_TRY(launch_match_wide(wide_args(ctx, p, B, M, status, span_counts, spans, max_spans), SelectedSrc{values, offsets, nullptr, 0}, base, nullptr, 0, p, ctx->num_cus, st));
        return HRX_OK;
    }
    if (p.fused) {
        RaggedMatchArgs r{};
        r.m = fused_args(ctx, p, values, B, M, status, span_counts, spans, max_spans);
        r.offsets = offsets; r.base = base;
        HIP_TRY(launch_match_ragged(r, p, ctx->num_cus, st));
        return HRX_OK;
    }
    const ViaRows v = plan_via_rows(HRX_LAYOUT_INPUT_RAGGED, 0, B, M, ctx->s.defs.size());
    return match_via_rows(ctx, v, B, M, status, span_counts, spans, max_spans, st, [&](size_t b0, size_t n, const uint8_t *&c, const uint32_t *&l) -> int {
        c = (const uint8_t *)ctx->match_chars.p;
        l = (const uint32_t *)ctx->match_lens.p;
        HIP_TRY(launch_ragged_slice(values, offsets, base, b0, n, (uint32_t)M, v.stride, (uint8_t *)ctx->match_chars.p, (uint32_t *)ctx->match_lens.p, st));
        return HRX_OK;
    });
}

// SELECTED (include/hrx.h): the argument rules of both entries in the order the errors are reported; the device entry's alignment rules come before its
// device check, so a host-only context reports them too
static int check_selected_args(int layout, const uint8_t *src, size_t src_stride, const uint32_t *lens, const uint64_t *offsets, size_t B, const uint32_t *sel,
                               size_t n_sel, size_t M, const uint64_t *status, const uint32_t *span_counts, const uint64_t *spans, size_t max_spans, bool device) {
    const bool ragged = layout == HRX_LAYOUT_INPUT_RAGGED;
    if (!ragged && layout != HRX_LAYOUT_STRING_MAJOR) return fail(HRX_ERR_ARG, "layout must be HRX_LAYOUT_STRING_MAJOR or HRX_LAYOUT_INPUT_RAGGED");
    if (n_sel > 0xffffffffull - 64) return fail(HRX_ERR_ARG, "selection too large");
    if (int rc = check_common_args(!src || (ragged ? !offsets : !lens), ragged ? ((uintptr_t)offsets & 7) != 0 : ((uintptr_t)lens & 3) != 0,
                                   "offsets, status, span_counts and spans must be 8-byte aligned, lens and sel 4-byte", B, M, status, span_counts, spans, max_spans))
        return rc;
    if (n_sel && !sel) return fail(HRX_ERR_ARG, "NULL sel");
    if ((uintptr_t)sel & 3) return fail(HRX_ERR_ARG, "offsets, status, span_counts and spans must be 8-byte aligned, lens and sel 4-byte");
    if (device && B && n_sel) {
        if ((uintptr_t)src & 15) return fail(HRX_ERR_ARG, "src must be 16-byte aligned");
        if (!ragged && ((src_stride & 15) || src_stride < 16)) return fail(HRX_ERR_ARG, "string-major src_stride % 16 == 0 and src_stride >= 16");
    }
    return HRX_OK;
}

// the device part of the selected match (device pointers; ctx->mu held, the device selected)
static int match_selected_device_locked(hrx_ctx *ctx, const SelectedSrc &src, size_t B, const uint32_t *sel, size_t n_sel, size_t M, uint64_t *status,
                                        uint32_t *span_counts, uint64_t *spans, size_t max_spans, hipStream_t st) {
    if (B == 0 || n_sel == 0) return HRX_OK;
    MatchPlan p;
    if (!match_plan(ctx->s, ctx->debug, switches_of(ctx), HRX_LAYOUT_STRING_MAJOR, n_sel, M, ctx->num_cus, p)) return fail(HRX_ERR_BOUNDS, "no match launch fits");
    if (p.wide) {
        HIP_TRY(launch_match_wide(wide_args(ctx, p, B, M, status, span_counts, spans, max_spans), src, 0, sel, n_sel, p, ctx->num_cus, st));
        return HRX_OK;
    }
    if (p.fused) {
        const MatchArgs m = fused_args(ctx, p, src.src, B, M, status, span_counts, spans, max_spans);
        HIP_TRY(launch_match_selected(m, src, sel, n_sel, p, ctx->num_cus, st));
        return HRX_OK;
    }
    const ViaRows v = plan_via_rows(HRX_LAYOUT_INPUT_RAGGED, 0, n_sel, M, ctx->s.defs.size(), true);
    const SpanScatter scatter{sel, (uint32_t)B, status, span_counts, spans};
    return match_via_rows(ctx, v, n_sel, M, nullptr, span_counts, spans, max_spans, st, [&](size_t k0, size_t n, const uint8_t *&c, const uint32_t *&l) -> int {
        c = (const uint8_t *)ctx->match_chars.p;
        l = (const uint32_t *)ctx->match_lens.p;
        HIP_TRY(launch_selected_slice(src, B, sel, k0, n, (uint32_t)M, v.stride, (uint8_t *)ctx->match_chars.p, (uint32_t *)ctx->match_lens.p, st));
        return HRX_OK;
    }, &scatter);
}

// the host entry points' device buffers for the results of a chunk of n strings (d_counts / d_spans: NULL where nothing is to come back) ...
static int host_result_bufs(hrx_ctx *ctx, size_t n, bool want_counts, size_t max_spans, uint32_t *&d_counts, uint64_t *&d_spans) {
    HIP_TRY(ctx->status.reserve(8 * n));
    HIP_TRY(ctx->match_counts.reserve(4 * n + 8));
    if (max_spans) HIP_TRY(ctx->match_spans.reserve(8 * n * max_spans));
    d_counts = (want_counts || max_spans) ? (uint32_t *)ctx->match_counts.p : nullptr;
    d_spans = max_spans ? (uint64_t *)ctx->match_spans.p : nullptr;
    return HRX_OK;
}
// ... and their way back: strings [b0, b0 + n) of the caller's arrays, complete when this returns
static int host_results_out(hrx_ctx *ctx, size_t b0, size_t n, uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans,
                            const uint32_t *d_counts, const uint64_t *d_spans, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(status + b0, ctx->status.p, 8 * n, hipMemcpyDeviceToHost, st));
    if (span_counts) HIP_TRY(hipMemcpyAsync(span_counts + b0, d_counts, 4 * n, hipMemcpyDeviceToHost, st));
    if (max_spans) HIP_TRY(hipMemcpyAsync(spans + b0 * max_spans, d_spans, 8 * n * max_spans, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return HRX_OK;
}

extern "C" {

int hrx_match_batch_device(hrx_ctx *ctx, int layout, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B, size_t M,
                           uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (int rc = check_match_args(chars, lens, B, M, status, span_counts, spans, max_spans)) return rc;
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    return match_device_locked(ctx, layout, chars, stride, lens, B, M, status, span_counts, spans, max_spans, (hipStream_t)stream);
}

int hrx_match_batch_host(hrx_ctx *ctx, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B, size_t M,
                         uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (int rc = check_match_args(chars, lens, B, M, status, span_counts, spans, max_spans)) return rc;
    if (B == 0) return HRX_OK;
    for (size_t b = 0; b < B; ++b)
        if (lens[b] <= M && lens[b] > stride) return fail(HRX_ERR_ARG, "a string is longer than the stride");
    if (ctx->device == HRX_DEVICE_NONE) {     // the native host walk, no row written
        const size_t threads = std::max<size_t>(1, std::min<size_t>(ctx->host_threads > 0 ? (size_t)ctx->host_threads : std::thread::hardware_concurrency(), B * M / 8192));
        host_match_batch(ctx->s, chars, stride, lens, B, M, status, span_counts, spans, max_spans, (int)threads);
        return HRX_OK;
    }
    // through the device: chunk by chunk in, match, out on the context's stream; only status / counts / spans come back
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    const size_t dstride = (stride + 15) & ~(size_t)15;
    size_t cb = std::max<size_t>(1024, ((size_t)64 << 20) / std::max<size_t>(1, dstride));    // ~64 MiB of input per chunk
    cb = std::min(cb, B);
    HIP_TRY(ctx->chars.reserve(dstride * cb + 16));
    HIP_TRY(ctx->lens.reserve(4 * cb));
    uint32_t *d_counts;
    uint64_t *d_spans;
    if (int rc = host_result_bufs(ctx, cb, span_counts != nullptr, max_spans, d_counts, d_spans)) return rc;
    hipStream_t st = ctx->stream;
    for (size_t b0 = 0; b0 < B; b0 += cb) {
        const size_t n = std::min(cb, B - b0);
        if (dstride != stride) HIP_TRY(hipMemsetAsync(ctx->chars.p, 0, dstride * n, st));
        HIP_TRY(hipMemcpy2DAsync(ctx->chars.p, dstride, chars + b0 * stride, stride, stride, n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->lens.p, lens + b0, 4 * n, hipMemcpyHostToDevice, st));
        if (int rc = match_device_locked(ctx, HRX_LAYOUT_STRING_MAJOR, (const uint8_t *)ctx->chars.p, dstride, (const uint32_t *)ctx->lens.p, n, M,
                                         (uint64_t *)ctx->status.p, d_counts, d_spans, max_spans, st))
            return rc;
        if (int rc = host_results_out(ctx, b0, n, status, span_counts, spans, max_spans, d_counts, d_spans, st)) return rc;
    }
    return HRX_OK;
}

int hrx_match_batch_device_ragged(hrx_ctx *ctx, const uint8_t *values, const uint64_t *offsets, size_t B, size_t M,
                                  uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (int rc = check_ragged_args(values, offsets, B, M, status, span_counts, spans, max_spans)) return rc;
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    if ((uintptr_t)values & 15) return fail(HRX_ERR_ARG, "values must be 16-byte aligned");
    if (B == 0) return HRX_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    return match_ragged_device_locked(ctx, values, offsets, 0, B, M, status, span_counts, spans, max_spans, (hipStream_t)stream);
}

int hrx_match_batch_host_ragged(hrx_ctx *ctx, const uint8_t *values, const uint64_t *offsets, size_t B, size_t M,
                                uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (int rc = check_ragged_args(values, offsets, B, M, status, span_counts, spans, max_spans)) return rc;
    if (B == 0) return HRX_OK;
    if (ctx->device == HRX_DEVICE_NONE) {     // the native host walk, no row written
        const size_t bytes = offsets[B] >= offsets[0] ? (size_t)(offsets[B] - offsets[0]) : 0;
        const size_t threads = std::max<size_t>(1, std::min<size_t>(ctx->host_threads > 0 ? (size_t)ctx->host_threads : std::thread::hardware_concurrency(),
                                                                    std::max<size_t>(bytes, B) / 8192));
        host_match_batch_ragged(ctx->s, values, offsets, B, M, status, span_counts, spans, max_spans, (int)threads);
        return HRX_OK;
    }
    // through the device: chunks of whole strings whose bytes span ~64 MiB; a chunk copies its one byte range (from the aligned 16 bytes its first
    // byte is in, so every string keeps its alignment) and its offsets as they are (the kernel subtracts the range's start); only status / counts /
    // spans come back.  Strings with decreasing offsets or longer than M are read by nobody and do not widen a range.
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    const size_t kSpan = (size_t)64 << 20;
    const size_t max_n = std::max<size_t>(1, std::min<size_t>((size_t)1 << 20, kSpan / (8 * max_spans + 12)));
    hipStream_t st = ctx->stream;
    for (size_t b0 = 0; b0 < B;) {
        uint64_t lo = UINT64_MAX, hi = 0;
        size_t b1 = b0;
        for (; b1 < B && b1 - b0 < max_n; ++b1) {
            const uint64_t o0 = offsets[b1], o1 = offsets[b1 + 1];
            if (o1 < o0 || o1 - o0 > M || o1 == o0) continue;
            const uint64_t nlo = std::min(lo, o0 & ~(uint64_t)15), nhi = std::max(hi, o1);
            if (b1 > b0 && nhi - nlo > kSpan) break;
            lo = nlo; hi = nhi;
        }
        const size_t n = b1 - b0;
        if (lo > hi) lo = hi = 0;          // (no byte to read in this chunk)
        const size_t bytes = (size_t)(hi - lo);
        HIP_TRY(ctx->chars.reserve(((bytes + 15) & ~(size_t)15) + 16));
        HIP_TRY(ctx->lens.reserve(8 * (n + 1)));
        uint32_t *d_counts;
        uint64_t *d_spans;
        if (int rc = host_result_bufs(ctx, n, span_counts != nullptr, max_spans, d_counts, d_spans)) return rc;
        if (bytes) HIP_TRY(hipMemcpyAsync(ctx->chars.p, values + lo, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->lens.p, offsets + b0, 8 * (n + 1), hipMemcpyHostToDevice, st));
        if (int rc = match_ragged_device_locked(ctx, (const uint8_t *)ctx->chars.p, (const uint64_t *)ctx->lens.p, lo, n, M, (uint64_t *)ctx->status.p,
                                                d_counts, d_spans, max_spans, st))
            return rc;
        if (int rc = host_results_out(ctx, b0, n, status, span_counts, spans, max_spans, d_counts, d_spans, st)) return rc;
        b0 = b1;
    }
    return HRX_OK;
}

int hrx_match_selected_device(hrx_ctx *ctx, int layout, const uint8_t *src, size_t src_stride, const uint32_t *lens, const uint64_t *offsets, size_t B,
                              const uint32_t *sel, size_t n_sel, size_t M, uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (int rc = check_selected_args(layout, src, src_stride, lens, offsets, B, sel, n_sel, M, status, span_counts, spans, max_spans, true)) return rc;
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    if (B == 0 || n_sel == 0) return HRX_OK;
    const bool ragged = layout == HRX_LAYOUT_INPUT_RAGGED;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    return match_selected_device_locked(ctx, SelectedSrc{src, ragged ? offsets : nullptr, ragged ? nullptr : lens, src_stride}, B, sel, n_sel, M, status,
                                        span_counts, spans, max_spans, (hipStream_t)stream);
}

int hrx_match_selected_host(hrx_ctx *ctx, int layout, const uint8_t *src, size_t src_stride, const uint32_t *lens, const uint64_t *offsets, size_t B,
                            const uint32_t *sel, size_t n_sel, size_t M, uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (int rc = check_selected_args(layout, src, src_stride, lens, offsets, B, sel, n_sel, M, status, span_counts, spans, max_spans, false)) return rc;
    if (B == 0 || n_sel == 0) return HRX_OK;
    const bool ragged = layout == HRX_LAYOUT_INPUT_RAGGED;
    if (ctx->device == HRX_DEVICE_NONE) {     // the native host walk, no row written
        const size_t threads = std::max<size_t>(1, std::min<size_t>(ctx->host_threads > 0 ? (size_t)ctx->host_threads : std::thread::hardware_concurrency(), n_sel * M / 8192));
        host_match_selected(ctx->s, src, src_stride, ragged ? nullptr : lens, ragged ? offsets : nullptr, B, sel, n_sel, M, status, span_counts, spans, max_spans,
                            (int)threads);
        return HRX_OK;
    }
    // through the device: chunks of the selection whose strings' bytes sum to ~64 MiB, packed back to back with offsets
    // of their own, matched by the ragged chunk path, the results copied out to index sel[k].  Only the selected strings' bytes cross the link; a
    // string with no valid length gets its status here and an index at or past B is passed over
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard guard;
    HIP_TRY(guard.set(ctx->device));
    const size_t kSpan = (size_t)64 << 20;
    const size_t max_n = std::max<size_t>(1, std::min<size_t>((size_t)1 << 20, kSpan / (8 * max_spans + 12)));
    hipStream_t st = ctx->stream;
    std::vector<uint8_t> packed;
    std::vector<uint64_t> offs, h_status, h_spans;
    std::vector<uint32_t> idx, h_counts;
    for (size_t k = 0; k < n_sel;) {
        packed.clear(); offs.assign(1, 0); idx.clear();
        for (; k < n_sel && idx.size() < max_n && packed.size() < kSpan; ++k) {
            const size_t b = sel[k];
            if (b >= B) continue;
            uint64_t n;
            const uint8_t *p;
            if (ragged) {
                n = offsets[b + 1] >= offsets[b] ? offsets[b + 1] - offsets[b] : UINT64_MAX;
                p = src + offsets[b];
            } else {
                n = lens[b] <= src_stride ? lens[b] : UINT64_MAX;
                p = src + b * src_stride;
            }
            if (n > M) {
                status[b] = kStatusBadLength;
                if (span_counts) span_counts[b] = 0;
                continue;
            }
            packed.insert(packed.end(), p, p + n);
            offs.push_back(packed.size());
            idx.push_back((uint32_t)b);
        }
        const size_t n = idx.size();
        if (n == 0) continue;
        HIP_TRY(ctx->chars.reserve(((packed.size() + 15) & ~(size_t)15) + 16));
        HIP_TRY(ctx->lens.reserve(8 * (n + 1)));
        uint32_t *d_counts;
        uint64_t *d_spans;
        if (int rc = host_result_bufs(ctx, n, span_counts != nullptr, max_spans, d_counts, d_spans)) return rc;
        if (!packed.empty()) HIP_TRY(hipMemcpyAsync(ctx->chars.p, packed.data(), packed.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->lens.p, offs.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
        if (int rc = match_ragged_device_locked(ctx, (const uint8_t *)ctx->chars.p, (const uint64_t *)ctx->lens.p, 0, n, M, (uint64_t *)ctx->status.p, d_counts,
                                                d_spans, max_spans, st))
            return rc;
        h_status.resize(n);
        if (span_counts) h_counts.resize(n);
        if (max_spans) h_spans.resize(n * max_spans);
        if (int rc = host_results_out(ctx, 0, n, h_status.data(), span_counts ? h_counts.data() : nullptr, h_spans.data(), max_spans, d_counts, d_spans, st)) return rc;
        for (size_t j = 0; j < n; ++j) {
            const size_t b = idx[j];
            status[b] = h_status[j];
            if (span_counts) span_counts[b] = h_counts[j];
            if (max_spans) std::memcpy(spans + b * max_spans, h_spans.data() + j * max_spans, 8 * max_spans);
        }
    }
    return HRX_OK;
}

int hrx_ragged_to_position_major_device(hrx_ctx *ctx, const uint8_t *values, const uint64_t *offsets, size_t B, size_t stride, uint8_t *chars_pm,
                                        uint32_t *lens, void *stream) {
    if (!ctx) return fail(HRX_ERR_ARG, "NULL ctx");
    if (ctx->device == HRX_DEVICE_NONE) return fail(HRX_ERR_HIP, "host-only context (HRX_DEVICE_NONE): no device to launch on");
    if (B == 0) return HRX_OK;
    if (!values || !offsets || !chars_pm || !lens) return fail(HRX_ERR_ARG, "NULL buffer");
    if (B > 0xffffffffull - 64 || stride / 16 > 0xffffffffull) return fail(HRX_ERR_ARG, "shape out of range");
    if ((stride & 15) || stride < 16 || ((uintptr_t)values & 15) || ((uintptr_t)chars_pm & 15) || ((uintptr_t)offsets & 7) || ((uintptr_t)lens & 3))
        return fail(HRX_ERR_ARG, "values and chars_pm must be 16-byte aligned, offsets 8-byte, lens 4-byte, stride % 16 == 0 and stride >= 16");
    DeviceGuard guard;      // (stateless: no context scratch, no lock)
    HIP_TRY(guard.set(ctx->device));
    HIP_TRY(launch_ragged_to_position_major(values, offsets, 0, B, stride, chars_pm, lens, (hipStream_t)stream));
    return HRX_OK;
}

static int describe_match(const DefsSet &s, uint32_t dbg, bool mpc_on, const MatchSwitches &sw, int layout, size_t B, size_t M, int num_cus, char *out, size_t cap) {
    // HRX_LAYOUT_INPUT_SELECTED | a source layout: the launch of hrx_match_selected_device with n_sel = B
    const bool selected = (layout & HRX_LAYOUT_INPUT_SELECTED) != 0;
    const char *src_name = nullptr;
    if (selected) {
        layout &= ~HRX_LAYOUT_INPUT_SELECTED;
        if (layout != HRX_LAYOUT_STRING_MAJOR && layout != HRX_LAYOUT_INPUT_RAGGED)
            return fail(HRX_ERR_ARG, "HRX_LAYOUT_INPUT_SELECTED goes with HRX_LAYOUT_STRING_MAJOR or HRX_LAYOUT_INPUT_RAGGED");
        src_name = layout == HRX_LAYOUT_INPUT_RAGGED ? "hrx::RaggedSrc" : "hrx::PaddedSrc";
    }
    const bool ragged = layout == HRX_LAYOUT_INPUT_RAGGED;
    if (!ragged && layout != HRX_LAYOUT_STRING_MAJOR && layout != HRX_LAYOUT_INPUT_POSITION_MAJOR)
        return fail(HRX_ERR_ARG, "layout must be HRX_LAYOUT_STRING_MAJOR, HRX_LAYOUT_INPUT_POSITION_MAJOR or HRX_LAYOUT_INPUT_RAGGED");
    MatchPlan p;
    if (!match_plan(s, dbg, sw, ragged ? HRX_LAYOUT_STRING_MAJOR : layout, B, M, num_cus, p)) return fail(HRX_ERR_BOUNDS, "no match launch fits");
    if (p.wide) {
        std::snprintf(out, cap, "hrx::match_wide_kernel<%zu, %d, %s, %s> grid=persistent threads=%d lds=%zu", s.defs.size(), p.wide,
                      selected ? src_name : ragged ? "hrx::RaggedSrc" : "hrx::PaddedSrc", selected ? "true" : "false", p.threads, p.lds_bytes);
        return HRX_OK;
    }
    if (p.fused) {
        const char *g = p.gtab ? "true" : "false", *h = p.half ? "true" : "false";
        if (selected)
            std::snprintf(out, cap, "hrx::match_selected_kernel<%zu, %s, %s, %s> grid=persistent threads=%d lds=%zu", s.defs.size(), g, h, src_name, p.threads, p.lds_bytes);
        else if (ragged) std::snprintf(out, cap, "hrx::match_ragged_kernel<%zu, %s, %s> grid=persistent threads=%d lds=%zu", s.defs.size(), g, h, p.threads, p.lds_bytes);
        else std::snprintf(out, cap, "hrx::match_lane_kernel<%zu, %s, %s> grid=%d threads=%d lds=%zu", s.defs.size(), g, h, p.grid, p.threads, p.lds_bytes);
        return HRX_OK;
    }
    const ViaRows v = plan_via_rows(selected ? HRX_LAYOUT_INPUT_RAGGED : layout, 0, B, M, s.defs.size(), selected);
    if (v.slice == 0) return fail(HRX_ERR_BOUNDS, "match via rows: one string's witness rows exceed the 768 MiB scratch");
    char w[3072];
    if (int rc = describe_config(s, dbg, 0u, mpc_on, v.layout, v.slice, M, num_cus, w, sizeof w)) return rc;
    if (selected) {
        std::snprintf(out, cap, "via rows, %zu slice(s) of %zu strings: hrx::selected_slice_kernel<%s> + %s + hrx::spans_from_masked_selected_kernel",
                      (B + v.slice - 1) / v.slice, v.slice, src_name, w);
        return HRX_OK;
    }
    std::snprintf(out, cap, "via rows, %zu slice(s) of %zu strings: %s%s + hrx::spans_from_masked_pm_kernel", (B + v.slice - 1) / v.slice, v.slice,
                  ragged ? "hrx::ragged_slice_kernel + " : v.gather ? "hrx::pm_input_slice_kernel + " : "", w);
    return HRX_OK;
}

int hrx_describe_match(const hrx_defs *defs, int layout, size_t B, size_t M, int num_cus, char *out, size_t cap) {
    if (!defs || !out || !cap) return fail(HRX_ERR_ARG, "NULL argument");
    if (!defs->s.finalized) return fail(HRX_ERR_STATE, "call hrx_defs_finalize first");
    if (num_cus < 1) return fail(HRX_ERR_ARG, "num_cus must be >= 1");
    if (M == 0 || M > (1u << 24)) return fail(HRX_ERR_ARG, "max_chars_size must be in 1..2^24");
    const char *mpc = std::getenv("HRX_MP_COMBINE");      // (what hrx_ctx_create would read now)
    return describe_match(defs->s, debug_flags_from_env(), mpc && std::atoi(mpc) != 0, MatchSwitches{match_via_rows_from_env(), false}, layout, B ? B : 1, M, num_cus, out, cap);
}

int hrx_ctx_describe_match(const hrx_ctx *ctx, int layout, size_t B, size_t M, char *out, size_t cap) {
    if (!ctx || !out || !cap) return fail(HRX_ERR_ARG, "NULL argument");
    if (M == 0 || M > (1u << 24)) return fail(HRX_ERR_ARG, "max_chars_size must be in 1..2^24");
    return describe_match(ctx->s, ctx->debug, ctx->mp_combine, switches_of(ctx), layout, B ? B : 1, M, ctx->num_cus > 0 ? ctx->num_cus : 256, out, cap);
}

}  // extern "C"

