// hrx_kernel_match.hip — the MATCH kernels (include/hrx.h hrx_match_batch_device): status words and revealed runs, no witness rows.
//
//   match_lane_kernel<D, GTAB, HALF>   fused: one lane per string, the lane algorithm of hrx_host_walk.cpp with every row store left out; at each
//                                 tile end tile_masks + SpanEmitter (hrx_lane.h).  The table: the narrow fused table staged into LDS, the same table
//                                 read out of L2 (GTAB: too large for LDS), or the HALF table (hrx_lane.h: 2-byte entries, 256 states in 128 KiB of LDS).
//                                 What leaves the chip is the status word, the run count and the runs: ~1 input byte read per row, nothing written per row.
//                                 The kernel is the padded input's addressing and prefetch around the lane core (hrx_match_tile.h MatchLane).
//   spans_from_masked_pm_kernel   "via rows": one lane per string over the masked rows [ceil(M/8)][nb][8] of a position-major witness launch.
//   spans_from_masked_selected_kernel   the same scan for hrx_match_selected_device: slot s of the slice -> the outputs of string sel[s].
//   pm_input_slice_kernel         "via rows" slices inside one block of position-major input -> string-major scratch.
#include "hrx_device.h"
#include "hrx_walk_pm.h"
#include "hrx_match_tile.h"

namespace hrx {

// workgroups of MatchPlan::threads lanes (64 .. kMatchThreads: smaller where the batch would leave CUs without one)
template <int D, bool GTAB, bool HALF>
__global__ __launch_bounds__(kMatchThreads) void match_lane_kernel(const MatchArgs a) {
    match_stage_table<GTAB, HALF>(a);
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const uint32_t n = a.lens[b], M = a.M;
    if (n > M) {
        a.status[b] = kStatusBadLength;
        if (a.span_counts) a.span_counts[b] = 0;
        return;
    }
    // where the lane's 16-byte input chunks are: string-major chars + b * stride + 16 i, or position-major (include/hrx.h) chunk i of string b
    const uint8_t *in;
    size_t step;
    if (a.in_pm) {
        const size_t k = b / kPmBlock, bb = b % kPmBlock;
        const size_t nb = min((size_t)kPmBlock, (size_t)a.B - k * kPmBlock);
        in = a.chars + k * kPmBlock * a.stride + bb * 16;
        step = nb * 16;
    } else {
        in = a.chars + b * a.stride;
        step = 16;
    }
    const uint32_t nchunks = (n + 15u) / 16u;     // chunks that hold bytes of the string: nothing beyond them is read
    auto load_tile = [&](uint32_t t0, uint4 (&cq)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t c = t0 / 16u + (uint32_t)j;
            cq[j] = c < nchunks ? *reinterpret_cast<const uint4 *>(in + (size_t)c * step) : make_uint4(0, 0, 0, 0);
        }
    };
    MatchLane<D, GTAB, HALF> lane;
    lane.reset(a, b);
    const uint32_t ntiles = (M + 63u) / 64u;
    uint4 cur[4], nxt[4];
    load_tile(0, cur);
    for (uint32_t t = 0; t < ntiles; ++t) {
        const uint32_t t0 = t * 64u;
        if (t + 1 < ntiles) load_tile(t0 + 64u, nxt);      // the next tile's bytes are on their way during this one's walk
        lane.tile(a, cur, t0, n, t + 1 == ntiles, t0 + 64u <= n && t0 + 64u < M, [&](uint32_t r) { return (uint32_t)in[(size_t)(r / 16u) * step + (r & 15u)]; });
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }
    lane.finish(a, b);
}

// "via rows": the runs of slot b of a slice from its masked rows (exact: no optimistic masks to undo).  SEL: the slot's status word, count and runs go
// to index o.sel[b] of o's arrays (an index at or past o.B_src: nothing is written); else to index b of a's own
template <bool SEL>
__device__ __forceinline__ void spans_from_masked(const MatchArgs &a, const SpanScatter &o) {
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    size_t ob = b;
    uint64_t *ospans = a.spans;
    uint32_t *ocounts = a.span_counts;
    if constexpr (SEL) {
        ob = o.sel[b];
        if (ob >= o.B_src) return;
        ospans = o.spans;
        ocounts = o.span_counts;
    }
    const size_t k = b / kPmBlock, bb = b % kPmBlock;
    const size_t nb = min((size_t)kPmBlock, (size_t)a.B - k * kPmBlock);
    const uint32_t M = a.M, noct = (M + 7u) / 8u;
    const uint16_t *mk = a.masked + k * kPmBlock * (size_t)noct * 8 + bb * 8;
    SpanEmitter em;
    em.init();
    SpanSlots out{ospans ? ospans + ob * a.max_spans : nullptr, a.max_spans};
    const uint64_t st = a.status[b];
    const bool ok = (st & 0xffu) == kStatusOk;
    if (ok && (a.max_spans || ocounts)) {
        for (uint32_t oc = 0; oc < noct; ++oc) {
            const uint4 q = *reinterpret_cast<const uint4 *>(mk + (size_t)oc * nb * 8);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t r = oc * 8u + (uint32_t)i;
                if (r >= M) break;
                const uint32_t v = (w[i >> 1] >> (16 * (i & 1) + 8)) & 0xffu;   // masked_substr_id (lib.rs:752-761)
                if (v != (em.open ? em.o_sid : 0u)) {
                    if (em.open) em.close(r, out);
                    if (v) { em.open = 1; em.o_start = r; em.o_sid = v; }
                }
            }
        }
        em.finish(M, out);
    }
    if constexpr (SEL) o.status[ob] = st;
    if (ocounts) ocounts[ob] = ok ? em.count : 0u;
}

__global__ __launch_bounds__(256) void spans_from_masked_pm_kernel(const MatchArgs a) { spans_from_masked<false>(a, SpanScatter{}); }
__global__ __launch_bounds__(256) void spans_from_masked_selected_kernel(const MatchArgs a, const SpanScatter o) { spans_from_masked<true>(a, o); }

__global__ __launch_bounds__(256) void pm_input_slice_kernel(const uint8_t *chars_pm, size_t stride, size_t B, size_t b0, size_t n, uint8_t *outp) {
    const size_t chunks = stride / 16;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * chunks) return;
    const size_t s = i / chunks, c = i % chunks, b = b0 + s;
    const size_t k = b / kPmBlock, bb = b % kPmBlock;
    const size_t nb = min((size_t)kPmBlock, B - k * kPmBlock);
    *reinterpret_cast<uint4 *>(outp + s * stride + c * 16) = *reinterpret_cast<const uint4 *>(chars_pm + k * kPmBlock * stride + (c * nb + bb) * 16);
}

// names the padded kernel template for fused_kernel (hrx_match_tile.h)
struct MatchLaneKernels {
    using fn = void (*)(MatchArgs);
    template <int D, bool GTAB, bool HALF> static fn get() { return match_lane_kernel<D, GTAB, HALF>; }
};

hipError_t launch_match_lane(const MatchArgs &a, const MatchPlan &p, hipStream_t stream) {
    if (a.B == 0) return hipSuccess;
    MatchLaneKernels::fn k;
    const hipError_t e = fused_kernel<MatchLaneKernels>(a.D, p, k);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(p.grid), dim3(p.threads), p.lds_bytes, stream, a);
    return hipGetLastError();
}

hipError_t launch_spans_from_masked(const MatchArgs &a, hipStream_t stream) {
    if (a.B == 0) return hipSuccess;
    hipLaunchKernelGGL(spans_from_masked_pm_kernel, dim3((unsigned)(((size_t)a.B + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_spans_from_masked_selected(const MatchArgs &a, const SpanScatter &o, hipStream_t stream) {
    if (a.B == 0) return hipSuccess;
    hipLaunchKernelGGL(spans_from_masked_selected_kernel, dim3((unsigned)(((size_t)a.B + 255) / 256)), dim3(256), 0, stream, a, o);
    return hipGetLastError();
}

hipError_t launch_pm_input_slice(const uint8_t *chars_pm, size_t stride, size_t B, size_t b0, size_t n, uint8_t *out, hipStream_t stream) {
    const size_t work = n * (stride / 16);
    if (work == 0) return hipSuccess;
    hipLaunchKernelGGL(pm_input_slice_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, chars_pm, stride, B, b0, n, out);
    return hipGetLastError();
}

}  // namespace hrx
