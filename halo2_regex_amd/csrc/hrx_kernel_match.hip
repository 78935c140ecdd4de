// hrx_kernel_match.hip — the MATCH kernels (include/hrx.h hrx_match_batch_device): status words and revealed runs, no witness rows.
//
//   match_lane_kernel<D, GTAB, HALF>   fused: one lane per string, the lane algorithm of hrx_host_walk.cpp with every row store left out; at each
//                                 tile end tile_masks + SpanEmitter (hrx_lane.h).  The table: the narrow fused table staged into LDS, the same table
//                                 read out of L2 (GTAB: too large for LDS), or the HALF table (hrx_lane.h: 2-byte entries, 256 states in 128 KiB of LDS).
//                                 What leaves the chip is the status word, the run count and the runs: ~1 input byte read per row, nothing written per row.
//   spans_from_masked_pm_kernel   "via rows": one lane per string over the masked rows [ceil(M/8)][nb][8] of a position-major witness launch.
//   pm_input_slice_kernel         "via rows" slices inside one block of position-major input -> string-major scratch.
#include "hrx_device.h"
#include "hrx_walk_pm.h"
#include "hrx_match_tile.h"

namespace hrx {

// workgroups of MatchPlan::threads lanes (64 .. kMatchThreads: smaller where the batch would leave CUs without one)
template <int D, bool GTAB, bool HALF>
__global__ __launch_bounds__(kMatchThreads) void match_lane_kernel(const MatchArgs a) {
    // the table at LDS offset 0 (the kernel declares no static LDS)
    if (!GTAB) {
        const uint32_t tab16 = (a.table_bytes + 15u) & ~15u;
        const uint8_t *img = HALF ? reinterpret_cast<const uint8_t *>(a.half_image) : reinterpret_cast<const uint8_t *>(a.table_image);
        for (uint32_t i = threadIdx.x * 16u; i < tab16; i += blockDim.x * 16u)
            *reinterpret_cast<uint4 *>(smem + i) = *reinterpret_cast<const uint4 *>(img + i);
        __syncthreads();
    }
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const uint32_t n = a.lens[b], M = a.M;
    const uint32_t max_spans = a.max_spans;
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
    uint32_t e[D], mx[D], acc_state[D], dead_row[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        e[d] = HALF ? a.dc[d].half_row_base + a.dc[d].first_state : a.dc[d].first_entry;       // states[d][0] = first_state_val: lib.rs:807
        mx[d] = 0;
        acc_state[d] = a.dc[d].first_state;
        dead_row[d] = 0xffffffffu;
    }
    uint32_t err_state[D], err_char[D];
    uint32_t sid_prev = 0, ov_row = 0xffffffffu;
    MaskCarry mc = {0, 0, 0, 0};
    SpanEmitter em;
    em.init();
    SpanSlots out{a.spans ? a.spans + b * max_spans : nullptr, max_spans};
    const uint32_t ntiles = (M + 63u) / 64u;
    uint4 cur[4], nxt[4];
    load_tile(0, cur);
    for (uint32_t t = 0; t < ntiles; ++t) {
        const uint32_t t0 = t * 64u;
        if (t + 1 < ntiles) load_tile(t0 + 64u, nxt);      // the next tile's bytes are on their way during this one's walk
        uint32_t e0[D], mx0[D];
#pragma unroll
        for (int d = 0; d < D; ++d) { e0[d] = e[d]; mx0[d] = mx[d]; }
        uint64_t nz;
        uint32_t sidq[16];
        const bool full = t0 + 64u <= n && t0 + 64u < M;
        const TileBits tb = full ? match_walk_tile<D, true, GTAB, HALF>(cur, a, e, mx, sid_prev, ov_row, acc_state, t0, n, nz, sidq)
                                 : match_walk_tile<D, false, GTAB, HALF>(cur, a, e, mx, sid_prev, ov_row, acc_state, t0, n, nz, sidq);
        // the first undefined transition of a def (rare: the tile is walked again row by row to find its row, state and byte)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (dead_row[d] == 0xffffffffu && mx[d] >= match_dead<HALF>(a, d) && mx0[d] < match_dead<HALF>(a, d)) {
                uint32_t x = e0[d];
                for (uint32_t p = 0; p < 64u && t0 + p < n; ++p) {
                    const uint32_t r = t0 + p;
                    const uint32_t ch = in[(size_t)(r / 16u) * step + (r & 15u)];
                    const uint32_t ne = match_next<GTAB, HALF>(a, x, ch);
                    if (ne >= match_dead<HALF>(a, d)) {
                        dead_row[d] = t0 + p;
                        err_state[d] = match_state<HALF>(a, d, x);
                        err_char[d] = ch;
                        break;
                    }
                    x = ne;
                }
            }
        }
        if (n == M && t + 1 == ntiles) {   // n == M: row n does not exist, s[n] is the live state
#pragma unroll
            for (int d = 0; d < D; ++d) acc_state[d] = match_state<HALF>(a, d, e[d]);
        }
        // reveal masks (lib.rs:598-764) and the runs they make
        const TileMasks tm = tile_masks<64>(tb, mc, t0, tile_is_exact(t0, n, M), rows_below(t0, n));
        if (max_spans || a.span_counts) em.tile(tm, mc, tb.ch, nz, t0, min(64u, M - t0), [&](int p) { return sid_byte(sidq, p); }, out);
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }
    em.finish(M, out);
    uint64_t status = 0;
    bool done = false;
#pragma unroll
    for (int d = 0; d < D; ++d)   // lowest def wins: the reference walks defs in order (lib.rs:806)
        if (!done && dead_row[d] != 0xffffffffu) { status = status_invalid((uint32_t)d, dead_row[d], err_state[d], err_char[d]); done = true; }
    if (!done && D > 1 && ov_row != 0xffffffffu) { status = status_overlap(ov_row); done = true; }
    if (!done) {
        uint32_t accept = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) accept |= (acc_state[d] == a.dc[d].accepted_state ? 1u : 0u) << d;
        status = status_ok(accept);
    }
    a.status[b] = status;
    if (a.span_counts) a.span_counts[b] = done ? 0u : em.count;
}

// "via rows": the runs of string b from its masked rows (exact: no optimistic masks to undo)
__global__ __launch_bounds__(256) void spans_from_masked_pm_kernel(const MatchArgs a) {
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    const size_t k = b / kPmBlock, bb = b % kPmBlock;
    const size_t nb = min((size_t)kPmBlock, (size_t)a.B - k * kPmBlock);
    const uint32_t M = a.M, noct = (M + 7u) / 8u;
    const uint16_t *mk = a.masked + k * kPmBlock * (size_t)noct * 8 + bb * 8;
    SpanEmitter em;
    em.init();
    SpanSlots out{a.spans ? a.spans + b * a.max_spans : nullptr, a.max_spans};
    const bool ok = (a.status[b] & 0xffu) == kStatusOk;
    if (ok && (a.max_spans || a.span_counts)) {
        for (uint32_t o = 0; o < noct; ++o) {
            const uint4 q = *reinterpret_cast<const uint4 *>(mk + (size_t)o * nb * 8);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t r = o * 8u + (uint32_t)i;
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
    if (a.span_counts) a.span_counts[b] = ok ? em.count : 0u;
}

__global__ __launch_bounds__(256) void pm_input_slice_kernel(const uint8_t *chars_pm, size_t stride, size_t B, size_t b0, size_t n, uint8_t *outp) {
    const size_t chunks = stride / 16;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * chunks) return;
    const size_t s = i / chunks, c = i % chunks, b = b0 + s;
    const size_t k = b / kPmBlock, bb = b % kPmBlock;
    const size_t nb = min((size_t)kPmBlock, B - k * kPmBlock);
    *reinterpret_cast<uint4 *>(outp + s * stride + c * 16) = *reinterpret_cast<const uint4 *>(chars_pm + k * kPmBlock * stride + (c * nb + bb) * 16);
}

template <int D, bool GTAB, bool HALF>
static hipError_t launch_match_one(const MatchArgs &a, const MatchPlan &p, hipStream_t stream) {
    static std::atomic<size_t> granted{0};
    if (p.lds_bytes) {
        const hipError_t e = ensure_lds(match_lane_kernel<D, GTAB, HALF>, granted, p.lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((match_lane_kernel<D, GTAB, HALF>), dim3(p.grid), dim3(p.threads), p.lds_bytes, stream, a);
    return hipGetLastError();
}
template <int D>
static hipError_t launch_match_d(const MatchArgs &a, const MatchPlan &p, hipStream_t stream) {
    if (p.half) return launch_match_one<D, false, true>(a, p, stream);
    if (p.gtab) return launch_match_one<D, true, false>(a, p, stream);
    return launch_match_one<D, false, false>(a, p, stream);
}

hipError_t launch_match_lane(const MatchArgs &a, const MatchPlan &p, hipStream_t stream) {
    if (a.B == 0) return hipSuccess;
    switch (a.D) {
    case 1: return launch_match_d<1>(a, p, stream);
    case 2: return launch_match_d<2>(a, p, stream);
    case 3: return launch_match_d<3>(a, p, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_spans_from_masked(const MatchArgs &a, hipStream_t stream) {
    if (a.B == 0) return hipSuccess;
    hipLaunchKernelGGL(spans_from_masked_pm_kernel, dim3((unsigned)(((size_t)a.B + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_pm_input_slice(const uint8_t *chars_pm, size_t stride, size_t B, size_t b0, size_t n, uint8_t *out, hipStream_t stream) {
    const size_t work = n * (stride / 16);
    if (work == 0) return hipSuccess;
    hipLaunchKernelGGL(pm_input_slice_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, chars_pm, stride, B, b0, n, out);
    return hipGetLastError();
}

}  // namespace hrx
