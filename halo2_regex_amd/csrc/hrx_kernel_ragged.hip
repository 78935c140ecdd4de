// hrx_kernel_ragged.hip — RAGGED input (include/hrx.h: strings back to back in one byte buffer, B + 1 u64 offsets, as an Arrow large-binary column).
//
//   match_ragged_kernel<D, GTAB, HALF>  the fused match of hrx_kernel_match.hip on ragged input: the same lane core (hrx_match_tile.h MatchLane), fed from the
//                                 aligned 16-byte chunks that hold the string's bytes, realigned with v_alignbyte_b32.  Persistent lanes: the grid fills
//                                 the device once at the kernel's occupancy, lane g walks strings g, g + G, g + 2G, ... in one flat tile loop, so a lane
//                                 that ends a short string starts its next at once.  A string stops after the tile that holds row min(n, M - 1)
//                                 (the padded kernel's later tiles change nothing).  No atomics, no counters, no scratch.
//   match_selected_kernel<D, GTAB, HALF, Src>  the same walk over a selection: lane position k walks string sel[k] of a ragged or
//                                 string-major batch and writes its results at index sel[k] (hrx_match_selected_device).
//   ragged_slice_kernel           "via rows": strings [b0, b0 + n) -> string-major [n][stride] zero-padded + lens, the input of the witness launch.
//   selected_slice_kernel<Src>    the same for a selection: slot s = string sel[k0 + s] of a ragged or string-major batch.
//   ragged_to_pm_kernel<Src, SEL> hrx_ragged_to_position_major_device (<RaggedSrc, false>): the batch -> HRX_LAYOUT_INPUT_POSITION_MAJOR + lens, one thread
//                                 per output chunk; hrx_gather_to_position_major_device (SEL): slot k = string sel[k] of a ragged or string-major batch.
// A string whose offsets decrease or whose length passes the limit (M; the stride for the staging kernels) has none of its bytes read.
#include "hrx_device.h"
#include "hrx_walk_pm.h"
#include "hrx_match_tile.h"
#include "hrx_ragged_src.h"

namespace hrx {

// bytes [16 c, 16 c + 16) of the string of n bytes at p, zero past n; reads only the aligned chunks that hold bytes of the string
__device__ __forceinline__ uint4 ragged_chunk(const uint8_t *p, uint32_t n, uint32_t c) {
    if ((uint64_t)c * 16u >= n) return make_uint4(0, 0, 0, 0);
    const uint32_t sh = (uint32_t)((uintptr_t)p & 15u);
    const uint4 *q = reinterpret_cast<const uint4 *>(p - sh);
    const uint32_t nck = (sh + n + 15u) / 16u;
    const uint4 lo = q[c], hi = c + 1u < nck ? q[c + 1] : make_uint4(0, 0, 0, 0);
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t o[4];
    realign<4>(w, sh, o);
    const uint32_t keep = n - 16u * c;       // >= 1
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = keep > 4u * k ? min(keep - 4u * k, 4u) : 0u;
        o[k] &= v >= 4u ? 0xffffffffu : ((1u << (8u * v)) - 1u);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

template <int D, bool GTAB, bool HALF>
__global__ __launch_bounds__(kMatchThreads) void match_ragged_kernel(const RaggedMatchArgs r) {
    const MatchArgs &a = r.m;
    match_stage_table<GTAB, HALF>(a);
    const size_t G = (size_t)gridDim.x * blockDim.x;
    const uint32_t M = a.M;
    size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // the lane's current string: first byte p, length n, the aligned chunk q that holds p (sh = p % 16), nck chunks from q hold its bytes,
    // tiles t < nt are walked
    const uint8_t *p = nullptr;
    const uint4 *q = nullptr;
    uint32_t n = 0, sh = 0, nck = 0, nt = 0, t = 0;
    MatchLane<D, GTAB, HALF> lane;
    uint4 win[5], nxt[4] = {};     // the tile's window: the chunk it starts in and the four after it (the last one starts the next tile)
    auto chunk = [&](uint32_t j) { return j < nck ? q[j] : make_uint4(0, 0, 0, 0); };
    // fresh: find the next string with a valid length at or after b (strings passed over get kStatusBadLength, count 0) and reset the lane's state
    for (bool fresh = true;;) {
        if (fresh) {
            for (; b < a.B; b += G) {
                if (ragged_string(a.chars, r.offsets, r.base, b, M, p, n)) break;
                a.status[b] = kStatusBadLength;
                if (a.span_counts) a.span_counts[b] = 0;
            }
            if (b >= a.B) break;
            fresh = false;
            sh = (uint32_t)((uintptr_t)p & 15u);
            q = reinterpret_cast<const uint4 *>(p - sh);
            nck = n ? (sh + n + 15u) / 16u : 0u;
            nt = min(n, M - 1u) / 64u + 1u;      // through the tile that holds row min(n, M - 1)
            t = 0;
            lane.reset(a, b);
#pragma unroll
            for (int j = 0; j < 5; ++j) win[j] = chunk((uint32_t)j);
        }
        const uint32_t t0 = t * 64u;
        if (t + 1 < nt) {      // the next tile's four new chunks are on their way during this one's walk
#pragma unroll
            for (int j = 0; j < 4; ++j) nxt[j] = chunk(4u * t + 5u + (uint32_t)j);
        }
        uint4 cq[4];
        {
            const uint32_t w[20] = {win[0].x, win[0].y, win[0].z, win[0].w, win[1].x, win[1].y, win[1].z, win[1].w, win[2].x, win[2].y,
                                    win[2].z, win[2].w, win[3].x, win[3].y, win[3].z, win[3].w, win[4].x, win[4].y, win[4].z, win[4].w};
            uint32_t o[16];
            realign<16>(w, sh, o);
#pragma unroll
            for (int j = 0; j < 4; ++j) cq[j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
        }
        // FULL only where every live lane of the wave has a full tile: lanes end their strings at different tiles, and a wave that ran both
        // forms of the walk for the same tile would pay for two walks (the general form gives the same bits on a full tile)
        lane.tile(a, cq, t0, n, t + 1 == nt, __all(t0 + 64u <= n && t0 + 64u < M), [&](uint32_t i) { return (uint32_t)p[i]; });
        win[0] = win[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) win[j + 1] = nxt[j];
        if (++t < nt) continue;
        // the string's last tile: the padded walk's later tiles hold rows > n only (no tags, no pending range left: this tile is exact)
        lane.finish(a, b);
        b += G;
        fresh = true;
    }
}

__global__ __launch_bounds__(256) void ragged_slice_kernel(const uint8_t *values, const uint64_t *offsets, uint64_t base, size_t b0, size_t n,
                                                           uint32_t limit, size_t stride, uint8_t *outp, uint32_t *lens) {
    const size_t units = stride / 16;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * units) return;
    const size_t s = i / units;
    const uint32_t c = (uint32_t)(i % units);
    const uint8_t *p;
    uint32_t len;
    const bool ok = ragged_string(values, offsets, base, b0 + s, limit, p, len);
    *reinterpret_cast<uint4 *>(outp + s * stride + (size_t)c * 16) = ok ? ragged_chunk(p, len, c) : make_uint4(0, 0, 0, 0);
    if (c == 0) lens[s] = ok ? len : 0xffffffffu;
}

// match_ragged_kernel's persistent-lane walk with two things made parameters: where a string lies (Src = RaggedSrc, or PaddedSrc: a padded slot is
// 16-byte aligned, the sh = 0 case of the window, and only the string's own tiles are walked) and which string lane position k = g, g + G, ... < n_sel
// walks: sel[k], its results at that index (an index at or past a.B is passed over: nothing read, nothing written).  A kernel of its own beside
// match_ragged_kernel, whose register allocation moved when the two shared one body
template <int D, bool GTAB, bool HALF, class Src>
__global__ __launch_bounds__(kMatchThreads) void match_selected_kernel(const MatchArgs a, const Src src, const uint32_t *sel, uint32_t n_sel) {
    match_stage_table<GTAB, HALF>(a);
    const size_t G = (size_t)gridDim.x * blockDim.x;
    const uint32_t M = a.M;
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x, b = 0;
    // the lane's current string: first byte p, length n, the aligned chunk q that holds p (sh = p % 16), nck chunks from q hold its bytes,
    // tiles t < nt are walked
    const uint8_t *p = nullptr;
    const uint4 *q = nullptr;
    uint32_t n = 0, sh = 0, nck = 0, nt = 0, t = 0;
    MatchLane<D, GTAB, HALF> lane;
    uint4 win[5], nxt[4] = {};     // the tile's window: the chunk it starts in and the four after it (the last one starts the next tile)
    auto chunk = [&](uint32_t j) { return j < nck ? q[j] : make_uint4(0, 0, 0, 0); };
    // fresh: find the next string with a valid length at or after k (strings passed over get kStatusBadLength, count 0) and reset the lane's state
    for (bool fresh = true;;) {
        if (fresh) {
            for (; k < n_sel; k += G) {
                b = sel[k];
                if (b >= a.B) continue;
                if (src.string(b, M, p, n)) break;
                a.status[b] = kStatusBadLength;
                if (a.span_counts) a.span_counts[b] = 0;
            }
            if (k >= n_sel) break;
            fresh = false;
            sh = (uint32_t)((uintptr_t)p & 15u);
            q = reinterpret_cast<const uint4 *>(p - sh);
            nck = n ? (sh + n + 15u) / 16u : 0u;
            nt = min(n, M - 1u) / 64u + 1u;      // through the tile that holds row min(n, M - 1)
            t = 0;
            lane.reset(a, b);
#pragma unroll
            for (int j = 0; j < 5; ++j) win[j] = chunk((uint32_t)j);
        }
        const uint32_t t0 = t * 64u;
        if (t + 1 < nt) {      // the next tile's four new chunks are on their way during this one's walk
#pragma unroll
            for (int j = 0; j < 4; ++j) nxt[j] = chunk(4u * t + 5u + (uint32_t)j);
        }
        uint4 cq[4];
        {
            const uint32_t w[20] = {win[0].x, win[0].y, win[0].z, win[0].w, win[1].x, win[1].y, win[1].z, win[1].w, win[2].x, win[2].y,
                                    win[2].z, win[2].w, win[3].x, win[3].y, win[3].z, win[3].w, win[4].x, win[4].y, win[4].z, win[4].w};
            uint32_t o[16];
            realign<16>(w, sh, o);
#pragma unroll
            for (int j = 0; j < 4; ++j) cq[j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
        }
        // FULL only where every live lane of the wave has a full tile: lanes end their strings at different tiles, and a wave that ran both
        // forms of the walk for the same tile would pay for two walks (the general form gives the same bits on a full tile)
        lane.tile(a, cq, t0, n, t + 1 == nt, __all(t0 + 64u <= n && t0 + 64u < M), [&](uint32_t i) { return (uint32_t)p[i]; });
        win[0] = win[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) win[j + 1] = nxt[j];
        if (++t < nt) continue;
        // the string's last tile: the padded walk's later tiles hold rows > n only (no tags, no pending range left: this tile is exact)
        lane.finish(a, b);
        k += G;
        fresh = true;
    }
}

// slot s = string sel[k0 + s] of the B_src the source has (an index at or past B_src, or a string with no valid length: a zero slot, lens = UINT32_MAX, nothing read)
template <class Src>
__global__ __launch_bounds__(256) void selected_slice_kernel(const Src src, const uint32_t *sel, uint32_t B_src, size_t k0, size_t n, uint32_t limit, size_t stride,
                                                             uint8_t *outp, uint32_t *lens) {
    const size_t units = stride / 16;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * units) return;
    const size_t s = i / units;
    const uint32_t c = (uint32_t)(i % units);
    const uint32_t b = sel[k0 + s];
    const uint8_t *p;
    uint32_t len;
    const bool ok = b < B_src && src.string(b, limit, p, len);
    *reinterpret_cast<uint4 *>(outp + s * stride + (size_t)c * 16) = ok ? ragged_chunk(p, len, c) : make_uint4(0, 0, 0, 0);
    if (c == 0) lens[s] = ok ? len : 0xffffffffu;
}

// a workgroup: 64 output slots x 8 output chunks (wave w writes chunks c0 + w and c0 + 4 + w of its 64 strings: 1 KiB contiguous per store, as
// chars_sm_to_pm_kernel); the four waves read the same 128 bytes of each string, so the strided reads share cache lines.
// SEL: slot b holds source string sel[b] of the B_src the source has (an index at or past B_src: a zero slot, nothing read); else string b itself
template <class Src, bool SEL>
__global__ __launch_bounds__(256) void ragged_to_pm_kernel(const Src src, const uint32_t *sel, uint32_t B_src, uint32_t B, uint32_t units, uint8_t *chars_pm,
                                                    uint32_t *lens) {
    const uint32_t b = blockIdx.x * 64u + (threadIdx.x & 63u);
    if (b >= B) return;
    const uint32_t blk0 = b / kPmBlock * kPmBlock, nb = min(kPmBlock, B - blk0);
    const uint8_t *p;
    uint32_t len;
    bool ok;
    if constexpr (SEL) {
        const uint32_t s = sel[b];
        ok = s < B_src && src.string(s, (uint64_t)units * 16u, p, len);
    } else {
        ok = src.string(b, (uint64_t)units * 16u, p, len);
    }
    uint4 *dst = reinterpret_cast<uint4 *>(chars_pm) + (size_t)blk0 * units + (b - blk0);
    for (uint32_t cg = blockIdx.y; cg * 8u < units; cg += gridDim.y) {
#pragma unroll
        for (uint32_t h = 0; h < 2u; ++h) {
            const uint32_t c = cg * 8u + h * 4u + (threadIdx.x >> 6);
            if (c < units) dst[(size_t)c * nb] = ok ? ragged_chunk(p, len, c) : make_uint4(0, 0, 0, 0);
        }
    }
    if (blockIdx.y == 0 && threadIdx.x < 64u) lens[b] = ok ? len : 0xffffffffu;
}

// names the ragged kernel template for fused_kernel (hrx_match_tile.h)
struct MatchRaggedKernels {
    using fn = void (*)(RaggedMatchArgs);
    template <int D, bool GTAB, bool HALF> static fn get() { return match_ragged_kernel<D, GTAB, HALF>; }
};

hipError_t launch_match_ragged(const RaggedMatchArgs &r, const MatchPlan &p, int num_cus, hipStream_t stream) {
    if (r.m.B == 0) return hipSuccess;
    MatchRaggedKernels::fn k;
    hipError_t e = fused_kernel<MatchRaggedKernels>(r.m.D, p, k);
    if (e != hipSuccess) return e;
    // persistent lanes: as many workgroups as the device holds at once (no more than the batch needs)
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, p.threads, p.lds_bytes);
    if (e != hipSuccess) return e;
    const size_t need = ((size_t)r.m.B + p.threads - 1) / p.threads;
    const size_t grid = std::min(need, (size_t)std::max(1, per_cu) * (size_t)std::max(1, num_cus));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(p.threads), p.lds_bytes, stream, r);
    return hipGetLastError();
}

// names the selected kernel template of one source for fused_kernel
template <class Src>
struct MatchSelectedKernels {
    using fn = void (*)(MatchArgs, Src, const uint32_t *, uint32_t);
    template <int D, bool GTAB, bool HALF> static fn get() { return match_selected_kernel<D, GTAB, HALF, Src>; }
};

template <class Src>
static hipError_t launch_selected(const MatchArgs &a, const Src &src, const uint32_t *sel, size_t n_sel, const MatchPlan &p, int num_cus, hipStream_t stream) {
    if (n_sel == 0 || a.B == 0) return hipSuccess;
    typename MatchSelectedKernels<Src>::fn k;
    hipError_t e = fused_kernel<MatchSelectedKernels<Src>>(a.D, p, k);
    if (e != hipSuccess) return e;
    // launch_match_ragged's grid with n_sel in place of B
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, p.threads, p.lds_bytes);
    if (e != hipSuccess) return e;
    const size_t need = (n_sel + p.threads - 1) / p.threads;
    const size_t grid = std::min(need, (size_t)std::max(1, per_cu) * (size_t)std::max(1, num_cus));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(p.threads), p.lds_bytes, stream, a, src, sel, (uint32_t)n_sel);
    return hipGetLastError();
}

hipError_t launch_match_selected(const MatchArgs &a, const SelectedSrc &s, const uint32_t *sel, size_t n_sel, const MatchPlan &p, int num_cus,
                                 hipStream_t stream) {
    if (s.offsets) return launch_selected(a, RaggedSrc{s.src, s.offsets, 0}, sel, n_sel, p, num_cus, stream);
    return launch_selected(a, PaddedSrc{s.src, s.lens, s.src_stride}, sel, n_sel, p, num_cus, stream);
}

hipError_t launch_selected_slice(const SelectedSrc &s, size_t B, const uint32_t *sel, size_t k0, size_t n, uint32_t limit, size_t stride, uint8_t *out,
                                 uint32_t *lens, hipStream_t stream) {
    const size_t work = n * (stride / 16);
    if (work == 0) return hipSuccess;
    const dim3 grid((unsigned)((work + 255) / 256));
    if (s.offsets)
        hipLaunchKernelGGL(selected_slice_kernel<RaggedSrc>, grid, dim3(256), 0, stream, RaggedSrc{s.src, s.offsets, 0}, sel, (uint32_t)B, k0, n, limit, stride, out, lens);
    else
        hipLaunchKernelGGL(selected_slice_kernel<PaddedSrc>, grid, dim3(256), 0, stream, PaddedSrc{s.src, s.lens, s.src_stride}, sel, (uint32_t)B, k0, n, limit,
                           stride, out, lens);
    return hipGetLastError();
}

hipError_t launch_ragged_slice(const uint8_t *values, const uint64_t *offsets, uint64_t base, size_t b0, size_t n, uint32_t limit, size_t stride,
                               uint8_t *out, uint32_t *lens, hipStream_t stream) {
    const size_t work = n * (stride / 16);
    if (work == 0) return hipSuccess;
    hipLaunchKernelGGL(ragged_slice_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, values, offsets, base, b0, n, limit, stride, out, lens);
    return hipGetLastError();
}

template <class Src, bool SEL>
static hipError_t launch_to_pm(const Src &src, const uint32_t *sel, size_t B_src, size_t B, size_t stride, uint8_t *chars_pm, uint32_t *lens,
                               hipStream_t stream) {
    if (B == 0) return hipSuccess;
    const uint32_t units = (uint32_t)(stride / 16);
    const size_t cgroups = (units + 7u) / 8u;
    hipLaunchKernelGGL((ragged_to_pm_kernel<Src, SEL>), dim3((unsigned)((B + 63) / 64), (unsigned)std::min<size_t>(cgroups, 65535)), dim3(256), 0, stream,
                       src, sel, (uint32_t)B_src, (uint32_t)B, units, chars_pm, lens);
    return hipGetLastError();
}

hipError_t launch_ragged_to_position_major(const uint8_t *values, const uint64_t *offsets, uint64_t base, size_t B, size_t stride, uint8_t *chars_pm,
                                           uint32_t *lens, hipStream_t stream) {
    return launch_to_pm<RaggedSrc, false>(RaggedSrc{values, offsets, base}, nullptr, B, B, stride, chars_pm, lens, stream);
}

hipError_t launch_gather_to_position_major(const uint8_t *src, size_t src_stride, const uint32_t *lens, const uint64_t *offsets, size_t B,
                                           const uint32_t *sel, size_t n_sel, size_t stride, uint8_t *chars_pm, uint32_t *lens_out, hipStream_t stream) {
    if (offsets) return launch_to_pm<RaggedSrc, true>(RaggedSrc{src, offsets, 0}, sel, B, n_sel, stride, chars_pm, lens_out, stream);
    return launch_to_pm<PaddedSrc, true>(PaddedSrc{src, lens, src_stride}, sel, B, n_sel, stride, chars_pm, lens_out, stream);
}

}  // namespace hrx
