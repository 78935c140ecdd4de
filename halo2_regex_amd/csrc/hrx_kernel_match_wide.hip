// hrx_kernel_match_wide.hip — the fused MATCH walk for four to eight defs (HRX_OPT_MATCH_FUSED_WIDE, include/hrx.h).
//
//   match_wide_kernel<D, G, Src, SEL>  match_selected_kernel's persistent-lane shell (hrx_kernel_ragged.hip) around the lane core of hrx_match_wide.h: the
//                                 config's CLASS-WIDE image staged to LDS offset 0 once per workgroup, lane position k = g, g + lanes, ... walks string
//                                 sel[k] (SEL) or string k of a ragged (RaggedSrc) or string-major (PaddedSrc) batch, G defs side by side per sweep, and
//                                 writes its status, run count and runs at that string's index.  Only the string's own tiles are walked; a string with no
//                                 valid length gets kStatusBadLength and count 0 with none of its bytes read; sel[k] >= B is passed over.
// No atomics, no counters, no scratch: the launch is deterministic and legal in a stream capture on a fresh context — what the via-rows route of these
// configs is not.
#include "hrx_device.h"
#include "hrx_walk_pm.h"
#include "hrx_ragged_src.h"
#include "hrx_match_wide.h"

namespace hrx {

// the lane core's table reads: the image lies at LDS offset 0 (the kernel declares no static LDS)
struct WideLds {
    __device__ __forceinline__ uint32_t lo(uint32_t off) const { return lds_u32(off); }
    __device__ __forceinline__ uint32_t lut(uint32_t off) const { return lds_u8(off); }
};

template <int D, int G, class Src, bool SEL>
__global__ __launch_bounds__(kMatchThreads) void match_wide_kernel(const MatchWideArgs a, const Src src, const uint32_t *sel, uint32_t n_sel) {
    for (uint32_t i = threadIdx.x * 16u; i < a.image_bytes; i += blockDim.x * 16u)
        *reinterpret_cast<uint4 *>(smem + i) = *reinterpret_cast<const uint4 *>(a.cw_image + i);
    __syncthreads();
    const WideLds tab;
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
    const uint32_t M = a.M;
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x, b = 0;
    // the lane's current string: first byte p, length n, the aligned chunk q that holds p (sh = p % 16), nck chunks from q hold its bytes,
    // tiles t < nt are walked
    const uint8_t *p = nullptr;
    const uint4 *q = nullptr;
    uint32_t n = 0, sh = 0, nck = 0, nt = 0, t = 0;
    MatchLaneWide<D, G> lane;
    uint4 win[5], nxt[4] = {};     // the tile's window: the chunk it starts in and the four after it (the last one starts the next tile)
    auto chunk = [&](uint32_t j) { return j < nck ? q[j] : make_uint4(0, 0, 0, 0); };
    // fresh: find the next string with a valid length at or after k (strings passed over get kStatusBadLength, count 0) and reset the lane's state
    for (bool fresh = true;;) {
        if (fresh) {
            for (; k < n_sel; k += lanes) {
                b = SEL ? (size_t)sel[k] : k;
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
        uint32_t cw[16];
        {
            const uint32_t w[20] = {win[0].x, win[0].y, win[0].z, win[0].w, win[1].x, win[1].y, win[1].z, win[1].w, win[2].x, win[2].y,
                                    win[2].z, win[2].w, win[3].x, win[3].y, win[3].z, win[3].w, win[4].x, win[4].y, win[4].z, win[4].w};
            realign<16>(w, sh, cw);
        }
        // FULL only where every live lane of the wave has a full tile (match_ragged_kernel: a wave that ran both forms of the walk for the same tile
        // would pay for two walks)
        lane.tile(tab, a, cw, t0, n, t + 1 == nt, __all(t0 + 64u <= n && t0 + 64u < M), [&](uint32_t i) { return (uint32_t)p[i]; });
        win[0] = win[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) win[j + 1] = nxt[j];
        if (++t < nt) continue;
        // the string's last tile: the padded walk's later tiles hold rows > n only (no tags, no pending range left: this tile is exact)
        lane.finish(a, b);
        k += lanes;
        fresh = true;
    }
}

namespace {
template <class Src, bool SEL>
struct MatchWideKernels {
    using fn = void (*)(MatchWideArgs, Src, const uint32_t *, uint32_t);
    // the kernel of (D, G) with the image's dynamic LDS granted
    template <int D, int G>
    static hipError_t one(size_t lds, fn &k) {
        static std::atomic<size_t> granted{0};
        k = match_wide_kernel<D, G, Src, SEL>;
        return ensure_lds(k, granted, lds);
    }
    // the widths plan_match_wide picks: four defs side by side, and at four defs one by one for batches of more than a wave per SIMD
    static hipError_t get(uint32_t D, int G, size_t lds, fn &k) {
        if (G == 1 && D == 4) return one<4, 1>(lds, k);
        if (G != 4) return hipErrorInvalidValue;
        switch (D) {
        case 4: return one<4, 4>(lds, k);
        case 5: return one<5, 4>(lds, k);
        case 6: return one<6, 4>(lds, k);
        case 7: return one<7, 4>(lds, k);
        case 8: return one<8, 4>(lds, k);
        default: return hipErrorInvalidValue;
        }
    }
};
}  // namespace

template <class Src, bool SEL>
static hipError_t launch_wide(const MatchWideArgs &a, const Src &src, const uint32_t *sel, size_t n, const MatchPlan &p, int num_cus, hipStream_t stream) {
    typename MatchWideKernels<Src, SEL>::fn k;
    hipError_t e = MatchWideKernels<Src, SEL>::get(a.D, p.wide, p.lds_bytes, k);
    if (e != hipSuccess) return e;
    // launch_match_ragged's grid: as many workgroups as the device holds at once (no more than the strings need)
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, p.threads, p.lds_bytes);
    if (e != hipSuccess) return e;
    const size_t need = (n + p.threads - 1) / p.threads;
    const size_t grid = std::min(need, (size_t)std::max(1, per_cu) * (size_t)std::max(1, num_cus));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(p.threads), p.lds_bytes, stream, a, src, sel, (uint32_t)n);
    return hipGetLastError();
}

hipError_t launch_match_wide(const MatchWideArgs &a, const SelectedSrc &s, uint64_t base, const uint32_t *sel, size_t n_sel, const MatchPlan &p, int num_cus,
                             hipStream_t stream) {
    const size_t n = sel ? n_sel : (size_t)a.B;
    if (n == 0 || a.B == 0) return hipSuccess;
    if (s.offsets) {
        const RaggedSrc src{s.src, s.offsets, base};
        return sel ? launch_wide<RaggedSrc, true>(a, src, sel, n, p, num_cus, stream) : launch_wide<RaggedSrc, false>(a, src, nullptr, n, p, num_cus, stream);
    }
    const PaddedSrc src{s.src, s.lens, s.src_stride};
    return sel ? launch_wide<PaddedSrc, true>(a, src, sel, n, p, num_cus, stream) : launch_wide<PaddedSrc, false>(a, src, nullptr, n, p, num_cus, stream);
}

}  // namespace hrx
