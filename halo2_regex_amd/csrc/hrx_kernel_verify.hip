// hrx_kernel_verify.hip — VERIFY on the device (include/hrx.h hrx_verify_rows_device*): the rules of hrx_verify.hpp over the witness rows where they lie.
//
// One lane per string, 64 strings per wave, one wave per workgroup.  A lane walks its string's rows in tiles of T rows: it issues the loads of the whole tile — the input
// bytes, every def's record quads, the masked octets — before it consumes any of them, then judges row r as soon as row r + 1 is there (Rotation::next), def by def, and
// carries one row (its byte, masked cell, records and sums) into the next tile.  In the position-major layouts consecutive lanes hold consecutive strings, so every load
// instruction of a wave reads one contiguous 1-KiB run; string-major rows go through the same loop with one strided element per lane and load.  The table lookups
// (hrx_verify.hpp: a [ns][256] array and two bitsets per def, in device memory) depend on nothing but the row's own cells.
// No atomics, no counters, no LDS, no workgroup waits for another; one store of the verdict word per string.
//
// Instantiations: DT = 1, 2, 3, 4 defs with the tile's records in registers (T = 32, 16, 16, 8), and DT = 0 — any number of defs, T = 8, the defs one after the other with
// the record before the tile read again in place of a carried one — for everything else (five defs and more; planes of five to eight defs).
//
// The chunked form (hrx_verify_rows_chunked_device*, below verify_rows_kernel): verify_chunk_kernel — one wave per (64 strings, chunk of the rows), the same
// tile loop over the chunk's tiles in the same instantiations, a summary of eight words per (string, chunk) into the caller's workspace — and
// verify_stitch_kernel, one lane per string, which folds the summaries in row order into the same verdict word.  Few long strings fill the device that way.
#include <hip/hip_runtime.h>

#include "../../include/hrx.h"
#include "hrx_kernel.hpp"
#include "hrx_verify.hpp"

namespace hrx {

namespace {

static_assert(kVfyPmBlock == HRX_PM_BLOCK, "hrx_verify.hpp and include/hrx.h");
enum : int { kRecSm = 0, kRecPm = 1, kRecPlanes = 2 };

// where string b's cells lie
struct VerifySrc {
    const unsigned char *chr;   // byte i at chr + (i / 16) * chr_step + i % 16
    size_t chr_step;
    const uint16_t *msk;        // position-major: octet o at msk + o * msk_step; string-major: row r at msk + r
    size_t msk_step;
    const uint32_t *rec;        // position-major: quad q of def d at rec + (q * D + d) * rec_step; string-major: (r, d) at rec + r * D + d
    size_t rec_step;            // planes: quad q at plane[(q % R) * D + d] + pl_off + (q / R) * rec_step
    size_t pl_off;
};

__device__ __forceinline__ VerifySrc verify_src(const VerifyArgs &a, const uint32_t b) {
    VerifySrc s;
    const bool pm = (a.layout & HRX_LAYOUT_POSITION_MAJOR) != 0, in_pm = (a.layout & HRX_LAYOUT_INPUT_POSITION_MAJOR) != 0;
    const uint32_t blk0 = (b / kVfyPmBlock) * kVfyPmBlock, nb = min(kVfyPmBlock, a.B - blk0), bl = b - blk0;
    const size_t q4 = (a.M + 3u) / 4u, q8 = (a.M + 7u) / 8u;
    if (in_pm) {
        s.chr = a.chars + (size_t)blk0 * a.stride + (size_t)bl * 16u;
        s.chr_step = (size_t)nb * 16u;
    } else {
        s.chr = a.chars + (size_t)b * a.stride;
        s.chr_step = 16u;
    }
    if (pm) {
        s.msk = a.masked + ((size_t)blk0 * q8 + bl) * 8u;
        s.msk_step = (size_t)nb * 8u;
        s.rec = a.records ? a.records + ((size_t)blk0 * q4 * a.D + bl) * 4u : nullptr;
        s.rec_step = (size_t)nb * 4u;
        const size_t R = a.n_stripes == 2u ? 2u : 1u;
        s.pl_off = ((size_t)blk0 * ((q4 + R - 1u) / R) + bl) * 4u;
    } else {
        s.msk = a.masked + (size_t)b * a.msk_pitch;
        s.msk_step = 0;
        s.rec = a.records + (size_t)b * a.rec_pitch * a.D;
        s.rec_step = 0;
        s.pl_off = 0;
    }
    return s;
}

// enable * char of rows base .. base + T - 1 (a 16-byte chunk is read where it holds a row below n: `stride` covers it)
template <int T>
__device__ __forceinline__ void load_chars(const VerifySrc &s, const uint32_t base, const uint32_t n, uint32_t (&c)[T]) {
    if constexpr (T >= 16) {
#pragma unroll
        for (int k = 0; k < T / 16; ++k) {
            const uint32_t r0 = base + 16u * k;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r0 < n) v = *reinterpret_cast<const uint4 *>(s.chr + (size_t)(r0 >> 4) * s.chr_step);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) c[16 * k + j] = r0 + j < n ? (w[j >> 2] >> (8 * (j & 3))) & 0xffu : 0u;
        }
    } else {
        static_assert(T == 8, "tiles of 8, 16 or 32 rows");
        uint2 v = make_uint2(0, 0);
        if (base < n) v = *reinterpret_cast<const uint2 *>(s.chr + (size_t)(base >> 4) * s.chr_step + (base & 8u));
        const uint32_t w[2] = {v.x, v.y};
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = base + j < n ? (w[j >> 2] >> (8 * (j & 3))) & 0xffu : 0u;
    }
}

// the masked cells of rows base .. base + T - 1 (rows >= M: 0, never judged)
template <int T, bool PM>
__device__ __forceinline__ void load_masked(const VerifySrc &s, const uint32_t base, const uint32_t M, uint32_t (&mk)[T]) {
    if constexpr (PM) {
#pragma unroll
        for (int k = 0; k < T / 8; ++k) {
            const uint32_t r0 = base + 8u * k;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r0 < M) v = *reinterpret_cast<const uint4 *>(s.msk + (size_t)(r0 >> 3) * s.msk_step);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) mk[8 * k + j] = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        }
    } else {
#pragma unroll
        for (int j = 0; j < T; ++j) mk[j] = base + j < M ? s.msk[base + j] : 0u;
    }
}

// def d's records of rows base .. base + T - 1 (rows >= M: 0, never judged)
template <int T, int REC>
__device__ __forceinline__ void load_records(const VerifyArgs &a, const VerifySrc &s, const uint32_t d, const uint32_t base, uint32_t (&x)[T]) {
    if constexpr (REC == kRecSm) {
#pragma unroll
        for (int j = 0; j < T; ++j) x[j] = base + j < a.M ? s.rec[(size_t)(base + j) * a.D + d] : 0u;
    } else {
#pragma unroll
        for (int k = 0; k < T / 4; ++k) {
            const uint32_t r0 = base + 4u * k, q = r0 >> 2;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r0 < a.M) {
                if constexpr (REC == kRecPm) {
                    v = *reinterpret_cast<const uint4 *>(s.rec + ((size_t)q * a.D + d) * s.rec_step);
                } else {
                    const uint32_t R = a.n_stripes == 2u ? 2u : 1u;
                    v = *reinterpret_cast<const uint4 *>(a.planes[(q % R) * a.D + d] + s.pl_off + (size_t)(q / R) * s.rec_step);
                }
            }
            x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
        }
    }
}

// def d's record of row r < M alone
template <int REC>
__device__ __forceinline__ uint32_t load_record(const VerifyArgs &a, const VerifySrc &s, const uint32_t d, const uint32_t r) {
    if constexpr (REC == kRecSm) return s.rec[(size_t)r * a.D + d];
    const uint32_t q = r >> 2;
    if constexpr (REC == kRecPm) return s.rec[((size_t)q * a.D + d) * s.rec_step + (r & 3u)];
    const uint32_t R = a.n_stripes == 2u ? 2u : 1u;
    return a.planes[(q % R) * a.D + d][s.pl_off + (size_t)(q / R) * s.rec_step + (r & 3u)];
}

// the kernel's loads behind the interface verify_lane (hrx_verify.hpp) walks over
template <int T, int REC>
struct DeviceTiles {
    const VerifyArgs &a;
    const VerifySrc &s;
    uint32_t n;
    __device__ __forceinline__ void chars(const uint32_t base, uint32_t (&c)[T]) const { load_chars<T>(s, base, n, c); }
    __device__ __forceinline__ void masked(const uint32_t base, uint32_t (&mk)[T]) const { load_masked<T, REC != kRecSm>(s, base, a.M, mk); }
    __device__ __forceinline__ void records(const uint32_t d, const uint32_t base, uint32_t (&x)[T]) const { load_records<T, REC>(a, s, d, base, x); }
    __device__ __forceinline__ uint32_t record(const uint32_t d, const uint32_t r) const { return load_record<REC>(a, s, d, r); }
};

template <int DT, int T, int REC>
__global__ __launch_bounds__(64) void verify_rows_kernel(const VerifyArgs a) {
    const uint32_t b = blockIdx.x * 64u + threadIdx.x;
    if (b >= a.B) return;
    const uint32_t n = a.lens[b];
    if (n > a.M) {             // the string has no rows
        a.verdict[b] = ~0ull;
        return;
    }
    const VerifySrc s = verify_src(a, b);
    a.verdict[b] = verify_lane<DT, T>(a.image, a.D, n, a.M, DeviceTiles<T, REC>{a, s, n});
}

template <int REC>
void launch_verify_form(const VerifyArgs &a, hipStream_t stream) {
    const dim3 grid((a.B + 63u) / 64u), block(64);
    switch (a.D) {
        case 1: hipLaunchKernelGGL((verify_rows_kernel<1, 32, REC>), grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((verify_rows_kernel<2, 16, REC>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((verify_rows_kernel<3, 16, REC>), grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL((verify_rows_kernel<4, 8, REC>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((verify_rows_kernel<0, 8, REC>), grid, block, 0, stream, a); break;
    }
}

// ---- the chunked form (hrx_verify_rows_chunked_device*): the same tile loop over one chunk of the rows, then a fold of the chunks' summaries.
// verify_rows_kernel above shares the loaders with it and nothing else: its text stays as it was.

// the loads behind verify_chunk_lane (hrx_verify.hpp): DeviceTiles' tiles; the row before and the row behind a chunk come as the quad that holds them in the
// position-major forms (the last and the first record of a quad: one contiguous 1-KiB run per load instruction there too), as one element string-major
template <int T, int REC>
struct ChunkTiles {
    const VerifyArgs &a;
    const VerifySrc &s;
    uint32_t n;
    __device__ __forceinline__ void chars(const uint32_t base, uint32_t (&c)[T]) const { load_chars<T>(s, base, n, c); }
    __device__ __forceinline__ void masked(const uint32_t base, uint32_t (&mk)[T]) const { load_masked<T, REC != kRecSm>(s, base, a.M, mk); }
    __device__ __forceinline__ void records(const uint32_t d, const uint32_t base, uint32_t (&x)[T]) const { load_records<T, REC>(a, s, d, base, x); }
    __device__ __forceinline__ uint32_t record(const uint32_t d, const uint32_t r) const {
        if constexpr (REC == kRecSm) {
            return load_record<REC>(a, s, d, r);
        } else {
            uint32_t x[4];
            load_records<4, REC>(a, s, d, r & ~3u, x);
            const uint32_t i = r & 3u;
            return i == 0u ? x[0] : i == 1u ? x[1] : i == 2u ? x[2] : x[3];
        }
    }
};

// One wave per (64 consecutive strings, one chunk); workgroup w: strings (w % groups) * 64 .., chunk w / groups — the waves in flight together read the same
// rows of neighbouring strings.  A summary goes out field by field, word f of (chunk k, string b) at (f K + k) B + b: eight contiguous 256-byte stores per wave.
template <int DT, int T, int REC>
__global__ __launch_bounds__(64) void verify_chunk_kernel(const VerifyChunkArgs ca) {
    const VerifyArgs &a = ca.a;
    const uint32_t groups = (a.B + 63u) / 64u;
    const uint32_t k = blockIdx.x / groups, b = (blockIdx.x - k * groups) * 64u + threadIdx.x;
    if (b >= a.B) return;
    const uint32_t n = a.lens[b];
    if (n > a.M) return;       // the string has no rows: verify_stitch_kernel reads no summary of it
    const uint32_t r0 = k * ca.chunk_rows, r1 = min(a.M, r0 + ca.chunk_rows);
    const VerifySrc s = verify_src(a, b);
    const VerifyChunk v = verify_chunk_lane<DT, T>(a.image, a.D, n, a.M, r0, r1, ChunkTiles<T, REC>{a, s, n});
    const size_t B = a.B, K = ca.K;
    uint32_t *out = ca.summaries + (size_t)k * B + b;
    out[0 * K * B] = v.flags;
    out[1 * K * B] = v.row;
    out[2 * K * B] = v.mask_row[0];
    out[3 * K * B] = v.mask_row[1];
    out[4 * K * B] = v.need1[0];
    out[5 * K * B] = v.need1[1];
    out[6 * K * B] = v.need0[0];
    out[7 * K * B] = v.need0[1];
}

// One lane per string: its K summaries in row order into the verdict word (verify_fold_chunk), one store
__global__ __launch_bounds__(64) void verify_stitch_kernel(const VerifyChunkArgs ca) {
    const VerifyArgs &a = ca.a;
    const uint32_t b = blockIdx.x * 64u + threadIdx.x;
    if (b >= a.B) return;
    if (a.lens[b] > a.M) {
        a.verdict[b] = ~0ull;
        return;
    }
    const size_t B = a.B, K = ca.K;
    VerifyAcc acc;
    verify_begin(acc);
    for (uint32_t k = 0; k < ca.K; ++k) {
        const uint32_t *in = ca.summaries + (size_t)k * B + b;
        VerifyChunk v;
        v.flags = in[0 * K * B];
        v.row = in[1 * K * B];
        v.mask_row[0] = in[2 * K * B];
        v.mask_row[1] = in[3 * K * B];
        v.need1[0] = in[4 * K * B];
        v.need1[1] = in[5 * K * B];
        v.need0[0] = in[6 * K * B];
        v.need0[1] = in[7 * K * B];
        verify_fold_chunk(acc, v);
    }
    a.verdict[b] = verify_finish(acc);
}

template <int REC>
void launch_chunk_form(const VerifyChunkArgs &ca, hipStream_t stream) {
    const dim3 grid((ca.a.B + 63u) / 64u * ca.K), block(64);
    switch (ca.a.D) {
        case 1: hipLaunchKernelGGL((verify_chunk_kernel<1, 32, REC>), grid, block, 0, stream, ca); break;
        case 2: hipLaunchKernelGGL((verify_chunk_kernel<2, 16, REC>), grid, block, 0, stream, ca); break;
        case 3: hipLaunchKernelGGL((verify_chunk_kernel<3, 16, REC>), grid, block, 0, stream, ca); break;
        case 4: hipLaunchKernelGGL((verify_chunk_kernel<4, 8, REC>), grid, block, 0, stream, ca); break;
        default: hipLaunchKernelGGL((verify_chunk_kernel<0, 8, REC>), grid, block, 0, stream, ca); break;
    }
}

}  // namespace

// the caller has checked chunk_rows, K and that ceil(B / 64) * K workgroups fit a grid
hipError_t launch_verify_chunked(const VerifyChunkArgs &ca, hipStream_t stream) {
    if (ca.a.B == 0 || ca.a.M == 0) return hipSuccess;
    if (!(ca.a.layout & HRX_LAYOUT_POSITION_MAJOR)) launch_chunk_form<kRecSm>(ca, stream);
    else if (ca.a.records) launch_chunk_form<kRecPm>(ca, stream);
    else launch_chunk_form<kRecPlanes>(ca, stream);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(verify_stitch_kernel, dim3((ca.a.B + 63u) / 64u), dim3(64), 0, stream, ca);
    return hipGetLastError();
}

hipError_t launch_verify_rows(const VerifyArgs &a, hipStream_t stream) {
    if (a.B == 0 || a.M == 0) return hipSuccess;
    if (!(a.layout & HRX_LAYOUT_POSITION_MAJOR)) launch_verify_form<kRecSm>(a, stream);
    else if (a.records) launch_verify_form<kRecPm>(a, stream);
    else launch_verify_form<kRecPlanes>(a, stream);
    return hipGetLastError();
}

}  // namespace hrx
