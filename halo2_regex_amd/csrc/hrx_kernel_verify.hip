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

// enable * char of rows base .. base + T - 1 (a 16-byte chunk is read where it holds a row below n: `stride` covers it)
template <int T>
__device__ __forceinline__ void load_chars(const RowsPlace &s, const uint32_t base, const uint32_t n, uint32_t (&c)[T]) {
    if constexpr (T >= 16) {
#pragma unroll
        for (int k = 0; k < T / 16; ++k) {
            const uint32_t r0 = base + 16u * k;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r0 < n) v = *reinterpret_cast<const uint4 *>(chr_chunk(s, r0));
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) c[16 * k + j] = r0 + j < n ? (w[j >> 2] >> (8 * (j & 3))) & 0xffu : 0u;
        }
    } else {
        static_assert(T == 8, "tiles of 8, 16 or 32 rows");
        uint2 v = make_uint2(0, 0);
        if (base < n) v = *reinterpret_cast<const uint2 *>(chr_chunk(s, base) + (base & 8u));
        const uint32_t w[2] = {v.x, v.y};
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = base + j < n ? (w[j >> 2] >> (8 * (j & 3))) & 0xffu : 0u;
    }
}

// the masked cells of rows base .. base + T - 1 (rows >= M: 0, never judged)
template <int T, bool PM>
__device__ __forceinline__ void load_masked(const RowsPlace &s, const uint32_t base, const uint32_t M, uint32_t (&mk)[T]) {
    if constexpr (PM) {
#pragma unroll
        for (int k = 0; k < T / 8; ++k) {
            const uint32_t r0 = base + 8u * k;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r0 < M) v = *reinterpret_cast<const uint4 *>(msk_octet(s, r0 >> 3));
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) mk[8 * k + j] = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        }
    } else {
#pragma unroll
        for (int j = 0; j < T; ++j) mk[j] = base + j < M ? msk_cell<false>(s, base + j) : 0u;
    }
}

// def d's records of rows base .. base + T - 1 (rows >= M: 0, never judged)
template <int T, int REC>
__device__ __forceinline__ void load_records(const VerifyArgs &a, const RowsPlace &s, const uint32_t d, const uint32_t base, uint32_t (&x)[T]) {
    if constexpr (REC == kRecSm) {
#pragma unroll
        for (int j = 0; j < T; ++j) x[j] = base + j < a.M ? rec_cell<kRecSm>(a, s, base + j, d) : 0u;
    } else {
#pragma unroll
        for (int k = 0; k < T / 4; ++k) {
            const uint32_t r0 = base + 4u * k;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r0 < a.M) v = *reinterpret_cast<const uint4 *>(rec_quad<REC>(a, s, r0 >> 2, d));
            x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
        }
    }
}

// the kernel's loads behind the interface verify_lane and verify_chunk_lane (hrx_verify.hpp) walk over.  QUAD (the chunked form): the row before and the row
// behind a chunk come as the quad that holds them in the position-major forms (the last and the first record of a quad: one contiguous 1-KiB run per load
// instruction there too), as one element string-major
template <int T, int REC, bool QUAD>
struct DeviceTiles {
    const VerifyArgs &a;
    const RowsPlace &s;
    uint32_t n;
    __device__ __forceinline__ void chars(const uint32_t base, uint32_t (&c)[T]) const { load_chars<T>(s, base, n, c); }
    __device__ __forceinline__ void masked(const uint32_t base, uint32_t (&mk)[T]) const { load_masked<T, REC != kRecSm>(s, base, a.M, mk); }
    __device__ __forceinline__ void records(const uint32_t d, const uint32_t base, uint32_t (&x)[T]) const { load_records<T, REC>(a, s, d, base, x); }
    __device__ __forceinline__ uint32_t record(const uint32_t d, const uint32_t r) const {
        if constexpr (QUAD && REC != kRecSm) {
            uint32_t x[4];
            load_records<4, REC>(a, s, d, r & ~3u, x);
            const uint32_t i = r & 3u;
            return i == 0u ? x[0] : i == 1u ? x[1] : i == 2u ? x[2] : x[3];
        } else {
            return rec_cell<REC>(a, s, r, d);
        }
    }
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
    const RowsPlace s = rows_place<true>(a, b);
    a.verdict[b] = verify_lane<DT, T>(a.image, a.D, n, a.M, DeviceTiles<T, REC, false>{a, s, n});
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
// verify_rows_kernel above shares the loaders with it; the two tile loops (verify_lane, verify_chunk_lane) are kept apart.

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
    const RowsPlace s = rows_place<true>(a, b);
    const VerifyChunk v = verify_chunk_lane<DT, T>(a.image, a.D, n, a.M, r0, r1, DeviceTiles<T, REC, true>{a, s, n});
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
    switch (rows_form(ca.a)) {
        case kRecSm: launch_chunk_form<kRecSm>(ca, stream); break;
        case kRecPm: launch_chunk_form<kRecPm>(ca, stream); break;
        default: launch_chunk_form<kRecPlanes>(ca, stream); break;
    }
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(verify_stitch_kernel, dim3((ca.a.B + 63u) / 64u), dim3(64), 0, stream, ca);
    return hipGetLastError();
}

hipError_t launch_verify_rows(const VerifyArgs &a, hipStream_t stream) {
    if (a.B == 0 || a.M == 0) return hipSuccess;
    switch (rows_form(a)) {
        case kRecSm: launch_verify_form<kRecSm>(a, stream); break;
        case kRecPm: launch_verify_form<kRecPm>(a, stream); break;
        default: launch_verify_form<kRecPlanes>(a, stream); break;
    }
    return hipGetLastError();
}

}  // namespace hrx
