// hrx_kernel_compress.hip — LOOKUP COMPRESS on the device (include/hrx.h hrx_lookup_compress_inputs_device* / hrx_lookup_compress_table_device): the rule of
// hrx_compress.hpp over the witness rows where they lie, and over the context's flat array of table tuples.
//
// Over rows: write-bound by design, 96 D bytes of cells per row against 1 + 4 D bytes read, and VALU-heavy in fact — a cell is a fold of hrx_fr.h, 24 to 32
// v_mad_u64_u32 for the sum, 9 for the quotient and a subtraction.  The grid is (row tiles, strings), as fr_columns_kernel has it.  A workgroup of 256 lanes
// serves up to kCzMaxTiles tiles of kCzRowsPerTile rows of ONE string: lane 0 takes the string's challenge mod r and computes its powers (two fr_mul per
// workgroup, not per row), the workgroup takes them out of LDS into scalar registers.  A wave owns 32 kCzStores consecutive rows of a tile.  A lane computes
// WHOLE cells — the even lane of a pair that of row k, the odd lane that of row k + 32 — and the pair swaps halves (one DPP quad_perm move per limb), so that
// no fold is computed twice and still every store instruction writes 32 consecutive rows, 1 KiB of full lines, 16 bytes per lane, streaming (store16_nt);
// the kCzStores store instructions of one column come before the next column's turn.  Position-major records and planes are loaded as the row's quad
// (rec_quad), `next` from the same quad or from the first record of the next one; input bytes through chr_chunk.
// No record value is an address here: states, ids and flags are folded as they lie.  No LDS beyond the powers, no atomics, no scratch, nothing allocated.
//
// Over the table: one lane per table row (a 16-byte tuple of the image), four rows in turn per lane, the run's challenge read once per workgroup.
#include <hip/hip_runtime.h>

#include "../../include/hrx.h"
#include "hrx_compress.hpp"
#include "hrx_fr_device.h"

namespace hrx {

namespace {

// the powers of the workgroup's challenge: computed by lane 0, handed on through LDS, kept in scalar registers (they are operands of every multiply-add)
__device__ __forceinline__ FrPowers powers_of(const uint64_t *theta, const bool canonical, FrPowers *lds) {
    if (threadIdx.x == 0) *lds = fr_powers(theta, canonical);
    __syncthreads();
    return FrPowers{fr_readfirstlane(lds->t1), fr_readfirstlane(lds->t2), fr_readfirstlane(lds->t3), fr_readfirstlane(lds->one)};
}

template <int REC>
__global__ __launch_bounds__(kCzThreads) void compress_inputs_kernel(const CompressArgs a) {
    __shared__ FrPowers pw;
    const uint32_t bi = blockIdx.y;              // index inside the launch's strings
    const uint32_t b = a.b_begin + bi;
    const FrPowers p = powers_of(a.theta + (size_t)bi * a.theta_stride, a.canonical != 0, &pw);
    const uint32_t M = a.M, n = a.lens[b];
    const bool none = n > M;                     // the string has no rows: zero cells, nothing read
    const RowsPlace s = rows_place<false>(a, b);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, h = lane & 1u, k = lane >> 1;
    constexpr uint32_t kPairs = kCzStores / 2u;
    for (uint32_t t = 0; t < a.tiles; ++t) {
        const uint32_t wbase = (blockIdx.x * a.tiles + t) * kCzRowsPerTile + wave * (kCzRowsPerStore * kCzStores);
        if (wbase >= M) break;                   // (wave-uniform; no barrier below)
        // pair pr of store instructions writes rows wbase + 64 pr + [0, 64): this lane computes the cell of row[pr], the even lanes the first 32
        uint32_t row[kPairs], c[kPairs];
        bool ok[kPairs];
#pragma unroll
        for (uint32_t pr = 0; pr < kPairs; ++pr) {
            row[pr] = wbase + pr * 2u * kCzRowsPerStore + h * kCzRowsPerStore + k;
            ok[pr] = row[pr] < M && !none;
            c[pr] = ok[pr] && row[pr] < n ? chr_cell(s, row[pr]) : 0u;
        }
        for (uint32_t d = 0; d < a.D; ++d) {
            const uint32_t dummy = a.dummy[d];
            CompressTuples tp[kPairs];
#pragma unroll
            for (uint32_t pr = 0; pr < kPairs; ++pr) {
                uint32_t x = 0, next = dummy;
                if (ok[pr]) {
                    const uint32_t r = row[pr];
                    // (the record's values are folded as they lie; none of them is used as an index)
                    if constexpr (REC == kRecSm) {
                        x = rec_cell<kRecSm>(a, s, r, d);
                        if (r + 1u < M) next = rec_cell<kRecSm>(a, s, r + 1u, d) & 0xffffu;
                    } else {
                        const uint32_t q = r >> 2, j = r & 3u;
                        const uint4 v = *reinterpret_cast<const uint4 *>(rec_quad<REC>(a, s, q, d));
                        x = j == 0u ? v.x : j == 1u ? v.y : j == 2u ? v.z : v.w;
                        if (r + 1u < M) next = (j == 0u ? v.y : j == 1u ? v.z : j == 2u ? v.w : *rec_quad<REC>(a, s, q + 1u, d)) & 0xffffu;
                    }
                }
                tp[pr] = compress_def_row(dummy, row[pr], n, c[pr], x, next);
            }
            // one column: the kCzStores store instructions of the wave's rows, before the next column's turn
            auto put_column = [&](const uint32_t col, const uint32_t (&e)[kPairs][4]) {
                uint64_t *colp = a.cells + ((size_t)(3u * d + col) * a.col_cells + (size_t)bi * M) * 4u + h * 2u;
#pragma unroll
                for (uint32_t pr = 0; pr < kPairs; ++pr) {
                    const Fr w = fr_fold(e[pr][0], e[pr][1], e[pr][2], e[pr][3], p);      // (a tuple of three components has e[0] = 0)
                    // the even lane sends the high half of its cell and takes the low half of the odd lane's
                    uint32_t got[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        got[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(h ? w.w[i] : w.w[4 + i]), 0xB1 /* quad_perm [1, 0, 3, 2] */, 0xf, 0xf, false);
                    const uint4 theirs = make_uint4(got[0], got[1], got[2], got[3]);
                    const uint32_t r_a = wbase + pr * 2u * kCzRowsPerStore + k, r_b = r_a + kCzRowsPerStore;
                    uint4 cell_a = h ? theirs : fr_lo16(w);
                    uint4 cell_b = h ? fr_hi16(w) : theirs;
                    if (none) cell_a = cell_b = make_uint4(0, 0, 0, 0);
                    if (r_a < M) store16_nt(colp + (size_t)r_a * 4u, cell_a);      // streaming: nothing reads the cells back here
                    if (r_b < M) store16_nt(colp + (size_t)r_b * 4u, cell_b);
                }
            };
            uint32_t e[kPairs][4];
#pragma unroll
            for (uint32_t pr = 0; pr < kPairs; ++pr) { e[pr][0] = tp[pr].trans[0]; e[pr][1] = tp[pr].trans[1]; e[pr][2] = tp[pr].trans[2]; e[pr][3] = tp[pr].trans[3]; }
            put_column(0u, e);
#pragma unroll
            for (uint32_t pr = 0; pr < kPairs; ++pr) { e[pr][0] = 0u; e[pr][1] = tp[pr].start[1]; e[pr][2] = tp[pr].start[2]; e[pr][3] = tp[pr].start[3]; }
            put_column(1u, e);
#pragma unroll
            for (uint32_t pr = 0; pr < kPairs; ++pr) { e[pr][0] = 0u; e[pr][1] = tp[pr].end[1]; e[pr][2] = tp[pr].end[2]; e[pr][3] = tp[pr].end[3]; }
            put_column(2u, e);
        }
    }
}

__global__ __launch_bounds__(kCzThreads) void compress_table_kernel(const CompressTableArgs a) {
    __shared__ FrPowers pw;
    const uint32_t t = blockIdx.y;               // the run
    const FrPowers p = powers_of(a.theta + (size_t)t * a.theta_stride, a.canonical != 0, &pw);
#pragma unroll
    for (uint32_t j = 0; j < kCzTableRowsPerGroup / kCzThreads; ++j) {
        const uint32_t w = blockIdx.x * kCzTableRowsPerGroup + j * kCzThreads + threadIdx.x;
        if (w < a.W) {
            const uint4 tup = reinterpret_cast<const uint4 *>(a.image)[w];
            fr_store16_nt(a.cells + ((size_t)t * a.W + w) * 4u, fr_fold(tup.x, tup.y, tup.z, tup.w, p));      // streaming: nothing reads the cells back here
        }
    }
}

template <int REC>
hipError_t launch_compress_form(const CompressArgs &a, hipStream_t stream) {
    const uint32_t rows_per_group = a.tiles * kCzRowsPerTile;
    hipLaunchKernelGGL(compress_inputs_kernel<REC>, dim3((a.M + rows_per_group - 1u) / rows_per_group, a.b_count), dim3(kCzThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

// the caller has checked the arguments, set a.tiles (1 .. kCzMaxTiles) and cut the strings so that b_count fits the grid's y dimension
hipError_t launch_compress_inputs(const CompressArgs &a, hipStream_t stream) {
    if (a.b_count == 0 || a.M == 0) return hipSuccess;
    switch (rows_form(a)) {
        case kRecSm: return launch_compress_form<kRecSm>(a, stream);
        case kRecPm: return launch_compress_form<kRecPm>(a, stream);
        default: return launch_compress_form<kRecPlanes>(a, stream);
    }
}

// ... and that n_theta fits the grid's y dimension
hipError_t launch_compress_table(const CompressTableArgs &a, hipStream_t stream) {
    if (a.n_theta == 0 || a.W == 0) return hipSuccess;
    hipLaunchKernelGGL(compress_table_kernel, dim3((a.W + kCzTableRowsPerGroup - 1u) / kCzTableRowsPerGroup, a.n_theta), dim3(kCzThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hrx
