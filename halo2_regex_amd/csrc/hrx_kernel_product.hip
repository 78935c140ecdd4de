// hrx_kernel_product.hip — LOOKUP PRODUCT on the device (include/hrx.h hrx_lookup_invert_table_device / hrx_lookup_product_device): the rule of
// hrx_product.hpp — the inverse tables 1 / (S + c) by batch inversion, and the grand product Z of halo2's lookup argument as a running product of terms
// that are three multiplications and two gathers each.  Both kernels are built on the workgroup product scan of hrx_fr_scan.h and cut their cells alike:
// a workgroup of kPdThreads lanes walks tiles of kPdTileRows cells, kPdRowsPerLane consecutive cells per lane, the running product carried in registers.
//
// Invert: one workgroup per run, ONE launch (kPdInvertLaunches).  Pass 1 walks the run's bins forward: every lane takes S[w] + c of its four words (a zero
// replaced by one and found again in pass 2 by the same test), the scan gives the product of everything before each word, which is written to the word's
// output cell as it is.  Lane 0 then inverts the run's total — fr_inv, about 380 dependent fr_mul, the other lanes wait at a barrier — and pass 2 walks
// the tiles backward with the words of a tile MIRRORED over the lanes, so that the same scan gives the product of everything behind each word: the word's
// inverse is (what lies before it) (what lies behind it) / total.  Pass 2 reads pass 1's cells of other lanes of the workgroup: plain stores and the
// barrier around the Fermat step order them.  Words [bins, W) get zero cells.
//
// Product: one workgroup per (string, lookup), tiles over the ENTRIES of the Z column — entry j is the product of the terms below j, so a tile's stores
// and its loads of the input cells lie on the same row borders.  A tile's input cells come in through LDS in compress's and permute's shape (lane pairs a
// cell, a wave's instruction 32 consecutive rows, whole lines) and the tile's Z cells leave through the same LDS cells with store16_nt; a lane's four cells
// are 128 bytes apart in LDS plus 16 bytes of padding per lane, so that eight lanes' 16-byte accesses cover the banks once.  The index columns are read
// 16 bytes per lane; table and inverse cells through the caches.  No index is an address before product_index_ok: a word that fails is replaced by the
// lookup's first word for the gather and the term is set to zero.  `open` is a launch of its own (one wave per string: a word has one writer).
// No atomics, no scratch, nothing allocated.
#include <hip/hip_runtime.h>

#include "../../include/hrx.h"
#include "hrx_device.h"
#include "hrx_fr_scan.h"
#include "hrx_product.hpp"

namespace hrx {

namespace {

constexpr uint32_t kPdWaves = kPdThreads / 64u;
static_assert(kPdRowsPerLane == 4u && kPdTileRows == 4u * kPdThreads, "a lane's cells: one 16-byte load of each index column, one 128-byte line");
// the LDS word of a tile's cell r: 8 words a cell, 4 words of padding behind every lane's four cells
__device__ __forceinline__ uint32_t cell_slot(const uint32_t r) { return r * 8u + (r >> 2) * 4u; }
constexpr uint32_t kPdTileWords = kPdTileRows * 8u + (kPdTileRows / 4u) * 4u;      // 36 KiB

// S[w] + c of one word as the scan's element: its Montgomery form; one where the word is none of the run's bins or the sum is zero (zero: the flag)
__device__ __forceinline__ Fr invert_element(const uint64_t *S, const uint32_t w, const uint32_t bins, const Fr &c, const bool canonical, bool &zero) {
    const Fr sc = fr_add(fr_load16(S + (size_t)(w < bins ? w : 0u) * 4u), c);
    zero = w >= bins || fr_is_zero(sc);
    return fr_select(zero, fr_R(), fr_to_mont(sc, canonical));
}

__global__ __launch_bounds__(kPdThreads) void lookup_invert_kernel(const InvertArgs a) {
    __shared__ Fr wtot[kPdWaves];
    __shared__ Fr inv_total;
    const uint32_t tid = threadIdx.x, run = blockIdx.x, bins = a.bins, W = a.W;
    const bool canonical = a.canonical != 0;
    const uint64_t *S = a.table + (size_t)run * W * 4u;
    uint64_t *out = a.inv + (size_t)run * W * 4u;
    const Fr c = fr_challenge(a.shift + (size_t)run * a.shift_stride);
    const uint32_t tiles = (bins + kPdTileRows - 1u) / kPdTileRows;

    // pass 1's cells are read back by other lanes of the workgroup in pass 2: plain stores (fr_store16) throughout
    Fr carry = fr_R();
    for (uint32_t t = 0; t < tiles; ++t) {           // pass 1: out[w] = the product of the elements before w
        const uint32_t w0 = t * kPdTileRows + kPdRowsPerLane * tid;
        Fr e[kPdRowsPerLane];                        // e[k]: the lane's elements 0 .. k multiplied
        // (the unroll counts are spelled out: a body of several fr_mul is beyond the size the compiler unrolls at by itself before it splits stack objects
        // into registers, and e[] indexed by a loop still rolled then is left in scratch)
#pragma unroll kPdRowsPerLane
        for (uint32_t k = 0; k < kPdRowsPerLane; ++k) {
            bool zero;
            const Fr x = invert_element(S, w0 + k, bins, c, canonical, zero);
            if (k == 0u) e[0] = x;
            else e[k] = fr_mul(e[k - 1u], x);
        }
        const FrScan sc = fr_block_scan_excl<kPdWaves>(e[kPdRowsPerLane - 1u], wtot);
        const Fr P = fr_mul(carry, sc.before);
        if (w0 < bins) fr_store16(out + (size_t)w0 * 4u, P);
#pragma unroll kPdRowsPerLane
        for (uint32_t k = 1; k < kPdRowsPerLane; ++k) {
            const Fr q = fr_mul(P, e[k - 1u]);
            if (w0 + k < bins) fr_store16(out + (size_t)(w0 + k) * 4u, q);
        }
        carry = fr_mul(carry, sc.total);
    }
    __syncthreads();
    if (tid == 0u) inv_total = fr_inv(carry);        // the Fermat step: once per run (the total is a product of non-zero elements)
    __syncthreads();                                 // ... and pass 1's cells are visible to the workgroup
    carry = inv_total;
    for (uint32_t t = tiles; t-- > 0u;) {            // pass 2: the tile's words mirrored over the lanes — `before` is what lies BEHIND a word
        const uint32_t m0 = t * kPdTileRows + (kPdTileRows - 1u) - kPdRowsPerLane * tid;      // the lane's k-th word is m0 - k
        Fr e[kPdRowsPerLane];
        bool zero[kPdRowsPerLane];
#pragma unroll kPdRowsPerLane
        for (uint32_t k = 0; k < kPdRowsPerLane; ++k) {
            const Fr x = invert_element(S, m0 - k, bins, c, canonical, zero[k]);
            if (k == 0u) e[0] = x;
            else e[k] = fr_mul(e[k - 1u], x);
        }
        const FrScan sc = fr_block_scan_excl<kPdWaves>(e[kPdRowsPerLane - 1u], wtot);
        const Fr P = fr_mul(carry, sc.before);       // (1 / total of the run) x (the elements behind the lane's first word)
#pragma unroll kPdRowsPerLane
        for (uint32_t k = 0; k < kPdRowsPerLane; ++k) {
            const uint32_t w = m0 - k;
            const Fr q = k == 0u ? P : fr_mul(P, e[k - 1u]);
            if (w < W) {                             // (W <= tiles x kPdTileRows: every pad word is some lane's)
                const Fr pre = w < bins ? fr_load16(out + (size_t)w * 4u) : q;      // pass 1's cell of this word; a pad word has none and becomes zero
                fr_store16(out + (size_t)w * 4u, fr_select(zero[k], Fr{}, fr_from_mont(fr_mul(q, pre), canonical)));
            }
        }
        carry = fr_mul(carry, sc.total);
    }
}

__global__ __launch_bounds__(kPdThreads) void lookup_product_kernel(const ProductArgs a) {
    __shared__ alignas(16) uint32_t tile[kPdTileWords];
    __shared__ Fr wtot[kPdWaves];
    const uint32_t tid = threadIdx.x, c = blockIdx.x % a.ncols, bi = blockIdx.x / a.ncols, k3 = c % 3u;
    const PermuteCol L = a.col[c];
    const uint32_t M = a.M, n = a.lens[a.b_begin + bi], n_rows = a.n_rows, entries = n_rows + 1u;
    const bool canonical = a.canonical != 0;
    const uint64_t *run = a.table + (size_t)bi * a.table_stride, *ib_run = a.inv_beta + (size_t)bi * a.table_stride,
                   *ig_run = a.inv_gamma + (size_t)bi * a.table_stride;
    const size_t pair = (size_t)c * a.b_count + bi;
    const uint64_t *in = a.in_cells + pair * M * 4u;
    const uint32_t *a_idx = a.a_idx + pair * a.idx_pitch, *s_idx = a.s_idx + pair * a.idx_pitch;
    uint64_t *z = a.z + pair * a.z_pitch * 4u;
    const uint32_t a_hi = n > M ? 0u : min(M, n_rows);                // the rows that have an input cell
    // what every lane of the workgroup holds alike goes into scalar registers
    const Fr s0 = fr_load16(run + (size_t)L.off * 4u);
    const Fr beta = fr_readfirstlane(fr_challenge(a.beta + (size_t)bi * a.challenge_stride));
    const Fr gamma = fr_readfirstlane(fr_challenge(a.gamma + (size_t)bi * a.challenge_stride));
    const Fr dab = fr_readfirstlane(fr_add(s0, beta));                // the dummy input + beta
    const Fr s0g = fr_readfirstlane(fr_add(s0, gamma));               // the table's first row + gamma: S of row 0 and of every row from T on
    Fr carry = fr_R();
    const uint32_t h = tid & 1u;
    for (uint32_t base = 0; base < entries; base += kPdTileRows) {
        if (base) __syncthreads();                   // the last tile's Z cells are read no more
#pragma unroll
        for (uint32_t it = 0; it < kPdTileRows / (kPdThreads / 2u); ++it) {      // the tile's input cells: lane pairs a cell, 32 consecutive rows per instruction
            const uint32_t r = it * (kPdThreads / 2u) + (tid >> 1), i = base + r;
            if (i < a_hi) *reinterpret_cast<uint4 *>(&tile[cell_slot(r) + h * 4u]) = *reinterpret_cast<const uint4 *>(in + (size_t)i * 4u + h * 2u);
        }
        __syncthreads();
        const uint32_t j0 = base + kPdRowsPerLane * tid;
        uint4 ia4 = make_uint4(0, 0, 0, 0), is4 = ia4;
        if (j0 < n_rows) {                           // (j0 + 3 < idx_pitch: the pitch is a multiple of 4)
            ia4 = *reinterpret_cast<const uint4 *>(a_idx + j0);
            is4 = *reinterpret_cast<const uint4 *>(s_idx + j0);
        }
        const uint32_t ia[4] = {ia4.x, ia4.y, ia4.z, ia4.w}, is[4] = {is4.x, is4.y, is4.z, is4.w};
        Fr e[kPdRowsPerLane];                        // e[k]: the lane's terms 0 .. k multiplied
#pragma unroll kPdRowsPerLane
        for (uint32_t k = 0; k < kPdRowsPerLane; ++k) {
            const uint32_t i = j0 + k;
            const bool row = i < n_rows;
            const bool ok = row && product_index_ok(ia[k], L.off, L.T) && product_index_ok(is[k], L.off, L.T);
            const uint32_t wa = ok ? ia[k] : L.off, ws = ok ? is[k] : L.off;          // no index is an address before the test
            const bool dummy = product_input_is_dummy(k3, i, M, n);
            const uint32_t tr = row ? product_table_row(i, L.T) : 0u;
            const Fr ab = fr_select(dummy, dab, fr_add(fr_load16(&tile[cell_slot(kPdRowsPerLane * tid + k)]), beta));
            const Fr sg = fr_select(tr == 0u, s0g, fr_add(fr_load16(run + (size_t)(L.off + tr) * 4u), gamma));
            const Fr t = product_term(ab, sg, fr_load16(ib_run + (size_t)wa * 4u), fr_load16(ig_run + (size_t)ws * 4u), canonical);
            const Fr term = fr_select(!row, fr_R(), fr_select(ok, t, Fr{}));      // entries behind the last row: one; a bad index: zero
            if (k == 0u) e[0] = term;
            else e[k] = fr_mul(e[k - 1u], term);
        }
        const FrScan sc = fr_block_scan_excl<kPdWaves>(e[kPdRowsPerLane - 1u], wtot);
        const Fr P = fr_mul(carry, sc.before);       // Z of the lane's first entry
#pragma unroll kPdRowsPerLane
        for (uint32_t k = 0; k < kPdRowsPerLane; ++k) {      // the lane's own LDS cells: nobody else has read or written them since the barrier
            const Fr q = k == 0u ? P : fr_mul(P, e[k - 1u]);
            fr_store16(&tile[cell_slot(kPdRowsPerLane * tid + k)], fr_from_mont(q, canonical));
        }
        carry = fr_readfirstlane(fr_mul(carry, sc.total));
        __syncthreads();
#pragma unroll
        for (uint32_t it = 0; it < kPdTileRows / (kPdThreads / 2u); ++it) {      // the tile's Z cells: whole lines, streaming
            const uint32_t r = it * (kPdThreads / 2u) + (tid >> 1), j = base + r;
            if (j < entries) store16_nt(z + (size_t)j * 4u + h * 2u, *reinterpret_cast<const uint4 *>(&tile[cell_slot(r) + h * 4u]));
        }
    }
}

// one wave per string: bit c of its word where Z[n_rows] of lookup c is not one
__global__ __launch_bounds__(kPdThreads) void lookup_product_open_kernel(const ProductArgs a) {
    const uint32_t lane = threadIdx.x & 63u, b = blockIdx.x * kPdWaves + (threadIdx.x >> 6);
    if (b >= a.b_count) return;                      // (wave-uniform; no barrier below)
    bool bad = false;
    if (lane < a.ncols) bad = !fr_eq(fr_load16(a.z + (((size_t)lane * a.b_count + b) * a.z_pitch + a.n_rows) * 4u), fr_unit(a.canonical != 0));
    const uint64_t m = __ballot(bad);
    if (lane == 0u) a.open[b] = (uint32_t)m;
}

}  // namespace

// the caller has checked the arguments and made sure n_runs fits a grid
hipError_t launch_lookup_invert(const InvertArgs &a, hipStream_t stream) {
    if (a.n_runs == 0 || a.W == 0) return hipSuccess;
    hipLaunchKernelGGL(lookup_invert_kernel, dim3(a.n_runs), dim3(kPdThreads), 0, stream, a);
    return hipGetLastError();
}

// ... and that b_count x ncols fits a grid, and ncols an open word where one is asked for
hipError_t launch_lookup_product(const ProductArgs &a, hipStream_t stream) {
    if (a.b_count == 0 || a.ncols == 0) return hipSuccess;
    hipLaunchKernelGGL(lookup_product_kernel, dim3(a.b_count * a.ncols), dim3(kPdThreads), 0, stream, a);
    if (hipError_t e = hipGetLastError()) return e;
    if (a.open) {
        hipLaunchKernelGGL(lookup_product_open_kernel, dim3((a.b_count + kPdWaves - 1u) / kPdWaves), dim3(kPdThreads), 0, stream, a);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace hrx
