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

__device__ __forceinline__ void load_cell(const uint64_t *p, uint32_t (&w)[8]) {
    const uint4 lo = *reinterpret_cast<const uint4 *>(p), hi = *reinterpret_cast<const uint4 *>(p + 2);
    w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w; w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
}
__device__ __forceinline__ void put_cell(uint64_t *p, const uint32_t (&w)[8]) {      // plain stores: read back inside the workgroup
    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<uint4 *>(p + 2) = make_uint4(w[4], w[5], w[6], w[7]);
}
__device__ __forceinline__ void lds_get(const uint32_t *p, uint32_t (&w)[8]) {
    const uint4 lo = *reinterpret_cast<const uint4 *>(p), hi = *reinterpret_cast<const uint4 *>(p + 4);
    w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w; w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
}
__device__ __forceinline__ void lds_put(uint32_t *p, const uint32_t (&w)[8]) {
    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<uint4 *>(p + 4) = make_uint4(w[4], w[5], w[6], w[7]);
}
// a challenge or shift: 4 u64 limbs of any 256-bit value, taken mod r
__device__ __forceinline__ void load_challenge(const uint64_t *p, uint32_t (&w)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { w[2 * i] = (uint32_t)p[i]; w[2 * i + 1] = (uint32_t)(p[i] >> 32); }
    fr_reduce(w);
}
// a value every lane of the workgroup holds alike, into scalar registers
__device__ __forceinline__ void uniform8(uint32_t (&x)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = __builtin_amdgcn_readfirstlane(x[i]);
}
__device__ __forceinline__ void copy8(uint32_t (&d)[8], const uint32_t (&s)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = s[i];
}

// S[w] + c of one word as the scan's element: its Montgomery form; one where the word is none of the run's bins or the sum is zero (zero: the flag)
__device__ __forceinline__ void invert_element(const uint64_t *S, const uint32_t w, const uint32_t bins, const uint32_t (&c)[8], const bool canonical,
                                               uint32_t (&out)[8], bool &zero) {
    uint32_t s[8], sc[8];
    load_cell(S + (size_t)(w < bins ? w : 0u) * 4u, s);
    fr_add(s, c, sc);
    zero = w >= bins || fr_is_zero(sc);
    product_to_mont(sc, canonical, out);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = zero ? kFrR32[i] : out[i];
}

__global__ __launch_bounds__(kPdThreads) void lookup_invert_kernel(const InvertArgs a) {
    __shared__ uint32_t wtot[kPdWaves][8];
    __shared__ uint32_t inv_total[8];
    const uint32_t tid = threadIdx.x, run = blockIdx.x, bins = a.bins, W = a.W;
    const bool canonical = a.canonical != 0;
    const uint64_t *S = a.table + (size_t)run * W * 4u;
    uint64_t *out = a.inv + (size_t)run * W * 4u;
    uint32_t c[8];
    load_challenge(a.shift + (size_t)run * a.shift_stride, c);
    const uint32_t tiles = (bins + kPdTileRows - 1u) / kPdTileRows;

    uint32_t carry[8];
    fr_one(false, carry);
    for (uint32_t t = 0; t < tiles; ++t) {           // pass 1: out[w] = the product of the elements before w
        const uint32_t w0 = t * kPdTileRows + kPdRowsPerLane * tid;
        uint32_t e[kPdRowsPerLane][8];               // e[k]: the lane's elements 0 .. k multiplied
#pragma unroll
        for (uint32_t k = 0; k < kPdRowsPerLane; ++k) {
            uint32_t x[8];
            bool zero;
            invert_element(S, w0 + k, bins, c, canonical, x, zero);
            if (k == 0u) copy8(e[0], x);
            else fr_mul(e[k - 1u], x, e[k]);
        }
        uint32_t before[8], total[8], P[8], q[8];
        fr_block_scan_excl<kPdWaves>(e[kPdRowsPerLane - 1u], before, total, wtot);
        fr_mul(carry, before, P);
        if (w0 < bins) put_cell(out + (size_t)w0 * 4u, P);
#pragma unroll
        for (uint32_t k = 1; k < kPdRowsPerLane; ++k) {
            fr_mul(P, e[k - 1u], q);
            if (w0 + k < bins) put_cell(out + (size_t)(w0 + k) * 4u, q);
        }
        fr_mul(carry, total, q);
        copy8(carry, q);
    }
    __syncthreads();
    if (tid == 0u) {                                 // the Fermat step: once per run (the total is a product of non-zero elements)
        uint32_t x[8];
        fr_inv(carry, x);
#pragma unroll
        for (int i = 0; i < 8; ++i) inv_total[i] = x[i];
    }
    __syncthreads();                                 // ... and pass 1's cells are visible to the workgroup
#pragma unroll
    for (int i = 0; i < 8; ++i) carry[i] = inv_total[i];
    for (uint32_t t = tiles; t-- > 0u;) {            // pass 2: the tile's words mirrored over the lanes — `before` is what lies BEHIND a word
        const uint32_t m0 = t * kPdTileRows + (kPdTileRows - 1u) - kPdRowsPerLane * tid;      // the lane's k-th word is m0 - k
        uint32_t e[kPdRowsPerLane][8];
        bool zero[kPdRowsPerLane];
#pragma unroll
        for (uint32_t k = 0; k < kPdRowsPerLane; ++k) {
            uint32_t x[8];
            invert_element(S, m0 - k, bins, c, canonical, x, zero[k]);
            if (k == 0u) copy8(e[0], x);
            else fr_mul(e[k - 1u], x, e[k]);
        }
        uint32_t before[8], total[8], P[8], q[8];
        fr_block_scan_excl<kPdWaves>(e[kPdRowsPerLane - 1u], before, total, wtot);
        fr_mul(carry, before, P);                    // (1 / total of the run) x (the elements behind the lane's first word)
#pragma unroll
        for (uint32_t k = 0; k < kPdRowsPerLane; ++k) {
            const uint32_t w = m0 - k;
            if (k == 0u) copy8(q, P);
            else fr_mul(P, e[k - 1u], q);
            if (w < W) {                             // (W <= tiles x kPdTileRows: every pad word is some lane's)
                uint32_t pre[8], inv[8], res[8];
                if (w < bins) load_cell(out + (size_t)w * 4u, pre);      // pass 1's cell of this word; a pad word has none and becomes zero
                else copy8(pre, q);
                fr_mul(q, pre, inv);
                product_from_mont(inv, canonical, res);
#pragma unroll
                for (int i = 0; i < 8; ++i) res[i] = zero[k] ? 0u : res[i];
                put_cell(out + (size_t)w * 4u, res);
            }
        }
        fr_mul(carry, total, q);
        copy8(carry, q);
    }
}

__global__ __launch_bounds__(kPdThreads) void lookup_product_kernel(const ProductArgs a) {
    __shared__ alignas(16) uint32_t tile[kPdTileWords];
    __shared__ uint32_t wtot[kPdWaves][8];
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
    uint32_t beta[8], gamma[8], dab[8], s0g[8], carry[8];
    load_challenge(a.beta + (size_t)bi * a.challenge_stride, beta);
    load_challenge(a.gamma + (size_t)bi * a.challenge_stride, gamma);
    {
        uint32_t s0[8];
        load_cell(run + (size_t)L.off * 4u, s0);
        fr_add(s0, beta, dab);                       // the dummy input + beta
        fr_add(s0, gamma, s0g);                      // the table's first row + gamma: S of row 0 and of every row from T on
    }
    uniform8(beta); uniform8(gamma); uniform8(dab); uniform8(s0g);
    fr_one(false, carry);
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
        uint32_t e[kPdRowsPerLane][8];               // e[k]: the lane's terms 0 .. k multiplied
#pragma unroll
        for (uint32_t k = 0; k < kPdRowsPerLane; ++k) {
            const uint32_t i = j0 + k;
            const bool row = i < n_rows;
            const bool ok = row && product_index_ok(ia[k], L.off, L.T) && product_index_ok(is[k], L.off, L.T);
            const uint32_t wa = ok ? ia[k] : L.off, ws = ok ? is[k] : L.off;          // no index is an address before the test
            uint32_t x[8], ab[8], sg[8], ib[8], ig[8], t[8];
            lds_get(&tile[cell_slot(kPdRowsPerLane * tid + k)], x);
            fr_add(x, beta, ab);
            const bool dummy = product_input_is_dummy(k3, i, M, n);
            const uint32_t tr = row ? product_table_row(i, L.T) : 0u;
            load_cell(run + (size_t)(L.off + tr) * 4u, x);
            fr_add(x, gamma, sg);
#pragma unroll
            for (int l = 0; l < 8; ++l) { ab[l] = dummy ? dab[l] : ab[l]; sg[l] = tr == 0u ? s0g[l] : sg[l]; }
            load_cell(ib_run + (size_t)wa * 4u, ib);
            load_cell(ig_run + (size_t)ws * 4u, ig);
            product_term(ab, sg, ib, ig, canonical, t);
#pragma unroll
            for (int l = 0; l < 8; ++l) t[l] = !row ? kFrR32[l] : ok ? t[l] : 0u;      // entries behind the last row: one; a bad index: zero
            if (k == 0u) copy8(e[0], t);
            else fr_mul(e[k - 1u], t, e[k]);
        }
        uint32_t before[8], total[8], P[8], q[8], res[8];
        fr_block_scan_excl<kPdWaves>(e[kPdRowsPerLane - 1u], before, total, wtot);
        fr_mul(carry, before, P);                    // Z of the lane's first entry
#pragma unroll
        for (uint32_t k = 0; k < kPdRowsPerLane; ++k) {      // the lane's own LDS cells: nobody else has read or written them since the barrier
            if (k == 0u) copy8(q, P);
            else fr_mul(P, e[k - 1u], q);
            product_from_mont(q, canonical, res);
            lds_put(&tile[cell_slot(kPdRowsPerLane * tid + k)], res);
        }
        fr_mul(carry, total, q);
        copy8(carry, q);
        uniform8(carry);
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
    if (lane < a.ncols) {
        uint32_t zl[8], one[8];
        load_cell(a.z + (((size_t)lane * a.b_count + b) * a.z_pitch + a.n_rows) * 4u, zl);
        fr_one(a.canonical != 0, one);
        bad = !fr_eq(zl, one);
    }
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
