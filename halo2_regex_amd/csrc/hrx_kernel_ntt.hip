// hrx_kernel_ntt.hip — FR NTT on the device (include/hrx.h hrx_fr_ntt_prepare_device / hrx_fr_ntt_device): the rule of hrx_ntt.hpp — x g^i, the
// bit-reversal permutation, k radix-2 decimation-in-time stages, 2^-k g^i — cut as ntt_plan says.
//
// ntt_pass_kernel: a workgroup of kNttThreads lanes holds a TILE of 2^tile_bits cells in LDS and runs `bits` stages on it, a barrier per stage, every lane
// tile / 2 / kNttThreads butterflies per stage (one fr_mul, one fr_add, one fr_sub each; the twiddle a 32-byte read of the workspace's table, which the
// caches hold).  The tile's cells come in and leave as whole 128-byte lines in compress's, permute's and product's shape (lane pairs a cell, a wave's
// instruction 32 consecutive cells).  What a tile is:
//   k <= kNttTileBits (ONE launch): 2^(tile_bits - k) whole columns; a cell is stored at the bit reversal of its index as it comes in.
//   k above: the permuting launch has run; stages [0, kNttTileBits) on 4096 consecutive cells, then passes of `bits` stages from s0 on: 2^bits rows 2^s0
//   cells apart, 2^cb = 4096 / 2^bits adjacent cells of each — the cells of 2^cb interleaved sub-transforms, 2 KiB or more contiguous per row.
// LDS layout: two planes, the low 16 bytes of every cell and then the high 16 bytes, so that lanes on consecutive cells read consecutive 16-byte slots —
// a stage whose pairs are 8 or more cells apart covers the banks once per 16 lanes — and no padding is needed.  The low bits of a slot are XORed with the
// top bits of the cell's index inside its column (its tile): what touches the cells in bit-reversed order (the scatter of the incoming cells, the forward
// shift: consecutive cells 2^(k-1) slots apart, all on one bank otherwise) then spreads over 16 slots.
// Shift powers: a lane takes tile / kNttThreads cells a fixed distance apart (lanes side by side on adjacent cells: no two on one bank), forms the first
// power by square-and-multiply (fr_pow_u32) and every next one with one fr_mul by g^(that distance); forward: in the first pass, on the cells as they lie
// bit-reversed in LDS; inverse: in the last pass together with 2^-k.  No table depends on g.
// ntt_permute_kernel (k above kNttTileBits only): the bit reversal of a column as blocks of 16 runs of 16 cells — block M of the input is block rev(M) of the
// output, transposed and bit-reversed inside, through LDS; in place a workgroup swaps the pair (M, rev M) and the workgroup of the larger number leaves.
// Entries [n_in, 2^k) are zero cells, never read.
// ntt_prepare_kernel: a lane per table entry, w^e by square-and-multiply from w = ROOT_OF_UNITY^(2^(28 - k)).
// No atomics, no scratch, nothing allocated, no grid-wide waiting: one launch per pass.
#include <hip/hip_runtime.h>

#include "../../include/hrx.h"
#include "hrx_fr_device.h"
#include "hrx_ntt.hpp"

namespace hrx {

namespace {

struct NttPass {
    const uint64_t *src;                            // the tile's cells come from here: `in` (the one-launch form) or `out`
    uint64_t *out;
    size_t src_pitch, out_pitch;                    // cells
    const uint32_t *ws;
    const uint64_t *shift;                          // NULL: none
    uint32_t n_cols, k, n_in;                       // n_in: the entries src has (2^k where src is out)
    uint32_t tile_bits, bits, s0, cb;
    uint32_t one_launch, first, last, inverse, canonical;
};
struct NttPermute {
    const uint64_t *in;
    uint64_t *out;
    size_t in_pitch, out_pitch;
    uint32_t k, n_in, in_place;
};

__device__ __forceinline__ uint32_t rev_bits(const uint32_t i, const uint32_t bits) { return bits ? __brev(i) >> (32u - bits) : 0u; }

// cell e of the workgroup's tile: its column and its index inside the column
__device__ __forceinline__ void tile_cell(const NttPass &a, const uint32_t e, uint32_t &col, uint32_t &i) {
    if (a.one_launch) {
        col = (blockIdx.x << (a.tile_bits - a.k)) + (e >> a.k);
        i = e & ((1u << a.k) - 1u);
    } else {
        const uint32_t tpc = a.k - a.tile_bits, tile = blockIdx.x & ((1u << tpc) - 1u), ltb = a.s0 - a.cb;
        col = blockIdx.x >> tpc;
        i = ((tile >> ltb) << (a.s0 + a.bits)) + ((tile & ((1u << ltb) - 1u)) << a.cb) + ((e >> a.cb) << a.s0) + (e & ((1u << a.cb) - 1u));
    }
}

__global__ __launch_bounds__(kNttThreads) void ntt_pass_kernel(const NttPass a) {
    uint4 *lds = reinterpret_cast<uint4 *>(smem);    // 16-byte slots: the plane of low halves, then the plane of high halves
    const uint32_t tid = threadIdx.x, h = tid & 1u, k = a.k, cells = 1u << a.tile_bits, per_lane = cells / kNttThreads, cmask = (1u << a.cb) - 1u;
    const bool inverse = a.inverse != 0;
    // the swizzle: the top sb bits of a cell's index inside its column (its tile) onto the slot's low bits (sb <= kk / 2: the two do not overlap)
    const uint32_t kk = a.one_launch ? k : a.tile_bits, sb = min(4u, kk >> 1), sw_shift = kk - sb, sw_mask = (1u << sb) - 1u;
    auto slot = [&](const uint32_t e) { return e ^ ((e >> sw_shift) & sw_mask); };
    auto get = [&](const uint32_t e) { return fr_load16(lds + slot(e), cells); };
    auto put = [&](const uint32_t e, const Fr &x) { fr_store16(lds + slot(e), x, cells); };

    for (uint32_t c = tid >> 1; c < cells; c += kNttThreads / 2u) {          // the tile's cells in: whole lines
        uint32_t col, i;
        tile_cell(a, c, col, i);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (col < a.n_cols && i < a.n_in) v = *reinterpret_cast<const uint4 *>(a.src + ((size_t)col * a.src_pitch + i) * 4u + h * 2u);
        const uint32_t e = a.one_launch ? ((c >> k) << k) | rev_bits(i, k) : c;
        lds[h * cells + slot(e)] = v;
    }
    Fr g, step, m;
    if (a.shift) step = g = ntt_shift(a.shift, a.canonical != 0);
    if (a.first && !inverse && a.shift) {            // x g^i on the cells as they lie bit-reversed: the lane's cells are i = tid + kNttThreads r (times 2^(k - 12))
        __syncthreads();
        const uint32_t tpc = a.one_launch ? 0u : k - a.tile_bits, low = a.one_launch ? 0u : rev_bits(blockIdx.x & ((1u << tpc) - 1u), tpc);
        const uint32_t qmask = (1u << kk) - 1u;
        const bool stepping = kk > kNttThreadBits;   // columns of as many cells as the workgroup has lanes, or fewer: the lane's cells have one index, in several columns
        if (stepping) step = fr_square_n(step, kNttThreadBits + tpc);
        m = fr_pow_u32(g, ((tid & qmask) << tpc) | low);
        for (uint32_t r = 0; r < per_lane; ++r) {
            const uint32_t q = tid + r * kNttThreads, e = (q & ~qmask) | rev_bits(q & qmask, kk);
            if (r && stepping) m = fr_mul(m, step);
            put(e, fr_mul(get(e), m));
        }
    }
    const uint32_t tile = a.one_launch ? 0u : blockIdx.x & ((1u << (k - a.tile_bits)) - 1u);
    const uint32_t low_pos = a.one_launch ? 0u : (tile & ((1u << (a.s0 - a.cb)) - 1u)) << a.cb;      // the tile's first cell, mod 2^s0
    for (uint32_t st = 0; st < a.bits; ++st) {
        __syncthreads();
        const uint32_t s = a.s0 + st;
        for (uint32_t u = tid; u < cells / 2u; u += kNttThreads) {
            const uint32_t l = u & cmask, mm = u >> a.cb, lowm = mm & ((1u << st) - 1u), m0 = ((mm >> st) << (st + 1u)) | lowm;
            const uint32_t e0 = (m0 << a.cb) | l, e1 = e0 + (1u << (st + a.cb));
            bool neg;
            const uint32_t ti = ntt_twiddle_index(k, s, (lowm << a.s0) + low_pos + l, inverse, neg);
            const Fr tw = fr_load16(a.ws + (size_t)ti * 8u);
            Fr x = get(e0), y = get(e1);
            ntt_butterfly(x, y, tw, neg);
            put(e0, x);
            put(e1, y);
        }
    }
    __syncthreads();
    if (a.last && inverse) {                         // 2^-k g^i: lanes side by side on adjacent cells, a lane's next cell a fixed distance on
        const Fr scale = fr_load16(a.ws + ntt_table_cells(k) * 8u);
        // one launch: cells tid + kNttThreads r, that far apart (one index where the columns are that short); a strided tile: lb bits of the lane pick the cell of a
        // row, the others a run of `rows` rows 2^s0 apart, and where a row is wider than the workgroup the lane takes 2^(cb - lb) such runs
        const uint32_t lb = min(a.cb, kNttThreadBits), rows = a.one_launch ? per_lane : per_lane >> (a.cb - lb);
        const bool stepping = a.shift && (a.one_launch ? k > kNttThreadBits : true);
        if (stepping) step = fr_square_n(step, a.one_launch ? kNttThreadBits : a.s0);
        for (uint32_t r = 0; r < per_lane; ++r) {
            const uint32_t mr = r % rows;
            const uint32_t e = a.one_launch ? tid + r * kNttThreads
                                            : (((tid >> lb) * rows + mr) << a.cb) | ((tid & ((1u << lb) - 1u)) + ((r / rows) << kNttThreadBits));
            if (!a.shift) {
                m = scale;
            } else if (mr == 0u) {
                uint32_t col, i;
                tile_cell(a, e, col, i);
                m = fr_mul(fr_pow_u32(g, i), scale);
            } else if (stepping) {
                m = fr_mul(m, step);
            }
            put(e, fr_mul(get(e), m));
        }
        __syncthreads();
    }
    for (uint32_t c = tid >> 1; c < cells; c += kNttThreads / 2u) {          // the tile's cells out: whole lines; the call's last pass streams
        uint32_t col, i;
        tile_cell(a, c, col, i);
        if (col >= a.n_cols) continue;
        const uint4 v = lds[h * cells + slot(c)];
        uint64_t *p = a.out + ((size_t)col * a.out_pitch + i) * 4u + h * 2u;
        if (a.last) store16_nt(p, v);
        else *reinterpret_cast<uint4 *>(p) = v;      // plain: the next pass reads them
    }
}

constexpr uint32_t kPermThreads = 256, kPermCells = 1u << (2u * kNttPermuteBits);
static_assert(kNttPermuteBits == 4u && kPermCells == kPermThreads, "a block is 16 runs of 16 cells: two steps of 128 cells, lane pairs a cell");

__global__ __launch_bounds__(kPermThreads) void ntt_permute_kernel(const NttPermute a) {
    __shared__ alignas(16) uint32_t blk[2][kPermCells * 8u];
    const uint32_t tid = threadIdx.x, h = tid & 1u, k = a.k, mb = k - 2u * kNttPermuteBits;
    const uint32_t M = blockIdx.x & ((1u << mb) - 1u), col = blockIdx.x >> mb, Mr = rev_bits(M, mb);
    if (a.in_place && M > Mr) return;                // (uniform; the workgroup of the pair's smaller number swaps both)
    const bool two = a.in_place && M != Mr;
    const uint64_t *in = a.in + (size_t)col * a.in_pitch * 4u;
    uint64_t *out = a.out + (size_t)col * a.out_pitch * 4u;
#pragma unroll
    for (uint32_t it = 0; it < 2u; ++it) {           // cell c = (run, cell of the run) of block M goes to cell rev8(c) of block rev(M)
        const uint32_t c = it * (kPermThreads / 2u) + (tid >> 1), run = (c >> kNttPermuteBits) << (k - kNttPermuteBits), lo = c & 15u;
        const uint32_t i = run + (M << kNttPermuteBits) + lo, i2 = run + (Mr << kNttPermuteBits) + lo, d = (__brev(c) >> 24) * 8u + h * 4u;
        uint4 v = make_uint4(0, 0, 0, 0), v2 = v;
        if (i < a.n_in) v = *reinterpret_cast<const uint4 *>(in + (size_t)i * 4u + h * 2u);
        if (two && i2 < a.n_in) v2 = *reinterpret_cast<const uint4 *>(in + (size_t)i2 * 4u + h * 2u);
        *reinterpret_cast<uint4 *>(&blk[0][d]) = v;
        if (two) *reinterpret_cast<uint4 *>(&blk[1][d]) = v2;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t it = 0; it < 2u; ++it) {
        const uint32_t c = it * (kPermThreads / 2u) + (tid >> 1), run = (c >> kNttPermuteBits) << (k - kNttPermuteBits), lo = c & 15u;
        const uint32_t j = run + (Mr << kNttPermuteBits) + lo, j2 = run + (M << kNttPermuteBits) + lo, s = c * 8u + h * 4u;
        *reinterpret_cast<uint4 *>(out + (size_t)j * 4u + h * 2u) = *reinterpret_cast<const uint4 *>(&blk[0][s]);      // plain stores: the next launch reads them
        if (two) *reinterpret_cast<uint4 *>(out + (size_t)j2 * 4u + h * 2u) = *reinterpret_cast<const uint4 *>(&blk[1][s]);
    }
}

__global__ __launch_bounds__(256) void ntt_prepare_kernel(const uint32_t k, uint32_t *ws) {
    const size_t n = ntt_table_cells(k), e = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= n) return;
    fr_store16(ws + e * 8u, fr_pow_u32(ntt_omega(k), (uint32_t)e));      // plain stores: the workspace is read by every later launch
    if (e == 0u) fr_store16(ws + n * 8u, ntt_inv_n(k));
}

}  // namespace

// the caller has checked k and the workspace
hipError_t launch_ntt_prepare(uint32_t k, uint32_t *ws, hipStream_t stream) {
    hipLaunchKernelGGL(ntt_prepare_kernel, dim3((unsigned)((ntt_table_cells(k) + 255u) / 256u)), dim3(256), 0, stream, k, ws);
    return hipGetLastError();
}

// ... and the arguments, and that every launch's workgroups fit a grid
hipError_t launch_ntt(const NttArgs &a, int device, hipStream_t stream) {
    if (a.n_cols == 0) return hipSuccess;
    static std::atomic<size_t> granted[64];
    const NttPlan plan = ntt_plan(a.k);
    NttPass p = {};
    p.out = a.out; p.out_pitch = a.out_pitch; p.ws = a.ws; p.shift = a.shift; p.n_cols = a.n_cols; p.k = a.k;
    p.inverse = a.inverse; p.canonical = a.canonical;
    auto launch = [&](unsigned grid) -> hipError_t {
        const size_t lds = (size_t)32u << p.tile_bits;
        if (lds > 65536u)                            // (the limit a kernel has without being asked: the smaller tiles never touch the attribute)
            if (hipError_t e = ensure_lds(ntt_pass_kernel, granted[device & 63], lds)) return e;
        hipLaunchKernelGGL(ntt_pass_kernel, dim3(grid), dim3(kNttThreads), lds, stream, p);
        return hipGetLastError();
    };
    if (plan.n_passes == 1u) {
        p.src = a.in; p.src_pitch = a.in_pitch; p.n_in = a.n_in;
        p.tile_bits = a.k < kNttPackBits ? kNttPackBits : a.k; p.bits = a.k; p.s0 = 0; p.cb = 0;
        p.one_launch = 1; p.first = 1; p.last = 1;
        return launch((a.n_cols + plan.cols_per_group - 1u) / plan.cols_per_group);
    }
    const NttPermute pm = {a.in, a.out, a.in_pitch, a.out_pitch, a.k, a.n_in, a.in == a.out ? 1u : 0u};
    hipLaunchKernelGGL(ntt_permute_kernel, dim3(a.n_cols << (a.k - 2u * kNttPermuteBits)), dim3(kPermThreads), 0, stream, pm);
    if (hipError_t e = hipGetLastError()) return e;
    p.src = a.out; p.src_pitch = a.out_pitch; p.n_in = 1u << a.k; p.tile_bits = kNttTileBits;
    uint32_t s0 = 0;
    for (uint32_t j = 0; j < plan.n_passes; ++j) {
        p.bits = plan.pass_bits[j]; p.s0 = s0; p.cb = kNttTileBits - p.bits;
        p.first = j == 0u; p.last = j + 1u == plan.n_passes;
        if (hipError_t e = launch(a.n_cols << (a.k - kNttTileBits))) return e;
        s0 += p.bits;
    }
    return hipSuccess;
}

}  // namespace hrx
