// hrx_kernel_quotient.hip — LOOKUP QUOTIENT on the device (include/hrx.h hrx_fr_vanishing_inverse_device / hrx_lookup_quotient_device): the rule of
// hrx_quotient.hpp — the five constraint expressions of every lookup at every point of the extended coset, folded with y, divided by X^n - 1.
//
// lookup_quotient_kernel: a workgroup of kQtThreads lanes takes a TILE of kQtTileCells consecutive points of one string, one point per lane, and carries v
// in registers across all 3 D lookups: h is read at most once and written once.  Per lookup the tile's cells of the five columns come in through LDS as
// whole 128-byte lines in compress's, permute's, product's and the NTT's shape (lane pairs a cell, a wave's instruction 32 consecutive cells); LDS holds a
// column as two planes — the low 16 bytes of every cell, then the high 16 bytes, 128 bytes of padding between them — so that lanes on consecutive cells
// read consecutive 16-byte slots and the two lanes of a cell write different banks.
// Rotated reads: a tile HALO in LDS.  Z is staged from the tile's first point for kQtTileCells + rot cells, A' from rot cells below it: Z[j + rot] and
// A'[j - rot] are then the lane's own slot plus rot in either buffer.  Every staged index is taken mod N (N a power of two: a mask), which is the wrap at
// both ends of the column and also what makes a column shorter than a tile, or shorter than rot lanes' reach, read nothing outside [0, N): the slots behind
// N hold wrapped copies, the lanes behind N compute on them and store nothing.
// The selectors and h_in are staged the same way before the first lookup, v leaves through the same LDS cells with store16_nt (fr_store16_nt's instruction,
// by halves: whole lines).  The challenges are read and their constants formed once per workgroup, by its first lane into LDS (every later read of them is a
// broadcast); a lane's points all meet one t_inv entry (the tile is a multiple of rot), read and converted once.
// vanishing_inverse_kernel: one workgroup, a lane per entry: fr_pow_u32 and fr_inv.
// No atomics, no scratch, nothing allocated, no grid-wide waiting: one launch.
#include <hip/hip_runtime.h>

#include "../../include/hrx.h"
#include "hrx_fr_device.h"
#include "hrx_quotient.hpp"

namespace hrx {

namespace {

constexpr uint32_t kQtWide = kQtTileCells + kQtMaxRot;      // a column with its halo
constexpr uint32_t kQtPad = 8;                              // 16-byte slots between a column's planes: 128 bytes
static_assert((kQtWide * 16u) % 256u == 0u && (kQtTileCells * 16u) % 256u == 0u, "a plane is whole rows of the 64 banks: the padding puts the high plane half a row on");

// a column of `CELLS` cells in LDS
template <uint32_t CELLS>
struct QtColumn {
    uint4 slot[2u * CELLS + kQtPad];
    static constexpr uint32_t kApart = CELLS + kQtPad;
    // cells [first, first + CELLS) mod N of a global column: lane pairs a cell
    __device__ __forceinline__ void stage(const uint64_t *col, const uint32_t first, const uint32_t mask) {
        const uint32_t h = threadIdx.x & 1u;
#pragma unroll 1      // (rolled: the loads of five columns in flight at once cost 16 registers that the fold needs)
        for (uint32_t r = threadIdx.x >> 1; r < CELLS; r += kQtThreads / 2u)
            slot[h * kApart + r] = *reinterpret_cast<const uint4 *>(col + (size_t)((first + r) & mask) * 4u + h * 2u);
    }
    __device__ __forceinline__ Fr get(const uint32_t r) const { return fr_load16(slot + r, kApart); }
    __device__ __forceinline__ void put(const uint32_t r, const Fr &x) { fr_store16(slot + r, x, kApart); }
};

// A challenge's limbs as values the compiler takes for a lane's own.  They are the same for the whole workgroup, and the compiler, seeing that, would form
// the constants on the scalar unit: 256-bit products in scalar registers, several hundred of them spilled into lanes of vector registers.
__device__ __forceinline__ void challenge_limbs(const uint64_t *p, uint64_t (&out)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint64_t x = p[i];
        asm volatile("" : "+v"(x));
        out[i] = x;
    }
}

// the cells of the lane's point as quotient_lookup reads them: LDS slots, read where a product needs them
struct TileCells {
    const QtColumn<kQtWide> &lz, &lap;
    const QtColumn<kQtTileCells> &la, &ls, &lsp;
    uint32_t tid, rot;
    __device__ __forceinline__ Fr z() const { return lz.get(tid); }
    __device__ __forceinline__ Fr z_next() const { return lz.get(tid + rot); }
    __device__ __forceinline__ Fr a() const { return la.get(tid); }
    __device__ __forceinline__ Fr ap() const { return lap.get(tid + rot); }
    __device__ __forceinline__ Fr ap_prev() const { return lap.get(tid); }
    __device__ __forceinline__ Fr s() const { return ls.get(tid); }
    __device__ __forceinline__ Fr sp() const { return lsp.get(tid); }
};

// Three workgroups a CU by LDS (45 KiB each), so three waves a SIMD by registers: 168 VGPRs, which the fold fits with the products taken one at a time
// (HRX_QT_STEP) — `make resource-usage` shows 160 and no scratch.
__global__ __launch_bounds__(kQtThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void lookup_quotient_kernel(const QuotientArgs a) {
    __shared__ QtColumn<kQtWide> lz, lap;            // Z from the tile's first point; A' from rot cells below it
    __shared__ QtColumn<kQtTileCells> la, ls, lsp;
    const uint32_t tid = threadIdx.x, N = 1u << a.ext_k, mask = N - 1u, rot = 1u << (a.ext_k - a.k);
    const uint32_t tiles = N > kQtTileCells ? N / kQtTileCells : 1u, bi = blockIdx.x / tiles, base = (blockIdx.x % tiles) * kQtTileCells;
    const bool canonical = a.canonical != 0;
    const size_t cs = (size_t)bi * a.challenge_stride;
    __shared__ QuotientConsts q;                     // the challenges' constants: read and formed once per workgroup, by its first lane
    if (tid == 0u) {
        uint64_t beta[4], gamma[4], y[4];
        challenge_limbs(a.beta + cs, beta);
        challenge_limbs(a.gamma + cs, gamma);
        challenge_limbs(a.y + cs, y);
        quotient_consts(q, beta, gamma, y, canonical);
    }
    lz.stage(a.selectors, base, mask);               // the selectors and h_in: through the columns' cells, before the first lookup needs them
    lap.stage(a.selectors + a.sel_pitch * 4u, base, mask);
    la.stage(a.selectors + 2u * a.sel_pitch * 4u, base, mask);
    if (a.h_in) ls.stage(a.h_in + (size_t)bi * a.h_pitch * 4u, base, mask);
    __syncthreads();
    const QuotientSel sel = quotient_selectors(lz.get(tid), lap.get(tid), la.get(tid), q);
    Fr v = a.h_in ? ls.get(tid) : Fr{};

    const size_t runs = a.s_stride ? a.b_count : 1u, run = a.s_stride ? bi : 0u;
    for (uint32_t c = 0; c < a.ncols; ++c) {
        const size_t col = ((size_t)c * a.b_count + bi) * a.pitch * 4u;
        __syncthreads();                             // the cells of the lookup before are read no more
        lz.stage(a.z_ext + col, base, mask);
        lap.stage(a.ap_ext + col, base - rot, mask);
        la.stage(a.a_ext + col, base, mask);
        ls.stage(a.s_ext + ((size_t)c * runs + run) * a.s_pitch * 4u, base, mask);
        lsp.stage(a.sp_ext + col, base, mask);
        __syncthreads();
        const TileCells x = {lz, lap, la, ls, lsp, tid, rot};
        v = quotient_lookup(v, x, q, sel);
    }
    if (a.divide) v = quotient_divide(v, fr_to_mont(fr_load16(a.t_inv + (size_t)(tid & (rot - 1u)) * 4u), canonical));
    __syncthreads();
    lz.put(tid, v);
    __syncthreads();
    uint64_t *h_out = a.h_out + (size_t)bi * a.h_pitch * 4u;
    const uint32_t h = tid & 1u;
#pragma unroll
    for (uint32_t r = tid >> 1; r < kQtTileCells; r += kQtThreads / 2u)      // the tile's cells out: whole lines, streaming; nothing at or above N
        if (base + r < N) store16_nt(h_out + (size_t)(base + r) * 4u + h * 2u, lz.slot[h * lz.kApart + r]);
}

__global__ __launch_bounds__(kQtMaxRot) void vanishing_inverse_kernel(const VanishArgs a) {
    const uint32_t c = threadIdx.x;
    if (c >= (1u << (a.ext_k - a.k))) return;
    const Fr g = a.shift ? ntt_shift(a.shift, a.canonical != 0) : fr_R();
    fr_store16(a.t_inv + (size_t)c * 4u, quotient_vanishing_inverse(g, a.k, a.ext_k, c, a.canonical != 0));      // plain stores: every quotient call reads them
}

}  // namespace

// the caller has checked the arguments, and that b_count x tiles fits a grid
hipError_t launch_lookup_quotient(const QuotientArgs &a, hipStream_t stream) {
    if (a.b_count == 0 || a.ncols == 0) return hipSuccess;
    const uint32_t N = 1u << a.ext_k, tiles = N > kQtTileCells ? N / kQtTileCells : 1u;
    hipLaunchKernelGGL(lookup_quotient_kernel, dim3(a.b_count * tiles), dim3(kQtThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_vanishing_inverse(const VanishArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(vanishing_inverse_kernel, dim3(1), dim3(kQtMaxRot), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hrx
