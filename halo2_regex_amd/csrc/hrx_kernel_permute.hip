// hrx_kernel_permute.hip — LOOKUP PERMUTE on the device (include/hrx.h hrx_lookup_permute_device): the rule of hrx_permute.hpp from the counts to the index
// columns A_idx, S_idx and the cells A', S' gathered from the compressed table.
//
// Write-bound by design: a lookup reads 4 T bytes of counts and writes 8 n_rows bytes of indices and 64 n_rows bytes of cells.  A workgroup of kPmThreads
// lanes serves one (string, lookup) and one range of positions (plan_permute).  It sums the counts in 64 bits (rule 1), then walks the table in chunks of
// kPmChunkRows rows, twelve consecutive rows per lane: one workgroup scan of (m', [m' != 0]) packed into a u64 gives every non-empty row its run's first position
// and its number among the non-empty rows, every empty row its place in the fill list.  The chunk's runs go to LDS compacted (nz, e); the empty rows go to
// the same LDS array from its end (K + Z = T) where the table is one chunk, else to the caller's workspace in a pass of their own before any position is
// written (a position's fill row may lie in any chunk).  The positions of the chunk's runs are then expanded in tiles of kPmTileRows on absolute tile borders:
// a lane takes four consecutive positions, finds the run of the first by bisection of e[] in LDS and steps to the others (runs are non-empty: one step at
// most), and writes each index column with one 16-byte streaming store — a wave writes 1 KiB of one column per instruction.  With cells the tile's indices
// are handed on through LDS and every lane copies 16 bytes — half a cell — per store, lane pairs a cell, 32 consecutive rows per instruction
// (lookup_compress_inputs_kernel's store shape); the table cells are read through the caches, consecutive positions of a run read one cell.
// No count value is an address: counts are summed and compared only; what indexes LDS, the workspace and the table are row numbers below T and run numbers
// below K.  No atomics, no scratch, nothing allocated.  The overflow words are a launch of their own (one wave per string: no two writers of a word).
#include <hip/hip_runtime.h>

#include "../../include/hrx.h"
#include "hrx_device.h"
#include "hrx_permute.hpp"

namespace hrx {

namespace {

constexpr uint32_t kPmWaves = kPmThreads / 64u;
constexpr uint32_t kPmRowsPerLane = kPmChunkRows / kPmThreads;
constexpr uint32_t kPmNoRow = 0xfffffffeu;          // tile entry of a position that is not this step's
static_assert(kPmChunkRows % kPmThreads == 0 && kPmTileRows == 4u * kPmThreads, "the lane shapes of the scan and of the expansion");

__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t *wsum) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor((unsigned long long)v, s, 64);
    __syncthreads();                                 // (wsum is free again)
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < kPmWaves; ++w) t += wsum[w];
    return t;
}

// the exclusive prefix of v over the workgroup's lanes; total: the workgroup's sum
__device__ __forceinline__ uint64_t block_scan_excl(const uint64_t v, uint64_t &total, uint64_t *wsum) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint64_t n = __shfl_up((unsigned long long)inc, off, 64);
        if (lane >= off) inc += n;
    }
    __syncthreads();
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kPmWaves; ++w) {
        const uint64_t x = wsum[w];
        if (w < wave) before += x;
        total += x;
    }
    return before + inc - v;
}

// four consecutive entries of an index column (16-byte aligned at i0): one store where all four are this step's, else word by word
__device__ __forceinline__ void put_quad(uint32_t *col, const uint32_t i0, const uint32_t (&v)[4], const bool (&in)[4]) {
    if (in[0] && in[1] && in[2] && in[3]) {
        store16_nt(col + i0, make_uint4(v[0], v[1], v[2], v[3]));
    } else {
#pragma unroll
        for (uint32_t x = 0; x < 4u; ++x)
            if (in[x]) col[i0 + x] = v[x];
    }
}

__global__ __launch_bounds__(kPmThreads) void lookup_permute_kernel(const PermuteArgs a) {
    __shared__ uint32_t rows[kPmChunkRows];          // nz[k] at k; one chunk: the empty rows from the end, zrow[j] at T - 1 - j
    __shared__ uint32_t e[kPmChunkRows];             // the first position of run k
    __shared__ alignas(16) uint32_t tile_a[kPmTileRows];
    __shared__ alignas(16) uint32_t tile_s[kPmTileRows];
    __shared__ uint64_t wsum[kPmWaves];
    const uint32_t tid = threadIdx.x;
    const uint32_t g = blockIdx.x % a.groups, pair = blockIdx.x / a.groups, c = pair % a.ncols, b = pair / a.ncols;
    const PermuteCol L = a.col[c];
    const uint32_t T = L.T, n_rows = a.n_rows;
    const uint32_t *m = a.counts + (size_t)b * a.W + L.off;
    const uint32_t g0 = g * a.group_rows, g1 = min(n_rows, g0 + a.group_rows);      // the workgroup's positions
    const size_t o = ((size_t)c * a.b_count + b) * a.pitch;
    const bool idx = a.a_idx != nullptr, cells = a.a_cells != nullptr;

    uint64_t sum = 0;                                // rule 1
    for (uint32_t t = tid; t < T; t += kPmThreads) sum += m[t];
    sum = block_sum(sum, wsum);
    if (sum > n_rows) {                              // rule 2 (uniform over the workgroup)
        if (idx) {
            for (uint32_t i0 = g0 + 4u * tid; i0 < g1; i0 += kPmTileRows) {
                const uint32_t v[4] = {kPmOverflow, kPmOverflow, kPmOverflow, kPmOverflow};
                const bool in[4] = {true, i0 + 1u < g1, i0 + 2u < g1, i0 + 3u < g1};
                put_quad(a.a_idx + o, i0, v, in);
                put_quad(a.s_idx + o, i0, v, in);
            }
        }
        if (cells) {
            for (size_t x = 2u * (size_t)g0 + tid; x < 2u * (size_t)g1; x += kPmThreads) {
                store16_nt(a.a_cells + o * 4u + x * 2u, make_uint4(0, 0, 0, 0));
                store16_nt(a.s_cells + o * 4u + x * 2u, make_uint4(0, 0, 0, 0));
            }
        }
        return;
    }
    const uint32_t pad = n_rows - (uint32_t)sum;     // rule 3
    const bool multi = T > kPmChunkRows;
    uint32_t *zws = multi ? a.zrows + (size_t)b * a.W + L.off : nullptr;
    const uint64_t *run = cells ? a.table + (size_t)b * a.table_stride : nullptr;

    // One chunk of the table: the lane's rows, the scan, the lists.  Returns through Kc / Pc the chunk's non-empty rows and positions.
    // fills: write the empty rows (to LDS, or to the workspace); runs: write nz / e
    auto chunk_lists = [&](const uint32_t c0, const uint32_t Ebase, const uint32_t Zbase, const bool fills, const bool runs, uint32_t &Kc, uint32_t &Pc) {
        const uint32_t t0 = c0 + tid * kPmRowsPerLane;
        uint32_t v[kPmRowsPerLane];
        uint64_t mine = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPmRowsPerLane; ++j) {
            const uint32_t t = t0 + j;
            v[j] = t < T ? permute_count(t, m[t], pad) : 0u;
            mine += (uint64_t)v[j] | (uint64_t)(v[j] != 0u) << 32;
        }
        uint64_t total;
        const uint64_t before = block_scan_excl(mine, total, wsum);
        uint32_t pos = Ebase + (uint32_t)before, k = (uint32_t)(before >> 32), z = Zbase + tid * kPmRowsPerLane - k;
#pragma unroll
        for (uint32_t j = 0; j < kPmRowsPerLane; ++j) {
            const uint32_t t = t0 + j;
            if (t < T) {
                if (v[j]) {
                    if (runs) { rows[k] = t; e[k] = pos; }
                    ++k;
                    pos += v[j];
                } else {
                    if (fills) {
                        if (multi) zws[z] = t;
                        else rows[T - 1u - z] = t;
                    }
                    ++z;
                }
            }
        }
        Kc = (uint32_t)(total >> 32);
        Pc = (uint32_t)total;
    };

    uint32_t Z = 0;
    if (multi) {                                     // the fill list first: every chunk's empty rows into the workspace
        uint32_t Zb = 0, Eb = 0;
        for (uint32_t c0 = 0; c0 < T; c0 += kPmChunkRows) {
            uint32_t Kc, Pc;
            chunk_lists(c0, Eb, Zb, true, false, Kc, Pc);
            Zb += min(kPmChunkRows, T - c0) - Kc;
            Eb += Pc;
        }
        Z = Zb;
        __syncthreads();                             // the workgroup's own stores to the workspace, read below
    }

    uint32_t Ebase = 0, Kbase = 0, Zbase = 0;
    for (uint32_t c0 = 0; c0 < T; c0 += kPmChunkRows) {
        if (c0) __syncthreads();                     // the last chunk's lists are read no more
        uint32_t Kc, Pc;
        chunk_lists(c0, Ebase, Zbase, !multi, true, Kc, Pc);
        if (!multi) Z = T - Kc;
        __syncthreads();
        const uint32_t lo = max(Ebase, g0), hi = min(Ebase + Pc, g1);       // the chunk's positions that are this workgroup's
        for (uint32_t base = lo & ~(kPmTileRows - 1u); base < hi && lo < hi; base += kPmTileRows) {
            const uint32_t i0 = base + 4u * tid;
            uint32_t av[4], sv[4];
            bool in[4];
            const uint32_t p = max(i0, lo);
            uint32_t kl = 0;
            if (p < min(i0 + 4u, hi)) {              // the run of the lane's first position: the last k with e[k] <= p (e[0] = Ebase <= lo)
                uint32_t kh = Kc;
                while (kh - kl > 1u) {
                    const uint32_t mid = (kl + kh) >> 1;
                    if (e[mid] <= p) kl = mid;
                    else kh = mid;
                }
            }
#pragma unroll
            for (uint32_t x = 0; x < 4u; ++x) {
                const uint32_t i = i0 + x;
                in[x] = i >= lo && i < hi;
                av[x] = sv[x] = kPmNoRow;
                if (in[x]) {
                    if (kl + 1u < Kc && e[kl + 1u] <= i) ++kl;
                    const uint32_t t = rows[kl];
                    const uint32_t j = permute_fill_place(i, e[kl], Kbase + kl);
                    uint32_t s = t;
                    if (j != kPmFirst) s = permute_fill_row(j, Z, j < Z ? (multi ? zws[j] : rows[T - 1u - j]) : 0u);
                    av[x] = L.off + t;
                    sv[x] = L.off + s;
                }
            }
            if (idx) {
                put_quad(a.a_idx + o, i0, av, in);
                put_quad(a.s_idx + o, i0, sv, in);
            }
            if (cells) {
                *reinterpret_cast<uint4 *>(&tile_a[4u * tid]) = make_uint4(av[0], av[1], av[2], av[3]);
                *reinterpret_cast<uint4 *>(&tile_s[4u * tid]) = make_uint4(sv[0], sv[1], sv[2], sv[3]);
                __syncthreads();
                const uint32_t h = tid & 1u;
                // one column's stores before the other's; a wave's instruction writes 32 consecutive rows, 1 KiB of full lines
#pragma unroll
                for (uint32_t it = 0; it < kPmTileRows / (kPmThreads / 2u); ++it) {
                    const uint32_t r = it * (kPmThreads / 2u) + (tid >> 1), w = tile_a[r];
                    if (w != kPmNoRow) store16_nt(a.a_cells + (o + base + r) * 4u + h * 2u, *reinterpret_cast<const uint4 *>(run + (size_t)w * 4u + h * 2u));
                }
#pragma unroll
                for (uint32_t it = 0; it < kPmTileRows / (kPmThreads / 2u); ++it) {
                    const uint32_t r = it * (kPmThreads / 2u) + (tid >> 1), w = tile_s[r];
                    if (w != kPmNoRow) store16_nt(a.s_cells + (o + base + r) * 4u + h * 2u, *reinterpret_cast<const uint4 *>(run + (size_t)w * 4u + h * 2u));
                }
                __syncthreads();                     // the tile's entries are read no more
            }
        }
        Ebase += Pc;
        Kbase += Kc;
        Zbase += min(kPmChunkRows, T - c0) - Kc;
    }
}

// one wave per string: bit c of its word where lookup c overflows (rules 1 and 2)
__global__ __launch_bounds__(kPmThreads) void lookup_permute_overflow_kernel(const PermuteArgs a) {
    const uint32_t lane = threadIdx.x & 63u, b = blockIdx.x * kPmWaves + (threadIdx.x >> 6);
    if (b >= a.b_count) return;                      // (wave-uniform; no barrier below)
    uint32_t over = 0;
    for (uint32_t c = 0; c < a.ncols; ++c) {
        const PermuteCol L = a.col[c];
        const uint32_t *m = a.counts + (size_t)b * a.W + L.off;
        uint64_t sum = 0;
        for (uint32_t t = lane; t < L.T; t += 64u) sum += m[t];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor((unsigned long long)sum, s, 64);
        if (sum > a.n_rows) over |= 1u << c;
    }
    if (lane == 0u) a.overflow[b] = over;
}

}  // namespace

// the caller has checked the arguments, set groups / group_rows (plan_permute) and made sure b_count x ncols x groups fits a grid
hipError_t launch_lookup_permute(const PermuteArgs &a, hipStream_t stream) {
    if (a.b_count == 0 || a.ncols == 0) return hipSuccess;
    if (a.overflow) {
        hipLaunchKernelGGL(lookup_permute_overflow_kernel, dim3((a.b_count + kPmWaves - 1u) / kPmWaves), dim3(kPmThreads), 0, stream, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(lookup_permute_kernel, dim3(a.b_count * a.ncols * a.groups), dim3(kPmThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hrx
