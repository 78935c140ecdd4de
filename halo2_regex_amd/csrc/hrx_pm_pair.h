// hrx_pm_pair.h — what the three wave roles of a position-major pair (loader, walker, finisher: hrx_kernel_pm.hip) share: the pair's
// LDS offsets, its place in the workgroup and its sequence of string groups; and two small rules every role spells the same way
// (a tile's 16 dwords, a chain entry's state number).  Device-only.
#pragma once
#include "hrx_walk_pm.h"

namespace hrx {

// the 16 dwords of a tile's four 16-byte pieces (64 bytes of one string, four rows per dword)
__device__ __forceinline__ void tile_words(const uint4 (&cq)[4], uint32_t (&w)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { w[4 * i] = cq[i].x; w[4 * i + 1] = cq[i].y; w[4 * i + 2] = cq[i].z; w[4 * i + 3] = cq[i].w; }
}

// chain entry -> the def's own state number (what a record, an error and the accept check speak of): the entry's row field minus the def's first row
template <bool WIDE, bool HALF, bool BYTE>
__device__ __forceinline__ uint32_t entry_state(const uint32_t e, const WitnessArgs &a, const int d) {
    if (BYTE) return e;
    if (HALF) return (e & 0xffu) - a.dc[d].half_row_base;
    return (WIDE ? ((e >> kWideRowShift) & 0xffu) : (e >> kNextShift)) - a.dc[d].row_base;
}

struct PmPair {
    uint32_t lane, pairs, pair;   // walker waves 0..pairs-1, loader waves pairs..2*pairs-1, FIN: finisher waves 2*pairs..3*pairs-1
    // ring + the walker's 4-KiB scratch (HALF: none, its slow path re-walks out of registers) + FIN: the 6-KiB tile summary
    // + counters (hrx_kernel.hpp pm_pair_bytes: the planner budgets the same bytes)
    uint32_t ring_base, scratch_off, sum_off;
    uint32_t ready_off, freed_off;
    // FIN: freed2 = ring slots the finisher is done with; sum_ready / sum_freed = tile summaries written / consumed
    uint32_t freed2_off, sum_ready_off, sum_freed_off;
    // dynamic groups: gq_ready = groups the loader has published, gq = the queue of their indices (16 entries)
    uint32_t gq_ready_off, gq_off;
    // CHUNKED launch (hrx_kernel_spec.hip): every string is cut into vs_chunks pieces of vs_tiles tiles and each piece is walked as a
    // group of its own — virtual group vg = chunk * vs_groups + real group, chunk-major, so that the chip still writes one compact
    // slab at a time — from the state, previous substr id and end flag the scout / compose launches found for its first row
    // (a.vs_init).  The roles work on absolute rows, so n, M, padding, the accept state and the error rows keep their meaning.
    bool vs, dyn;
    uint32_t gt;                  // tiles per (virtual) group
    uint32_t vs_groups, vs_tiles; // (WitnessArgs)
    uint32_t g_first, g_stride;

    __device__ __forceinline__ uint32_t vg_real(const uint32_t vg) const { return vs ? vg % vs_groups : vg; }
    __device__ __forceinline__ uint32_t vg_tile0(const uint32_t vg) const { return vs ? (vg / vs_groups) * vs_tiles : 0u; }
    // j-th group of this pair (j = 0, 1, ..); >= n_groups: there is none.  Static: a fixed stride.  Dynamic (plan_witness_launch:
    // batches of >= 8 long groups per pair): the first group is static, every further one is whatever the pair's LOADER drew from
    // the launch's counter when it got there (it runs ahead of the other two waves) and published in the LDS queue — pairs on
    // faster XCDs simply draw more often.
    __device__ __forceinline__ uint32_t group_at(const uint32_t j) const {
        if (!dyn || j == 0u) return g_first + j * g_stride;
        ring_wait(gq_ready_off, j);
        return lds_vol_u32(gq_off + (j & 15u) * 4u);
    }
    __device__ __forceinline__ uint32_t slot(const uint32_t seq, const uint32_t nring) const { return ring_base + (seq % nring) * kPmTileBytes; }
};

// wave `wave` of a workgroup whose LDS holds tab_bytes of table in front of the pairs' areas; wg = the workgroup's place in the launch
template <bool HALF, bool FIN>
__device__ __forceinline__ PmPair pm_pair(const WitnessArgs &a, const uint32_t nring, const uint32_t tab_bytes, const uint32_t wave, const uint32_t wg) {
    const uint32_t pairs = (blockDim.x >> 6) / (FIN ? 3u : 2u), pair = wave % pairs;
    const uint32_t ring_base = tab_bytes + pair * (uint32_t)pm_pair_bytes(nring, HALF, FIN);
    const uint32_t scratch_off = ring_base + nring * kPmTileBytes;
    const uint32_t sum_off = scratch_off + (HALF ? 0u : kPmTileBytes);
    const uint32_t ready_off = sum_off + (FIN ? kPmSummaryBytes : 0u);
    const bool vs = FIN && a.vs_init != nullptr;
    return PmPair{threadIdx.x & 63u, pairs, pair, ring_base, scratch_off, sum_off, ready_off, ready_off + 4u,
                  ready_off + 8u, ready_off + 12u, ready_off + 16u, ready_off + 20u, ready_off + 32u,
                  vs, a.group_counter != nullptr, vs ? a.vs_tiles : (a.M + 63u) >> 6, a.vs_groups, a.vs_tiles,
                  xcd_slot(wg, gridDim.x, (a.debug & kDbgXcdRemap) != 0) * pairs + pair, gridDim.x * pairs};
}

}  // namespace hrx
