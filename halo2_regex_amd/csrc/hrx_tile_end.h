// hrx_tile_end.h — what every kernel of the witness family does when a 64-row tile's reveal masks are known (hrx_lane.h tile_masks):
// take an earlier optimistic end mask back, and assemble the tile's eight octets of masked rows.  Device-only.
//   callers: hrx_kernel_pm.hip (finisher; walker without finisher), hrx_kernel_pmd.hip (combiner), hrx_kernel_mp.hip (witness_combine_summary_kernel).
//   (The pp finisher and witness_combine_kernel keep their own text: NOTES_MEASUREMENTS.md §23.)
#pragma once
#include "hrx_walk_pm.h"

namespace hrx {

// ---- where the masked row r of string b lies -------------------------------------------------
// position-major [M/8][nb][8] u16 of the block of nb strings that starts at string blk0 (hrx_lane.h kPmBlock); q8 = ceil(M / 8)
struct PmBlockRows {
    uint16_t *masked;
    uint32_t blk0, nb;
    size_t q8;
    __device__ __forceinline__ size_t at(const uint32_t b, const uint32_t r) const { return ((size_t)blk0 * q8 + (size_t)(r >> 3) * nb + (b - blk0)) * 8u + (r & 7u); }
    // the wave zeroes rows [fs, end) of string b, a row per lane and step; dummy (kDbgFixToDummy, profiling only): the same stores, all on the string's first tile
    __device__ __forceinline__ void zero(const uint32_t b, const uint32_t fs, const uint32_t end, const uint32_t lane, const bool dummy) const {
        for (uint32_t r = fs + lane; r < end; r += 64u) masked[at(b, dummy ? (r & 63u) : r)] = 0;
    }
};
// string-major [B][pitch] u16
struct SmPitchRows {
    uint16_t *masked;
    size_t pitch;
    __device__ __forceinline__ void zero(const uint32_t b, const uint32_t fs, const uint32_t end, const uint32_t lane, const bool dummy) const {
        for (uint32_t r = fs + lane; r < end; r += 64u) masked[(size_t)b * pitch + (dummy ? (r & 63u) : r)] = 0;
    }
};
// one of the two, chosen at compile time (kernels with a string-major switch)
template <bool SM>
struct PmOrSmRows {
    PmBlockRows pm;
    SmPitchRows sm;
    __device__ __forceinline__ void zero(const uint32_t b, const uint32_t fs, const uint32_t end, const uint32_t lane, const bool dummy) const {
        if (SM) sm.zero(b, fs, end, lane, dummy);
        else pm.zero(b, fs, end, lane, dummy);
    }
};
// position-major, long ranges (the BYTE finisher: a random DFA's repairs reach back hundreds of rows): the rows up to the next octet border
// two bytes at a time (lanes 0 .. 6), then a whole octet — 16 bytes — per lane: 512 rows per store instruction (`end` is a multiple of 64;
// one row per lane took a store instruction, each touching eight lines, per 64 rows)
struct PmBlockOctets {
    PmBlockRows rows;
    __device__ __forceinline__ void zero(const uint32_t b, const uint32_t fs, const uint32_t end, const uint32_t lane, const bool dummy) const {
        const uint32_t o0 = (fs + 7u) >> 3, o1 = end >> 3;
        const uint32_t rh = fs + lane;
        if (rh < (o0 << 3)) rows.masked[rows.at(b, dummy ? (rh & 63u) : rh)] = 0;
        for (uint32_t o = o0 + lane; o < o1; o += 64u) {
            const uint32_t oo = dummy ? (o & 7u) : o;
            *reinterpret_cast<uint4 *>(reinterpret_cast<unsigned char *>(rows.masked) + ((size_t)rows.blk0 * rows.q8 + (size_t)oo * rows.nb + (b - rows.blk0)) * 16u) = make_uint4(0, 0, 0, 0);
        }
    }
};

// An earlier optimistic end_mask = 1 turned out wrong (hrx_lane.h; rare with real definitions): every lane whose string has such a range
// (`fix`, from row fix_start) is taken in turn and the whole wave zeroes that string's masked rows [fix_start, fix_end) — the rows before
// fix_end are in memory already.  b0 = the string of lane 0.  skip (kDbgSkipFixups, profiling only): leave them.
template <class Rows>
__device__ __forceinline__ void take_back_end_mask(const bool fix, const uint32_t fix_start, const uint32_t fix_end, const uint32_t b0, const uint32_t lane,
                                                   const Rows &rows, const bool dummy = false, const bool skip = false) {
    uint64_t fixm = __ballot(fix && fix_start < fix_end);
    if (skip) fixm = 0;
    while (fixm) {
        const int j = __ffsll((unsigned long long)fixm) - 1;
        fixm &= fixm - 1;
        const uint32_t fs = (uint32_t)__builtin_amdgcn_readlane((int)fix_start, j);
        rows.zero(b0 + (uint32_t)j, fs, fix_end, lane, dummy);
    }
}

// The masked rows of a tile (lib.rs:752-761): eight octets of 8 x {masked_char, masked_substr_id} from the tile's 16 raw dwords, its 16 dwords
// of substr-id bytes and its 64 mask bits; out(k, v) takes octet k.
template <class Out>
__device__ __forceinline__ void tile_octets(const uint32_t (&cw)[16], const uint32_t (&sid)[16], const uint64_t mask, Out &&out) {
    const uint32_t mlo = (uint32_t)mask, mhi = (uint32_t)(mask >> 32);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t mbyte = ((k < 4 ? mlo : mhi) >> (8 * (k & 3))) & 0xffu;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (mbyte) v = masked_octet(cw[2 * k], cw[2 * k + 1], sid[2 * k], sid[2 * k + 1], mbyte);
        out(k, v);
    }
}
// ... stored at mp + k * mstep, only the octets that exist ([ceil(M/8)][..][8]: octet k of the tile at row t0 exists if t0 + 8 k < M;
// all: the caller knows they all do); nt: streaming stores; enabled = !kDbgSkipMasked
__device__ __forceinline__ void store_tile_octets(const uint32_t (&cw)[16], const uint32_t (&sid)[16], const uint64_t mask, unsigned char *mp, const size_t mstep,
                                                  const bool all, const uint32_t t0, const uint32_t M, const bool nt, const bool enabled) {
    tile_octets(cw, sid, mask, [&](const int k, const uint4 &v) {
        if ((all || t0 + (uint32_t)k * 8u < M) && enabled) store16(mp + (size_t)k * mstep, v, nt);
    });
}

}  // namespace hrx
