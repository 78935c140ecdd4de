// hrx_match_tile.h — the tile walk of the fused MATCH kernels (hrx_kernel_match.hip: padded input, hrx_kernel_ragged.hip: ragged input):
// one lane walks 64 rows of one string over every def and returns the tile's bitvectors and substr-id bytes; the kernels differ only in where
// the 64 input bytes come from.  Included after hrx_device.h and hrx_walk_pm.h.
#pragma once

namespace hrx {

// delta(state, byte) for the walk's current entry e (lib.rs:810)
template <bool GTAB, bool HALF>
__device__ __forceinline__ uint32_t match_next(const MatchArgs &a, uint32_t e, uint32_t c) {
    if (HALF) return lds_u16(half_next_addr(e, c << 1));
    const uint32_t off = (e & ~kTagMask) | (c << 2);
    return GTAB ? a.table_image[off >> 2] : lds_u32(off);
}
// the walk's entry -> the state it stands for, the narrow format's tag of the transition it came by, the entry of the first / padding rows
template <bool HALF> __device__ __forceinline__ uint32_t match_state(const MatchArgs &a, int d, uint32_t e) {
    return HALF ? (e & 0xffu) - a.dc[d].half_row_base : (e >> kNextShift) - a.dc[d].row_base;
}
template <bool HALF> __device__ __forceinline__ uint32_t match_tag(uint32_t e) { return HALF ? half_tag(e) : e & kTagMask; }
// an undefined transition: the narrow table's absorbing dead row is each def's last; a HALF entry marks it in its high byte (the walk then goes on from row 0)
template <bool HALF> __device__ __forceinline__ uint32_t match_dead(const MatchArgs &a, int d) { return HALF ? kHalfDead : a.dc[d].dead_entry; }

// byte p of the tile's substr-id bytes (four rows per dword) without an indexed register array (which would go to scratch memory)
__device__ __forceinline__ uint32_t sid_byte(const uint32_t (&sidq)[16], int p) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) w = (p >> 2) == j ? sidq[j] : w;
    return (w >> (8 * (p & 3))) & 0xffu;
}

// one 64-row tile of one lane: the walk of every def, the tile bitvectors, the substr-id bytes (sidq, four rows per dword) and nz (bit p: SID[t0 + p] != 0).
// FULL: every row of the tile is < n and < M - 1
template <int D, bool FULL, bool GTAB, bool HALF>
__device__ __forceinline__ TileBits match_walk_tile(const uint4 (&cq)[4], const MatchArgs &a, uint32_t (&e)[D], uint32_t (&mx)[D], uint32_t &sid_prev,
                                                    uint32_t &ov_row, uint32_t (&acc_state)[D], uint32_t t0, uint32_t n, uint64_t &nz, uint32_t (&sidq)[16]) {
    uint32_t st[2] = {0, 0}, en1[2] = {0, 0}, ch[2] = {0, 0}, z[2] = {0, 0};
    const uint32_t cw[16] = {cq[0].x, cq[0].y, cq[0].z, cq[0].w, cq[1].x, cq[1].y, cq[1].z, cq[1].w,
                             cq[2].x, cq[2].y, cq[2].z, cq[2].w, cq[3].x, cq[3].y, cq[3].z, cq[3].w};
#pragma unroll
    for (int i = 0; i < 16; ++i) sidq[i] = 0;
#pragma unroll
    for (int p = 0; p < 64; ++p) {
        const uint32_t r = t0 + (uint32_t)p;
        if (!FULL && r >= a.M) break;
        const uint32_t c = (cw[p >> 2] >> (8 * (p & 3))) & 0xffu;
        uint32_t sid = 0, stn = 0, enn = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            uint32_t tag = 0;
            if (FULL || r < n) {
                const uint32_t ne = match_next<GTAB, HALF>(a, e[d], c);
                mx[d] = max(mx[d], ne);                                   // reaching the dead row / a dead entry = an undefined transition (lib.rs:817)
                tag = match_tag<HALF>(ne);
                if (!FULL && r + 1 >= a.M) tag &= ~kTagEnd;               // end_enable of row M-1 is never assigned: lib.rs:501
                e[d] = ne;
            } else {
                if (r == n) acc_state[d] = match_state<HALF>(a, d, e[d]);            // the state at row n: lib.rs:437-457
                e[d] = HALF ? a.dc[d].half_row_base : a.dc[d].dummy_entry;           // rows > n carry no tag: lib.rs:404-418
            }
            sid += tag & 0xffu;
            stn += (tag >> 8) & 1u;
            enn += (tag >> 9) & 1u;
        }
        if (D > 1) {
            if (stn > 1) ov_row = min(ov_row, r);
            if (enn > 1) ov_row = min(ov_row, r + 1u);
        }
        st[p >> 5] |= (stn ? 1u : 0u) << (p & 31);
        en1[p >> 5] |= (enn ? 1u : 0u) << (p & 31);
        ch[p >> 5] |= (sid != sid_prev ? 1u : 0u) << (p & 31);
        z[p >> 5] |= (sid & 0xffu ? 1u : 0u) << (p & 31);
        sid_prev = sid;
        sidq[p >> 2] |= (sid & 0xffu) << (8 * (p & 3));
    }
    nz = (uint64_t)z[0] | ((uint64_t)z[1] << 32);
    TileBits tb;
    tb.st = (uint64_t)st[0] | ((uint64_t)st[1] << 32);
    tb.en1 = (uint64_t)en1[0] | ((uint64_t)en1[1] << 32);
    tb.ch = (uint64_t)ch[0] | ((uint64_t)ch[1] << 32);
    return tb;
}

}  // namespace hrx
