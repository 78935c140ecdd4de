// hrx_match_tile.h — the lane core of the fused MATCH kernels (hrx_kernel_match.hip: padded input, hrx_kernel_ragged.hip: ragged input).
//   match_stage_table   the table into LDS, once per workgroup
//   match_walk_tile     one lane walks 64 rows of one string over every def and returns the tile's bitvectors and substr-id bytes
//   MatchLane           a lane's state for one string: reset, one tile (walk, first undefined transition, masks, runs), finish (status word, count)
//   fused_kernel<K>     host side: the launch ladder of both kernels, D x {narrow LDS, HALF, global table} with the dynamic-LDS grant
// The kernels keep what differs: where a tile's 64 input bytes come from, the loop around the tile and the FULL decision.  MatchLane's arrays are
// indexed by unrolled loops only and every member function is inlined into the kernel, so the state lives in registers (no scratch memory).
// Included after hrx_device.h and hrx_walk_pm.h.
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

// the table at LDS offset 0 (the kernels declare no static LDS)
template <bool GTAB, bool HALF>
__device__ __forceinline__ void match_stage_table(const MatchArgs &a) {
    if (GTAB) return;
    const uint32_t tab16 = (a.table_bytes + 15u) & ~15u;
    const uint8_t *img = HALF ? reinterpret_cast<const uint8_t *>(a.half_image) : reinterpret_cast<const uint8_t *>(a.table_image);
    for (uint32_t i = threadIdx.x * 16u; i < tab16; i += blockDim.x * 16u)
        *reinterpret_cast<uint4 *>(smem + i) = *reinterpret_cast<const uint4 *>(img + i);
    __syncthreads();
}

// one lane's walk of one string
template <int D, bool GTAB, bool HALF>
struct MatchLane {
    uint32_t e[D], mx[D], acc_state[D], dead_row[D], err_state[D], err_char[D];
    uint32_t sid_prev, ov_row;
    MaskCarry mc;
    SpanEmitter em;
    uint64_t *slots;        // the string's run slots (NULL: none)

    // the start of string b
    __device__ __forceinline__ void reset(const MatchArgs &a, size_t b) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            e[d] = HALF ? a.dc[d].half_row_base + a.dc[d].first_state : a.dc[d].first_entry;       // states[d][0] = first_state_val: lib.rs:807
            mx[d] = 0;
            acc_state[d] = a.dc[d].first_state;
            dead_row[d] = 0xffffffffu;
        }
        sid_prev = 0;
        ov_row = 0xffffffffu;
        mc = MaskCarry{0, 0, 0, 0};
        em.init();
        slots = a.spans ? a.spans + b * a.max_spans : nullptr;
    }

    // rows [t0, t0 + 64) of a string of n bytes: cq holds the tile's bytes (zero past n), byte_at(r) is byte r < n of the string.
    // full: every row of the tile is < n and < M - 1 (the caller may pass false for such a tile: the general walk gives the same bits).
    // last: no tile of this string is walked after this one
    template <class ByteAt>
    __device__ __forceinline__ void tile(const MatchArgs &a, const uint4 (&cq)[4], uint32_t t0, uint32_t n, bool last, bool full, const ByteAt &byte_at) {
        const uint32_t M = a.M;
        uint32_t e0[D], mx0[D];
#pragma unroll
        for (int d = 0; d < D; ++d) { e0[d] = e[d]; mx0[d] = mx[d]; }
        uint64_t nz;
        uint32_t sidq[16];
        const TileBits tb = full ? match_walk_tile<D, true, GTAB, HALF>(cq, a, e, mx, sid_prev, ov_row, acc_state, t0, n, nz, sidq)
                                 : match_walk_tile<D, false, GTAB, HALF>(cq, a, e, mx, sid_prev, ov_row, acc_state, t0, n, nz, sidq);
        // the first undefined transition of a def (rare: the tile is walked again row by row to find its row, state and byte)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (dead_row[d] == 0xffffffffu && mx[d] >= match_dead<HALF>(a, d) && mx0[d] < match_dead<HALF>(a, d)) {
                uint32_t x = e0[d];
                for (uint32_t p = 0; p < 64u && t0 + p < n; ++p) {
                    const uint32_t ch = byte_at(t0 + p);
                    const uint32_t ne = match_next<GTAB, HALF>(a, x, ch);
                    if (ne >= match_dead<HALF>(a, d)) {
                        dead_row[d] = t0 + p;
                        err_state[d] = match_state<HALF>(a, d, x);
                        err_char[d] = ch;
                        break;
                    }
                    x = ne;
                }
            }
        }
        if (n == M && last) {   // n == M: row n does not exist, s[n] is the live state
#pragma unroll
            for (int d = 0; d < D; ++d) acc_state[d] = match_state<HALF>(a, d, e[d]);
        }
        // reveal masks (lib.rs:598-764) and the runs they make
        const TileMasks tm = tile_masks<64>(tb, mc, t0, tile_is_exact(t0, n, M), rows_below(t0, n));
        SpanSlots out{slots, a.max_spans};
        if (a.max_spans || a.span_counts) em.tile(tm, mc, tb.ch, nz, t0, min(64u, M - t0), [&](int p) { return sid_byte(sidq, p); }, out);
    }

    // after the last tile: the status word and the run count of string b
    __device__ __forceinline__ void finish(const MatchArgs &a, size_t b) {
        SpanSlots out{slots, a.max_spans};
        em.finish(a.M, out);
        uint64_t status = 0;
        bool done = false;
#pragma unroll
        for (int d = 0; d < D; ++d)   // lowest def wins: the reference walks defs in order (lib.rs:806)
            if (!done && dead_row[d] != 0xffffffffu) { status = status_invalid((uint32_t)d, dead_row[d], err_state[d], err_char[d]); done = true; }
        if (!done && D > 1 && ov_row != 0xffffffffu) { status = status_overlap(ov_row); done = true; }
        if (!done) {
            uint32_t accept = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) accept |= (acc_state[d] == a.dc[d].accepted_state ? 1u : 0u) << d;
            status = status_ok(accept);
        }
        a.status[b] = status;
        if (a.span_counts) a.span_counts[b] = done ? 0u : em.count;
    }
};

// the kernel a fused launch runs: K::get<D, GTAB, HALF>() for the plan's table form, with the plan's dynamic LDS granted (host side; K names
// one of the two kernel templates, K::fn is its function-pointer type)
template <class K, int D, bool GTAB, bool HALF>
static hipError_t fused_kernel_one(const MatchPlan &p, typename K::fn &k) {
    static std::atomic<size_t> granted{0};
    k = K::template get<D, GTAB, HALF>();
    return p.lds_bytes ? ensure_lds(k, granted, p.lds_bytes) : hipSuccess;
}
template <class K, int D>
static hipError_t fused_kernel_d(const MatchPlan &p, typename K::fn &k) {
    if (p.half) return fused_kernel_one<K, D, false, true>(p, k);
    if (p.gtab) return fused_kernel_one<K, D, true, false>(p, k);
    return fused_kernel_one<K, D, false, false>(p, k);
}
template <class K>
static hipError_t fused_kernel(uint32_t D, const MatchPlan &p, typename K::fn &k) {
    switch (D) {
    case 1: return fused_kernel_d<K, 1>(p, k);
    case 2: return fused_kernel_d<K, 2>(p, k);
    case 3: return fused_kernel_d<K, 3>(p, k);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace hrx
