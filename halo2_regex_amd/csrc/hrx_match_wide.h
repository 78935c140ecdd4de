// hrx_match_wide.h — the lane core of the fused MATCH walk for four to eight defs (hrx_kernel_match_wide.hip): one lane per string on
// the CLASS-WIDE image (hrx_lane.h, hrx_defs.cpp), no witness row written.
//   MatchWideArgs    the kernel's arguments: the image, its class LUTs, eight defs' constants, the outputs
//   WideAcc          what the sweeps of one tile add up: per-row substr-id sums, "some def" / "more than one def" starts and ends here
//   wide_sweep       one lane walks the tile's 64 rows over G defs side by side
//   MatchLaneWide    a lane's state for one string, MatchLane's life cycle (hrx_match_tile.h): reset, tile, finish
// match_walk_tile walks every def inside the row loop, so its 64-row unroll carries every def's chain; here the loops are turned round: defs outermost,
// G at a time, and what the rows need of all defs together is accumulated across the sweeps.
// The header is plain C++ over a table reader (Tab::lo, Tab::lut), as hrx_lane.h: hipcc compiles it for the kernel (the image in LDS), g++ for
// tests/host_cpp/test_match_wide_host.cpp (the image in memory, under the sanitizers); it is not a CPU fallback.  Arrays are indexed by unrolled loops
// only and every function is inlined into the kernel, so the state lives in registers (no scratch memory).
#pragma once
#include <stddef.h>

#include "hrx_defs.hpp"
#include "hrx_lane.h"

// full unrolling is what keeps the lane's arrays in registers on the device; the host build has no use for it (g++ does not know the pragma)
#if defined(__clang__)
#define HRX_UNROLL _Pragma("unroll")
#else
#define HRX_UNROLL
#endif

namespace hrx {

constexpr uint32_t kWideMaxDefs = 8;        // kMaxDefsPerLaunch (hrx_kernel.hpp): the status word's accept bits
struct MatchWideArgs {
    const uint8_t *cw_image;        // the CLASS-WIDE image (device copy of DefsSet::cw_image), staged to LDS offset 0
    uint32_t image_bytes;           // its size, 16-byte rounded
    uint32_t cw_lut_off;            // offset of def 0's 256-byte class LUT in it (value = column x 8)
    uint32_t B, M, D;
    uint64_t *status;
    uint32_t *span_counts;          // may be NULL
    uint64_t *spans;                // [B][max_spans], NULL when max_spans == 0
    uint32_t max_spans;
    DefConsts dc[kWideMaxDefs];     // DefsSet::cw_consts: first / dummy / dead entries are row << kCwRowShift
};

HRX_HD uint32_t wide_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
HRX_HD uint32_t wide_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// the fields of a CLASS-WIDE lo word.  Its 2-bit start / end counters hold one def's flag each: lo words are never summed here (four defs would overflow them)
constexpr uint32_t kWideSidMask = 0xffu, kWideFlagMask = 3u;
HRX_HD uint32_t wide_row(uint32_t e) { return e & kCwRowMask; }
HRX_HD uint32_t wide_state(const MatchWideArgs &a, int d, uint32_t e) { return (wide_row(e) >> kCwRowShift) - a.dc[d].row_base; }

// What the sweeps of one tile leave, bit p / field p <-> row t0 + p.  sid: the sums of the defs' substr ids, two rows a dword — 16-bit fields, so that eight
// defs' ids add up unmasked, as match_walk_tile's sum does (what `ch` compares); st / en: some def starts at the row / ends behind it, st2 / en2: more than one does
struct WideAcc {
    uint32_t sid[32];
    uint64_t st, st2, en, en2;
    HRX_HD void clear() {
HRX_UNROLL
        for (int i = 0; i < 32; ++i) sid[i] = 0;
        st = st2 = en = en2 = 0;
    }
    // a sweep's own bitvectors (some / more than one of ITS defs) join the earlier sweeps'
    HRX_HD void join(uint64_t s, uint64_t s2, uint64_t e, uint64_t e2) {
        st2 |= s2 | (st & s);
        st |= s;
        en2 |= e2 | (en & e);
        en |= e;
    }
    // the lowest row that two defs flag together: a start at row r, an end at row r + 1 (match_walk_tile's ov_row)
    HRX_HD uint32_t overlap_row(uint32_t ov_row, uint32_t t0) const {
        if (st2) ov_row = wide_min(ov_row, t0 + (uint32_t)ctz64(st2));
        if (en2) ov_row = wide_min(ov_row, t0 + (uint32_t)ctz64(en2) + 1u);
        return ov_row;
    }
    // after the last sweep: the tile's bitvectors, nz (bit p: SID[t0 + p] & 0xff != 0) and the substr-id bytes (sidq, four rows a dword).  ch compares the
    // unmasked sums, the first row's with sid_prev (the previous tile's last; rows the walk did not reach hold 0, as in match_walk_tile)
    HRX_HD TileBits bits(uint32_t &sid_prev, uint32_t rows, uint64_t &nz, uint32_t (&sidq)[16]) const {
        uint32_t ch[2] = {0, 0}, z[2] = {0, 0};
HRX_UNROLL
        for (int j = 0; j < 32; ++j) {
            const uint32_t lo = sid[j] & 0xffffu, hi = sid[j] >> 16;
            const uint32_t prev = j ? sid[j ? j - 1 : 0] >> 16 : sid_prev;       // (j ? :  keeps the unrolled index in range)
            const int p = 2 * j;
            ch[p >> 5] |= (lo != prev ? 1u : 0u) << (p & 31) | (hi != lo ? 2u : 0u) << (p & 31);
            z[p >> 5] |= (lo & 0xffu ? 1u : 0u) << (p & 31) | (hi & 0xffu ? 2u : 0u) << (p & 31);
        }
HRX_UNROLL
        for (int q = 0; q < 16; ++q) {
            const uint32_t a = sid[2 * q], b = sid[2 * q + 1];
            sidq[q] = (a & 0xffu) | ((a >> 8) & 0xff00u) | ((b & 0xffu) << 16) | ((b << 8) & 0xff000000u);
        }
        TileBits tb;
        tb.st = st;
        tb.en1 = en;
        tb.ch = (uint64_t)ch[0] | ((uint64_t)ch[1] << 32);
        if (rows < 64u) tb.ch &= (1ull << rows) - 1ull;      // (the walk stops at row M: no bit behind it)
        nz = (uint64_t)z[0] | ((uint64_t)z[1] << 32);
        sid_prev = sid[31] >> 16;       // (a tile of fewer than 64 rows ends at row M: no tile of the string follows it)
        return tb;
    }
};

// the status word of a string: the lowest def's undefined transition, then the overlap row, then the accept bits (the reference walks defs in order:
// lib.rs:806); ok = false: the run count is 0
template <int D>
HRX_HD uint64_t wide_status(const MatchWideArgs &a, const uint32_t *dead_row, const uint32_t *err_state, const uint32_t *err_char, uint32_t ov_row,
                            const uint32_t *acc_state, bool &ok) {
    uint64_t status = 0;
    bool done = false;
HRX_UNROLL
    for (int d = 0; d < D; ++d)
        if (!done && dead_row[d] != 0xffffffffu) { status = status_invalid((uint32_t)d, dead_row[d], err_state[d], err_char[d]); done = true; }
    if (!done && ov_row != 0xffffffffu) { status = status_overlap(ov_row); done = true; }
    if (!done) {
        uint32_t accept = 0;
HRX_UNROLL
        for (int d = 0; d < D; ++d) accept |= (acc_state[d] == a.dc[d].accepted_state ? 1u : 0u) << d;
        status = status_ok(accept);
    }
    ok = !done;
    return status;
}

// defs [S, S + G) of D over the tile's 64 rows, side by side.  Per def and row: the column from the def's class LUT (off the chain), the chain word = the entry's lo
// word at (row field | column), the running max of the row field (reaching the dead row = an undefined transition), the tag fields into the sums.  The hi word
// (the witness record) is never read.  FULL: every row of the tile is < n and < M - 1
template <int D, int G, int S, bool FULL, class Tab>
HRX_HD void wide_sweep(const Tab &tab, const MatchWideArgs &a, const uint32_t (&cw)[16], uint32_t (&e)[D], uint32_t (&mx)[D], uint32_t (&acc_state)[D], uint32_t t0,
                       uint32_t n, WideAcc &acc) {
    constexpr int N = S + G <= D ? G : D - S;
    uint32_t st[2] = {0, 0}, st2[2] = {0, 0}, en[2] = {0, 0}, en2[2] = {0, 0};
HRX_UNROLL
    for (int p = 0; p < 64; ++p) {
        const uint32_t r = t0 + (uint32_t)p;
        if (!FULL && r >= a.M) break;
        const uint32_t c = (cw[p >> 2] >> (8 * (p & 3))) & 0xffu;
        uint32_t sid = 0, stn = 0, enn = 0;
HRX_UNROLL
        for (int j = 0; j < N; ++j) {
            const int d = S + j;
            uint32_t w = 0;       // the transition's lo word; rows >= n carry no tag: lib.rs:404-418
            if (FULL || r < n) {
                const uint32_t ne = tab.lo(wide_row(e[d]) | tab.lut(a.cw_lut_off + 256u * (uint32_t)d + c));
                mx[d] = wide_max(mx[d], wide_row(ne));                   // lib.rs:817
                w = ne;
                if (!FULL && r + 1 >= a.M) w &= ~(kWideFlagMask << kWideEndShift);      // end_enable of row M-1 is never assigned: lib.rs:501
                e[d] = ne;
            } else {
                if (r == n) acc_state[d] = wide_state(a, d, e[d]);      // the state at row n: lib.rs:437-457
                e[d] = a.dc[d].dummy_entry;
            }
            sid += (w >> kWideSidShift) & kWideSidMask;
            stn += (w >> kWideStartShift) & kWideFlagMask;
            enn += w >> kWideEndShift;
        }
        acc.sid[p >> 1] += sid << (16 * (p & 1));
        st[p >> 5] |= (stn ? 1u : 0u) << (p & 31);
        en[p >> 5] |= (enn ? 1u : 0u) << (p & 31);
        if (N > 1) {
            st2[p >> 5] |= (stn > 1u ? 1u : 0u) << (p & 31);
            en2[p >> 5] |= (enn > 1u ? 1u : 0u) << (p & 31);
        }
    }
    acc.join((uint64_t)st[0] | ((uint64_t)st[1] << 32), (uint64_t)st2[0] | ((uint64_t)st2[1] << 32), (uint64_t)en[0] | ((uint64_t)en[1] << 32),
             (uint64_t)en2[0] | ((uint64_t)en2[1] << 32));
}
template <int D, int G, int S, bool FULL, class Tab>
HRX_HD void wide_sweeps(const Tab &tab, const MatchWideArgs &a, const uint32_t (&cw)[16], uint32_t (&e)[D], uint32_t (&mx)[D], uint32_t (&acc_state)[D], uint32_t t0,
                        uint32_t n, WideAcc &acc) {
    wide_sweep<D, G, S, FULL>(tab, a, cw, e, mx, acc_state, t0, n, acc);
    if constexpr (S + G < D) wide_sweeps<D, G, S + G, FULL>(tab, a, cw, e, mx, acc_state, t0, n, acc);
}

// one lane's walk of one string
template <int D, int G>
struct MatchLaneWide {
    uint32_t e[D], mx[D], acc_state[D], dead_row[D], err_state[D], err_char[D];
    uint32_t sid_prev, ov_row;
    MaskCarry mc;
    SpanEmitter em;
    uint64_t *slots;        // the string's run slots (NULL: none)

    // the start of string b
    HRX_HD void reset(const MatchWideArgs &a, size_t b) {
HRX_UNROLL
        for (int d = 0; d < D; ++d) {
            e[d] = a.dc[d].first_entry;       // states[d][0] = first_state_val: lib.rs:807
            mx[d] = 0;
            acc_state[d] = a.dc[d].first_state;
            dead_row[d] = 0xffffffffu;
            err_state[d] = err_char[d] = 0;
        }
        sid_prev = 0;
        ov_row = 0xffffffffu;
        mc = MaskCarry{0, 0, 0, 0};
        em.init();
        slots = a.spans ? a.spans + b * a.max_spans : nullptr;
    }

    // rows [t0, t0 + 64) of a string of n bytes: cw holds the tile's bytes (zero past n), byte_at(r) is byte r < n of the string.
    // full: every row of the tile is < n and < M - 1 (the caller may pass false for such a tile: the general walk gives the same bits).
    // last: no tile of this string is walked after this one
    template <class Tab, class ByteAt>
    HRX_HD void tile(const Tab &tab, const MatchWideArgs &a, const uint32_t (&cw)[16], uint32_t t0, uint32_t n, bool last, bool full, const ByteAt &byte_at) {
        const uint32_t M = a.M;
        uint32_t e0[D], mx0[D];
HRX_UNROLL
        for (int d = 0; d < D; ++d) { e0[d] = e[d]; mx0[d] = mx[d]; }
        WideAcc acc;
        acc.clear();
        if (full) wide_sweeps<D, G, 0, true>(tab, a, cw, e, mx, acc_state, t0, n, acc);
        else wide_sweeps<D, G, 0, false>(tab, a, cw, e, mx, acc_state, t0, n, acc);
        ov_row = acc.overlap_row(ov_row, t0);
        uint64_t nz;
        uint32_t sidq[16];
        const TileBits tb = acc.bits(sid_prev, wide_min(64u, M - t0), nz, sidq);
        // the first undefined transition of a def (rare: the tile is walked again row by row to find its row, state and byte)
HRX_UNROLL
        for (int d = 0; d < D; ++d) {
            if (dead_row[d] == 0xffffffffu && mx[d] >= a.dc[d].dead_entry && mx0[d] < a.dc[d].dead_entry) {
                uint32_t x = e0[d];
                for (uint32_t p = 0; p < 64u && t0 + p < n; ++p) {
                    const uint32_t ch = byte_at(t0 + p);
                    const uint32_t ne = tab.lo(wide_row(x) | tab.lut(a.cw_lut_off + 256u * (uint32_t)d + ch));
                    if (wide_row(ne) >= a.dc[d].dead_entry) {
                        dead_row[d] = t0 + p;
                        err_state[d] = wide_state(a, d, x);
                        err_char[d] = ch;
                        break;
                    }
                    x = ne;
                }
            }
        }
        if (n == M && last) {   // n == M: row n does not exist, s[n] is the live state
HRX_UNROLL
            for (int d = 0; d < D; ++d) acc_state[d] = wide_state(a, d, e[d]);
        }
        // reveal masks (lib.rs:598-764) and the runs they make
        const TileMasks tm = tile_masks<64>(tb, mc, t0, tile_is_exact(t0, n, M), rows_below(t0, n));
        SpanSlots out{slots, a.max_spans};
        if (a.max_spans || a.span_counts) em.tile(tm, mc, tb.ch, nz, t0, wide_min(64u, M - t0), [&](int p) { return wide_sid_byte(sidq, p); }, out);
    }

    // byte p of the tile's substr-id bytes without an indexed register array (sid_byte of hrx_match_tile.h)
    static HRX_HD uint32_t wide_sid_byte(const uint32_t (&sidq)[16], int p) {
        uint32_t w = 0;
HRX_UNROLL
        for (int j = 0; j < 16; ++j) w = (p >> 2) == j ? sidq[j] : w;
        return (w >> (8 * (p & 3))) & 0xffu;
    }

    // after the last tile: the status word and the run count of string b
    HRX_HD void finish(const MatchWideArgs &a, size_t b) {
        SpanSlots out{slots, a.max_spans};
        em.finish(a.M, out);
        bool ok;
        a.status[b] = wide_status<D>(a, dead_row, err_state, err_char, ov_row, acc_state, ok);
        if (a.span_counts) a.span_counts[b] = ok ? em.count : 0u;
    }
};

}  // namespace hrx
