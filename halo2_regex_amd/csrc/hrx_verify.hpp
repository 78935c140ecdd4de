// hrx_verify.hpp — the rules of VERIFY (include/hrx.h: hrx_verify_rows_device* / hrx_verify_rows_host) that must exist once: which gate, lookup or assignment
// rule of RegexVerifyConfig::configure (src/lib.rs:126-305), of the accept chain (lib.rs:427-457) and of the reveal gates (lib.rs:593-764) a witness row breaks.
// No HIP dependency: the kernels (hrx_kernel_verify.hip), the host forms (hrx_verify_host.cpp) and tests/host_cpp/test_verify_host.cpp /
// test_verify_chunk_host.cpp all include it.  The chunked rule — a summary per chunk of a string's rows and a fold of the summaries — follows verify_lane.
//
// The checker shares nothing with the walk: its tables are built from the rows RegexTableConfig::load assigns (src/table.rs:61-198; table_transition_rows /
// table_endpoint_rows of hrx_defs.cpp) and it is handed state[r], state[r + 1], char[r] and the tags of every row, so every lookup stands alone.
//
// A row r is judged once row r + 1 is known (Rotation::next); row M - 1 is judged against the cell nobody assigns (the dummy state, no flags).  Per string:
//   VerifyAcc acc;  verify_begin(acc)
//   sums[0] = sum over the defs of verify_sums_of(rec[0][d], 0 < n)
//   for r = 0 .. M - 1:   for every def: verify_def_row(..., r, rec[r][d], state of rec[r + 1][d] or the dummy);  sums[r + 1] likewise (+ verify_end_sum(rec[r][d]) if r + 1 < M)
//                         verify_mask_row(acc, r, char[r], masked[r], sums[r], sums[r + 1])        (sums[M] = 0)
//   verdict = verify_finish(acc)
// verify_string below is exactly that loop over an accessor; the kernel runs it tile by tile with the rows in registers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hrx_rows.hpp"        // HRX_XHD, RowsIn: the rows the rules are run over

#if defined(__clang__)
#define HRX_VFY_UNROLL _Pragma("unroll")     // the tile loops index register arrays: every index a constant once unrolled
#else
#define HRX_VFY_UNROLL
#endif

namespace hrx {

// the verdict word's check bits (= HRX_VERIFY_* of include/hrx.h = FAIL_* of tests/mock_prover.py)
constexpr uint32_t kVfyFirstState = 1, kVfyEnable = 2, kVfyTransition = 4, kVfyStartLookup = 8, kVfyEndLookup = 16, kVfyAccept = 32;
constexpr uint32_t kVfyFlags = 64, kVfyPadding = 128, kVfyMask = 256;
constexpr uint32_t kVfyRowShift = 32;               // bits 32..56: the lowest row at which a reported check fails
constexpr uint32_t kVfyNoRow = 0xffffffffu;
constexpr uint32_t kVfyNoEntry = 0xffffffffu;       // transition array: no row (char, cur) in the table

// One def's tables inside the image (all offsets in u32 words from the image's start).  The image is [D] VerifyDef, then every def's arrays:
//   tab    [ns][256] u32   next | substr_id << 16 of transition row (char, cur), kVfyNoEntry where the table has none
//   start  bitset [nsid][ns]   (substr_id, state, dummy) is an endpoint row (serves the start lookup)
//   end    bitset [nsid][ns]   (substr_id, dummy, state) is an endpoint row (serves the end lookup)
struct VerifyDef {
    uint32_t tab, start, end;
    uint32_t ns, nsid;                  // states 0 .. dummy; substr ids 0 .. the largest in the endpoint rows
    uint32_t dummy, first, accepted;
};
constexpr uint32_t kVfyDefWords = sizeof(VerifyDef) / 4;

// what a string's check carries from row to row (eight words: O(1) whatever M is)
struct VerifyAcc {
    uint32_t bits, row;                 // the failed checks but the masked rows, the lowest row of any of them
    uint32_t start_mask, prev_sid;      // reveal gates, forward scan (lib.rs:593-680)
    uint32_t need1, need0;              // lowest masked row since the last backward event that is right iff end_mask is 1 / iff it is 0
    uint32_t mask_row;                  // lowest masked row known to be wrong
    uint32_t overlap;                   // two defs flag one row: the masked rows are out of contract, their check is not reported
};

HRX_XHD void verify_begin(VerifyAcc &a) {
    a.bits = 0; a.row = kVfyNoRow;
    a.start_mask = 0; a.prev_sid = 0;
    a.need1 = kVfyNoRow; a.need0 = kVfyNoRow; a.mask_row = kVfyNoRow;
    a.overlap = 0;
}

HRX_XHD uint32_t vfy_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
HRX_XHD uint32_t vfy_bit(const uint32_t *bits, uint32_t i) { return (bits[i >> 5] >> (i & 31u)) & 1u; }

// A row's sums over the defs, one word: Sum(substr_id * enable) (lib.rs:467-471) | Sum(start_enable) << 16 | Sum(end_enable of the row before) << 24.
// What record x of row r adds to the sums of row r ...
HRX_XHD uint32_t verify_sums_of(uint32_t x, bool enabled) { return (enabled ? (x >> 16) & 0xffu : 0u) | ((x >> 24) & 1u) << 16; }
// ... and to those of row r + 1 (lib.rs:501-519: end_enable[r] lands on EN[r + 1], r = 0 .. M - 2)
HRX_XHD uint32_t verify_end_sum(uint32_t x) { return ((x >> 25) & 1u) << 24; }

// Every check of one def on row r, in two steps so that a caller with many rows in hand can issue all their lookups before it judges any:
// verify_def_look says where the row's three lookups lie (always inside the image, whatever the row holds), verify_def_judge takes what lies there.
// c = enable[r] * char[r]; x = the def's record of row r; next_state = the state of row r + 1, the def's dummy where r + 1 == M.
struct VerifyLook {
    uint32_t tab, start, end;           // word indices into the image: the transition entry of (state, c); the words of the two membership bits
};
HRX_XHD VerifyLook verify_def_look(const VerifyDef &T, uint32_t c, uint32_t x, uint32_t next_state) {
    const uint32_t state = x & 0xffffu, sid = (x >> 16) & 0xffu;
    const uint32_t row0 = (sid < T.nsid ? sid : 0u) * T.ns;
    VerifyLook k;
    k.tab = T.tab + (state < T.ns ? state : T.dummy) * 256u + c;
    k.start = T.start + ((row0 + (state < T.ns ? state : 0u)) >> 5);
    k.end = T.end + ((row0 + (next_state < T.ns ? next_state : 0u)) >> 5);
    return k;
}
// e, sw, ew: the image's words at the three indices.  Straight-line code: every rule is evaluated on every row and masked by the row's kind
HRX_XHD void verify_def_judge(const VerifyDef &T, uint32_t r, uint32_t n, uint32_t M, uint32_t x, uint32_t next_state, uint32_t e, uint32_t sw, uint32_t ew,
                              VerifyAcc &a) {
    const bool en = r < n, last = r + 1u == M;
    const uint32_t state = x & 0xffffu, sid = (x >> 16) & 0xffu, fl = x >> 24, se = fl & 1u, ee = (fl >> 1) & 1u;
    const bool last_unassigned = last && en;    // n == M: Rotation::next of row M - 1 is a cell match_substrs never assigns
    const bool sid_in = sid < T.nsid, st_in = state < T.ns, nx_in = next_state < T.ns;
    const uint32_t row0 = (sid_in ? sid : 0u) * T.ns;
    const uint32_t sbit = (sw >> ((row0 + (st_in ? state : 0u)) & 31u)) & 1u, ebit = (ew >> ((row0 + (nx_in ? next_state : 0u)) & 31u)) & 1u;
    uint32_t bits = 0;
    // gate "The state must start from the first state value" (lib.rs:173-191)
    bits |= r == 0 && en && state != T.first ? kVfyFirstState : 0u;
    // gate "The transition of enable flags" (lib.rs:193-205): enable is [r < n], boolean and never rising; kept so that the checker mirrors verify() gate for gate
    const int chg = (int)en - (int)(r + 1u < n);
    bits |= !last && chg * (1 - chg) != 0 ? kVfyEnable : 0u;
    // lookup "characters and their state" (lib.rs:207-233).  A disabled row looks (0, dummy, dummy, 0) up: the table's first row (build_verify_image checks it)
    bits |= en && !last_unassigned && !(st_in && e == (next_state | sid << 16)) ? kVfyTransition : 0u;
    // lookups "start_state of substring" / "end_state of substring" (lib.rs:235-284): a row without the flag looks the dummy endpoint row up
    bits |= se && !(sid_in && st_in && sbit) ? kVfyStartLookup : 0u;
    bits |= ee && !last_unassigned && !(sid_in && nx_in && ebit) ? kVfyEndLookup : 0u;
    // beyond verify(): the flags are exactly derive_is_start_end's (lib.rs:847-888; the lookups clamp what is out of range, as the torch checker does) gated by
    // enable (lib.rs:482-519); lib.rs:501: the end flags stop at row M - 2
    const bool tagged = en && sid != 0;
    const uint32_t exp_se = tagged ? sbit : 0u, exp_ee = tagged && !last ? ebit : 0u;
    bits |= exp_se != se || exp_ee != ee ? kVfyFlags : 0u;
    // accept chain (lib.rs:427-457): at the row where enable drops (pre = 1 at row 0) the state is the accepted one
    bits |= r == n && state != T.accepted ? kVfyAccept : 0u;
    // padding (lib.rs:387-418): no tag and no flag from row n on, the dummy state after row n; flag bits above the two that exist
    bits |= fl > 3u || (!en && (sid != 0 || fl != 0)) || (r > n && state != T.dummy) ? kVfyPadding : 0u;
    a.bits |= bits;
    a.row = bits ? vfy_min(a.row, r) : a.row;
}
HRX_XHD void verify_def_row(const uint32_t *img, const VerifyDef &T, uint32_t r, uint32_t n, uint32_t M, uint32_t c, uint32_t x, uint32_t next_state, VerifyAcc &a) {
    const VerifyLook k = verify_def_look(T, c, x, next_state);
    verify_def_judge(T, r, n, M, x, next_state, img[k.tab], img[k.start], img[k.end], a);
}

// The masked row r against the reveal gates (lib.rs:593-764) evaluated on the records' own sums: mask = start_mask * end_mask,
//   start_mask[r]: the last forward event at a row <= r decides (set: a start flag where the tag changes; reset: an end flag and no start flag there),
//   end_mask[r]:   the first backward event at a row p >= r decides (set: EN[p + 1] where the tag changes behind p; reset: ST[p + 1] and no EN[p + 1] there),
// no event: 0.  Walking forward, end_mask of the rows since the last backward event is not known yet: such a row is filed under what it needs
// (need1 / need0, the lowest row each) and judged by the next backward event, or by the end of the rows (no event: 0).
// c = enable[r] * char[r], got = the masked cell, s / sn = the sums of rows r and r + 1 (row M: 0).
HRX_XHD void verify_mask_row(VerifyAcc &a, uint32_t r, uint32_t c, uint32_t got, uint32_t s, uint32_t sn) {
    const uint32_t sid = s & 0xffffu, st = (s >> 16) & 0xffu, en = s >> 24;
    const uint32_t sidn = sn & 0xffffu, stn = (sn >> 16) & 0xffu, enn = sn >> 24;
    if (st > 1u || en > 1u) a.overlap = 1u;
    if (a.prev_sid != sid) {                       // pre_substr_id = 0 at row 0
        if (st) a.start_mask = 1u;
        else if (en) a.start_mask = 0u;
    }
    a.prev_sid = sid;
    const uint32_t e = c | sid << 8;               // what the cell holds where the mask is 1
    if (a.start_mask && got == 0u) {
        if (e != 0u) a.need0 = vfy_min(a.need0, r);
    } else if (a.start_mask && got == e) {
        a.need1 = vfy_min(a.need1, r);
    } else if (got != 0u) {
        a.mask_row = vfy_min(a.mask_row, r);       // neither 0 nor the revealed cell, or revealed outside every range
    }
    if (sidn != sid) {
        if (enn) {                                 // set: end_mask = 1 back to the previous event
            a.mask_row = vfy_min(a.mask_row, a.need0);
            a.need0 = a.need1 = kVfyNoRow;
        } else if (stn) {                          // reset
            a.mask_row = vfy_min(a.mask_row, a.need1);
            a.need0 = a.need1 = kVfyNoRow;
        }
    }
}

HRX_XHD uint64_t verify_finish(const VerifyAcc &a) {
    uint32_t bits = a.bits, row = a.row;
    const uint32_t mask_row = vfy_min(a.mask_row, a.need1);     // no event behind them: end_mask = 0
    if (!a.overlap && mask_row != kVfyNoRow) {
        bits |= kVfyMask;
        row = vfy_min(row, mask_row);
    }
    return bits ? (uint64_t)bits | (uint64_t)row << kVfyRowShift : 0ull;
}

// One string of n <= M characters over an accessor: src.chr(r) (r < n only), src.rec(r, d), src.msk(r).  n > M: all ones (the string has no rows).
template <class Src>
inline uint64_t verify_string(const uint32_t *img, uint32_t D, uint32_t n, uint32_t M, const Src &src) {
    if (n > M) return ~0ull;
    const VerifyDef *defs = reinterpret_cast<const VerifyDef *>(img);
    VerifyAcc a;
    verify_begin(a);
    uint32_t s = 0;
    for (uint32_t d = 0; d < D; ++d) s += verify_sums_of(src.rec(0, d), 0 < n);
    for (uint32_t r = 0; r < M; ++r) {
        const uint32_t c = r < n ? src.chr(r) : 0u;
        uint32_t sn = 0;
        for (uint32_t d = 0; d < D; ++d) {
            const uint32_t x = src.rec(r, d);
            uint32_t next_state = defs[d].dummy;
            if (r + 1u < M) {
                const uint32_t xn = src.rec(r + 1u, d);
                next_state = xn & 0xffffu;
                sn += verify_sums_of(xn, r + 1u < n) + verify_end_sum(x);
            }
            verify_def_row(img, defs[d], r, n, M, c, x, next_state, a);
        }
        verify_mask_row(a, r, c, src.msk(r), s, sn);
        s = sn;
    }
    return verify_finish(a);
}

// The same loop as the kernel runs it: tile by tile, T rows at a time, over a source of whole tiles —
//   src.chars(base, c[T])        enable * char of rows base .. base + T - 1
//   src.masked(base, mk[T])      their masked cells            (rows >= M: anything, never judged)
//   src.records(d, base, x[T])   def d's records of those rows (likewise)
//   src.record(d, r)             def d's record of row r < M alone
// — every load of a tile issued before any of it is consumed.  Row r is judged when row r + 1 is there, so one row is carried from tile to tile: its
// byte, masked cell and sums, and with DT > 0 (the config's DT defs, the tile's records all in registers) every def's record.  DT == 0: any number of
// defs, one after the other, the record before the tile read again (a carried one would be an array indexed by the def: no such thing in registers).
// n <= M.  tests/host_cpp/test_verify_host.cpp runs this loop on the host against verify_string.
template <int DT, int T, class Tiles>
HRX_XHD uint64_t verify_lane(const uint32_t *img, const uint32_t Dn, const uint32_t n, const uint32_t M, const Tiles &src) {
    const uint32_t D = DT ? (uint32_t)DT : Dn;
    const VerifyDef *defs = reinterpret_cast<const VerifyDef *>(img);
    VerifyAcc acc;
    verify_begin(acc);
    uint32_t c_prev = 0, mk_prev = 0, s_prev = 0;
    uint32_t x_prev[DT ? DT : 1] = {};
    for (uint32_t base = 0; base < M; base += T) {
        uint32_t c[T], mk[T], x[DT ? DT : 1][T], sums[T];
        src.chars(base, c);
        src.masked(base, mk);
        if constexpr (DT > 0) {
HRX_VFY_UNROLL
            for (int d = 0; d < DT; ++d) src.records((uint32_t)d, base, x[d]);
        }
HRX_VFY_UNROLL
        for (int j = 0; j < T; ++j) sums[j] = 0;
        // def d over the tile: xd its records, xp its record of the row before the tile; returns its record of the tile's last row below M
        auto def_tile = [&](const uint32_t d, const uint32_t(&xd)[T], uint32_t xp) {
            const VerifyDef def = defs[d];
            // the lookups of every row the tile judges, all issued before any is used (rows that do not exist look the dummy row up)
            uint32_t e[T], sw[T], ew[T];
HRX_VFY_UNROLL
            for (int j = 0; j < T; ++j) {
                const bool live = base + j < M && base + j > 0;
                const VerifyLook k = verify_def_look(def, live ? (j ? c[j ? j - 1 : 0] : c_prev) : 0u, live ? (j ? xd[j ? j - 1 : 0] : xp) : def.dummy, live ? xd[j] & 0xffffu : 0u);
                e[j] = img[k.tab]; sw[j] = img[k.start]; ew[j] = img[k.end];
            }
HRX_VFY_UNROLL
            for (int j = 0; j < T; ++j) {
                const uint32_t r1 = base + j;          // the row xd[j] holds; row r1 - 1 is judged
                if (r1 < M) {
                    sums[j] += verify_sums_of(xd[j], r1 < n);
                    if (r1 > 0) {
                        sums[j] += verify_end_sum(xp);
                        verify_def_judge(def, r1 - 1u, n, M, xp, xd[j] & 0xffffu, e[j], sw[j], ew[j], acc);
                    }
                    xp = xd[j];
                }
            }
            return xp;
        };
        if constexpr (DT > 0) {
HRX_VFY_UNROLL
            for (int d = 0; d < DT; ++d) x_prev[d] = def_tile((uint32_t)d, x[d], x_prev[d]);
        } else {
            for (uint32_t d = 0; d < D; ++d) {
                src.records(d, base, x[0]);
                def_tile(d, x[0], base ? src.record(d, base - 1u) : 0u);
            }
        }
HRX_VFY_UNROLL
        for (int j = 0; j < T; ++j) {
            const uint32_t r1 = base + j;
            if (r1 < M) {
                if (r1 > 0) verify_mask_row(acc, r1 - 1u, c_prev, mk_prev, s_prev, sums[j]);
                c_prev = c[j]; mk_prev = mk[j]; s_prev = sums[j];
            }
        }
    }
    // row M - 1 against the cell nobody assigns
    if constexpr (DT > 0) {
HRX_VFY_UNROLL
        for (int d = 0; d < DT; ++d) verify_def_row(img, defs[d], M - 1u, n, M, c_prev, x_prev[d], defs[d].dummy, acc);
    } else {
        for (uint32_t d = 0; d < D; ++d) verify_def_row(img, defs[d], M - 1u, n, M, c_prev, src.record(d, M - 1u), defs[d].dummy, acc);
    }
    verify_mask_row(acc, M - 1u, c_prev, mk_prev, s_prev, 0u);
    return verify_finish(acc);
}

// ---- the same verdict out of CHUNKS of a string's rows (hrx_verify_rows_chunked_*): chunk k judges rows [r0, r1) = [k C, min(M, (k + 1) C)) on its own,
// leaves a summary, and verify_fold_chunk folds the summaries of a string in row order into a VerifyAcc that verify_finish turns into verify_string's word.
// Every def check is a function of rows r and r + 1 alone: bits, row and overlap fold by OR, min and OR.  The reveal mask carries state both ways:
//   forward   start_mask at r0 is decided by an event before the chunk, which the chunk cannot see: it runs verify_mask_row's classification under both
//             hypotheses h = 0, 1 (from prev_sid of row r0 - 1, nothing pending) and leaves mask_row[h], need1[h], need0[h] as they stand at r1, and what its
//             LAST forward event did to start_mask (the same under both: an event overrides the hypothesis);
//   backward  rows pending from before the chunk are resolved by its FIRST backward event, which the summary names.
// A chunk reads rows r0 - 1 .. r1: the row before for prev_sid and the end_enable share of row r0's sums, the row behind for Rotation::next and the sums
// that decide the backward event at row r1 - 1 (r1 == M: the cell nobody assigns, sums 0).  Rows are absolute, so every min is order-free.
constexpr uint32_t kVfyChunkAlign = 32;             // chunk_rows is a multiple of this: whole tiles of every T, whole quads, octets and 16-byte input chunks
constexpr uint32_t kVfyChunkFields = 8;             // u32 words of a summary; the workspace holds them field by field: word f of (chunk k, string b) at (f K + k) B + b
constexpr uint32_t kVfyEvNone = 0, kVfyEvSet = 1, kVfyEvReset = 2;
constexpr uint32_t kVfyChunkOverlap = 1u << 9, kVfyChunkFwdShift = 10, kVfyChunkBackShift = 12;

struct VerifyChunk {
    uint32_t flags;                     // the failed def checks (bits 0..8) | overlap << 9 | last forward event << 10 | first backward event << 12
    uint32_t row;                       // the lowest row of the failed def checks
    uint32_t mask_row[2], need1[2], need0[2];       // [h]: as VerifyAcc's, had start_mask been h at r0
};
static_assert(sizeof(VerifyChunk) == 4 * kVfyChunkFields, "a summary is kVfyChunkFields words");

// what a chunk's walk carries from row to row: the reveal-mask state once per hypothesis (named halves, not an array: every field stays a register)
struct VerifyMaskHalf {
    uint32_t sm, need1, need0, mask_row;            // start_mask under this hypothesis; as VerifyAcc's
};
struct VerifyChunkAcc {
    VerifyAcc d;                        // bits, row, overlap, prev_sid (the def checks write bits and row through verify_def_judge)
    VerifyMaskHalf h0, h1;
    uint32_t fwd, back;
};
HRX_XHD void verify_chunk_begin(VerifyChunkAcc &A) {
    verify_begin(A.d);
    A.h0 = VerifyMaskHalf{0u, kVfyNoRow, kVfyNoRow, kVfyNoRow};
    A.h1 = VerifyMaskHalf{1u, kVfyNoRow, kVfyNoRow, kVfyNoRow};
    A.fwd = A.back = kVfyEvNone;
}
// verify_mask_row's classification of row r (got: the masked cell, e: what it holds where the mask is 1) ...
HRX_XHD void verify_half_row(VerifyMaskHalf &H, uint32_t r, uint32_t got, uint32_t e) {
    if (H.sm && got == 0u) {
        if (e != 0u) H.need0 = vfy_min(H.need0, r);
    } else if (H.sm && got == e) {
        H.need1 = vfy_min(H.need1, r);
    } else if (got != 0u) {
        H.mask_row = vfy_min(H.mask_row, r);
    }
}
// ... and its backward event (set: end_mask = 1 back to the previous event; else reset)
HRX_XHD void verify_half_event(VerifyMaskHalf &H, bool set) {
    H.mask_row = vfy_min(H.mask_row, set ? H.need0 : H.need1);
    H.need0 = H.need1 = kVfyNoRow;
}
// verify_mask_row under both hypotheses
HRX_XHD void verify_chunk_mask_row(VerifyChunkAcc &A, uint32_t r, uint32_t c, uint32_t got, uint32_t s, uint32_t sn) {
    const uint32_t sid = s & 0xffffu, st = (s >> 16) & 0xffu, en = s >> 24;
    const uint32_t sidn = sn & 0xffffu, stn = (sn >> 16) & 0xffu, enn = sn >> 24;
    if (st > 1u || en > 1u) A.d.overlap = 1u;
    if (A.d.prev_sid != sid) {
        if (st) { A.h0.sm = A.h1.sm = 1u; A.fwd = kVfyEvSet; }
        else if (en) { A.h0.sm = A.h1.sm = 0u; A.fwd = kVfyEvReset; }
    }
    A.d.prev_sid = sid;
    const uint32_t e = c | sid << 8;
    verify_half_row(A.h0, r, got, e);
    verify_half_row(A.h1, r, got, e);
    if (sidn != sid && (enn || stn)) {
        verify_half_event(A.h0, enn != 0u);
        verify_half_event(A.h1, enn != 0u);
        if (A.back == kVfyEvNone) A.back = enn ? kVfyEvSet : kVfyEvReset;
    }
}
HRX_XHD VerifyChunk verify_chunk_finish(const VerifyChunkAcc &A) {
    VerifyChunk k;
    k.flags = A.d.bits | (A.d.overlap ? kVfyChunkOverlap : 0u) | A.fwd << kVfyChunkFwdShift | A.back << kVfyChunkBackShift;
    k.row = A.d.row;
    k.mask_row[0] = A.h0.mask_row; k.need1[0] = A.h0.need1; k.need0[0] = A.h0.need0;
    k.mask_row[1] = A.h1.mask_row; k.need1[1] = A.h1.need1; k.need0[1] = A.h1.need0;
    return k;
}

// the next chunk of a string into what the chunks before it left (verify_begin, then every chunk in row order, then verify_finish)
HRX_XHD void verify_fold_chunk(VerifyAcc &a, const VerifyChunk &k) {
    a.bits |= k.flags & 511u;
    a.row = vfy_min(a.row, k.row);
    a.overlap |= (k.flags >> 9) & 1u;
    const uint32_t fwd = (k.flags >> kVfyChunkFwdShift) & 3u, back = (k.flags >> kVfyChunkBackShift) & 3u;
    if (back != kVfyEvNone) {           // the rows pending from the chunks before: judged as verify_mask_row judges them at the event
        a.mask_row = vfy_min(a.mask_row, back == kVfyEvSet ? a.need0 : a.need1);
        a.need0 = a.need1 = kVfyNoRow;
    }
    const uint32_t h = a.start_mask & 1u;
    a.mask_row = vfy_min(a.mask_row, h ? k.mask_row[1] : k.mask_row[0]);
    a.need1 = vfy_min(a.need1, h ? k.need1[1] : k.need1[0]);
    a.need0 = vfy_min(a.need0, h ? k.need0[1] : k.need0[0]);
    if (fwd == kVfyEvSet) a.start_mask = 1u;
    else if (fwd == kVfyEvReset) a.start_mask = 0u;
}

HRX_XHD uint32_t verify_chunk_count(uint32_t M, uint32_t chunk_rows) { return (M + chunk_rows - 1u) / chunk_rows; }
// 0: not a chunk size (chunk_rows a positive multiple of kVfyChunkAlign, M in range)
inline size_t verify_chunked_workspace_bytes(size_t B, size_t M, size_t chunk_rows) {
    if (chunk_rows == 0 || chunk_rows % kVfyChunkAlign || M == 0 || M > kRowsMaxRows || B > 0xffffffffull - 64) return 0;
    return (size_t)kVfyChunkFields * 4u * (M / chunk_rows + (M % chunk_rows != 0)) * B;
}

// rows [r0, r1) of one string of n <= M characters over verify_string's accessor: 0 <= r0 < r1 <= M
template <class Src>
inline VerifyChunk verify_chunk_string(const uint32_t *img, uint32_t D, uint32_t n, uint32_t M, uint32_t r0, uint32_t r1, const Src &src) {
    const VerifyDef *defs = reinterpret_cast<const VerifyDef *>(img);
    VerifyChunkAcc A;
    verify_chunk_begin(A);
    uint32_t s = 0;
    for (uint32_t d = 0; d < D; ++d) {
        s += verify_sums_of(src.rec(r0, d), r0 < n);
        if (r0 > 0) {
            const uint32_t xb = src.rec(r0 - 1u, d);
            s += verify_end_sum(xb);
            A.d.prev_sid += verify_sums_of(xb, r0 - 1u < n) & 0xffffu;
        }
    }
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t c = r < n ? src.chr(r) : 0u;
        uint32_t sn = 0;
        for (uint32_t d = 0; d < D; ++d) {
            const uint32_t x = src.rec(r, d);
            uint32_t next_state = defs[d].dummy;
            if (r + 1u < M) {
                const uint32_t xn = src.rec(r + 1u, d);
                next_state = xn & 0xffffu;
                sn += verify_sums_of(xn, r + 1u < n) + verify_end_sum(x);
            }
            verify_def_row(img, defs[d], r, n, M, c, x, next_state, A.d);
        }
        verify_chunk_mask_row(A, r, c, src.msk(r), s, sn);
        s = sn;
    }
    return verify_chunk_finish(A);
}

// The chunk as the kernel walks it: verify_lane's tile loop over the tiles of [r0, r1) — r0 a multiple of kVfyChunkAlign, r1 one or M — with the row before
// the chunk and the row behind it read alone (src.record).  n <= M.
template <int DT, int T, class Tiles>
HRX_XHD VerifyChunk verify_chunk_lane(const uint32_t *img, const uint32_t Dn, const uint32_t n, const uint32_t M, const uint32_t r0, const uint32_t r1,
                                      const Tiles &src) {
    const uint32_t D = DT ? (uint32_t)DT : Dn;
    const VerifyDef *defs = reinterpret_cast<const VerifyDef *>(img);
    VerifyChunkAcc A;
    verify_chunk_begin(A);
    uint32_t c_prev = 0, mk_prev = 0, s_prev = 0;
    uint32_t x_prev[DT ? DT : 1] = {};
    if (r0 > 0) {                                   // the row before the chunk: its tags are prev_sid, its end flags land on row r0's sums
        uint32_t sb = 0;
        if constexpr (DT > 0) {
HRX_VFY_UNROLL
            for (int d = 0; d < DT; ++d) { x_prev[d] = src.record((uint32_t)d, r0 - 1u); sb += verify_sums_of(x_prev[d], r0 - 1u < n); }
        } else {
            for (uint32_t d = 0; d < D; ++d) sb += verify_sums_of(src.record(d, r0 - 1u), r0 - 1u < n);
        }
        A.d.prev_sid = sb & 0xffffu;
    }
    for (uint32_t base = r0; base < r1; base += T) {
        uint32_t c[T], mk[T], x[DT ? DT : 1][T], sums[T];
        src.chars(base, c);
        src.masked(base, mk);
        if constexpr (DT > 0) {
HRX_VFY_UNROLL
            for (int d = 0; d < DT; ++d) src.records((uint32_t)d, base, x[d]);
        }
HRX_VFY_UNROLL
        for (int j = 0; j < T; ++j) sums[j] = 0;
        auto def_tile = [&](const uint32_t d, const uint32_t(&xd)[T], uint32_t xp) {
            const VerifyDef def = defs[d];
            uint32_t e[T], sw[T], ew[T];
HRX_VFY_UNROLL
            for (int j = 0; j < T; ++j) {
                const bool live = base + j < M && base + j > r0;
                const VerifyLook k = verify_def_look(def, live ? (j ? c[j ? j - 1 : 0] : c_prev) : 0u, live ? (j ? xd[j ? j - 1 : 0] : xp) : def.dummy, live ? xd[j] & 0xffffu : 0u);
                e[j] = img[k.tab]; sw[j] = img[k.start]; ew[j] = img[k.end];
            }
HRX_VFY_UNROLL
            for (int j = 0; j < T; ++j) {
                const uint32_t rj = base + j;          // the row xd[j] holds; row rj - 1 is judged where it is the chunk's
                if (rj < M) {
                    sums[j] += verify_sums_of(xd[j], rj < n);
                    if (rj > 0) sums[j] += verify_end_sum(xp);
                    if (rj > r0) verify_def_judge(def, rj - 1u, n, M, xp, xd[j] & 0xffffu, e[j], sw[j], ew[j], A.d);
                    xp = xd[j];
                }
            }
            return xp;
        };
        if constexpr (DT > 0) {
HRX_VFY_UNROLL
            for (int d = 0; d < DT; ++d) x_prev[d] = def_tile((uint32_t)d, x[d], x_prev[d]);
        } else {
            for (uint32_t d = 0; d < D; ++d) {
                src.records(d, base, x[0]);
                def_tile(d, x[0], base ? src.record(d, base - 1u) : 0u);
            }
        }
HRX_VFY_UNROLL
        for (int j = 0; j < T; ++j) {
            const uint32_t rj = base + j;
            if (rj < M) {
                if (rj > r0) verify_chunk_mask_row(A, rj - 1u, c_prev, mk_prev, s_prev, sums[j]);
                c_prev = c[j]; mk_prev = mk[j]; s_prev = sums[j];
            }
        }
    }
    // row r1 - 1 against row r1, or against the cell nobody assigns
    uint32_t sn = 0;
    auto last_row = [&](const uint32_t d, const uint32_t xp) {
        uint32_t next_state = defs[d].dummy;
        if (r1 < M) {
            const uint32_t xn = src.record(d, r1);
            next_state = xn & 0xffffu;
            sn += verify_sums_of(xn, r1 < n) + verify_end_sum(xp);
        }
        verify_def_row(img, defs[d], r1 - 1u, n, M, c_prev, xp, next_state, A.d);
    };
    if constexpr (DT > 0) {
HRX_VFY_UNROLL
        for (int d = 0; d < DT; ++d) last_row((uint32_t)d, x_prev[d]);
    } else {
        for (uint32_t d = 0; d < D; ++d) last_row(d, src.record(d, r1 - 1u));
    }
    verify_chunk_mask_row(A, r1 - 1u, c_prev, mk_prev, s_prev, sn);
    return verify_chunk_finish(A);
}

// The image of a config out of the rows RegexTableConfig::load assigns: per def transition rows (char, cur, next, substr_id) x n_tr and endpoint rows
// (substr_id, start, end) x n_ep as table_transition_rows / table_endpoint_rows give them, first_state_val and accepted_state_val.  false: rows a dense
// table cannot hold (the first row of either table is not the dummy row, a value out of range, two rows with one (char, cur) key that disagree).
struct VerifyDefRows {
    const uint64_t *tr;
    size_t n_tr;
    const uint64_t *ep;
    size_t n_ep;
    uint64_t first, accepted;
};
inline bool build_verify_image(const VerifyDefRows *rows, size_t D, std::vector<uint32_t> &img) {
    img.assign(D * kVfyDefWords, 0u);
    for (size_t d = 0; d < D; ++d) {
        const VerifyDefRows &R = rows[d];
        if (R.n_tr < 1 || R.n_ep < 1) return false;
        const uint64_t dummy = R.tr[1];
        // table.rs:98-101, 126-144: the first row of each table is the dummy row
        if (R.tr[0] != 0 || R.tr[2] != dummy || R.tr[3] != 0 || R.ep[0] != 0 || R.ep[1] != dummy || R.ep[2] != dummy || dummy > 0xffffu) return false;
        VerifyDef T{};
        T.dummy = (uint32_t)dummy; T.ns = T.dummy + 1u;
        T.first = (uint32_t)(R.first > 0xffffffffull ? 0xffffffffull : R.first);
        T.accepted = (uint32_t)(R.accepted > 0xffffffffull ? 0xffffffffull : R.accepted);
        uint64_t max_sid = 0;
        for (size_t k = 0; k < R.n_ep; ++k) max_sid = R.ep[3 * k] > max_sid ? R.ep[3 * k] : max_sid;
        if (max_sid > 0xffu) return false;
        T.nsid = (uint32_t)max_sid + 1u;
        const size_t bit_words = ((size_t)T.nsid * T.ns + 31u) / 32u;
        T.tab = (uint32_t)img.size();
        T.start = T.tab + T.ns * 256u;
        T.end = T.start + (uint32_t)bit_words;
        img.resize((size_t)T.end + bit_words, 0u);
        for (size_t k = 0; k < (size_t)T.ns * 256u; ++k) img[T.tab + k] = kVfyNoEntry;
        for (size_t k = 0; k < R.n_tr; ++k) {
            const uint64_t ch = R.tr[4 * k], cur = R.tr[4 * k + 1], next = R.tr[4 * k + 2], sid = R.tr[4 * k + 3];
            if (ch > 0xffu || cur > dummy || next > 0xffffu || sid > 0xffu) return false;
            uint32_t &e = img[T.tab + (size_t)cur * 256u + ch];
            const uint32_t v = (uint32_t)next | (uint32_t)sid << 16;
            if (e != kVfyNoEntry && e != v) return false;        // defs.rs:100 keeps (char as u8, cur) in a HashMap: one row per key
            e = v;
        }
        for (size_t k = 0; k < R.n_ep; ++k) {
            const uint64_t sid = R.ep[3 * k], st = R.ep[3 * k + 1], en = R.ep[3 * k + 2];
            if (st > dummy || en > dummy) return false;
            // rows whose end is the dummy serve the start lookup (its third component is the constant dummy), rows whose start is the dummy the end lookup
            if (en == dummy) { const size_t i = (size_t)sid * T.ns + st; img[T.start + i / 32] |= 1u << (i % 32); }
            if (st == dummy) { const size_t i = (size_t)sid * T.ns + en; img[T.end + i / 32] |= 1u << (i % 32); }
        }
        memcpy(&img[d * kVfyDefWords], &T, sizeof T);
    }
    return true;
}

// What a launch of verify_rows_kernel reads (hrx_kernel_verify.hip): the rows, and
struct VerifyArgs : RowsIn {
    const uint32_t *image;                          // build_verify_image, on the device
    uint64_t *verdict;
};
// ... and the two launches of the chunked form: verify_chunk_kernel writes the summaries, verify_stitch_kernel folds them into a.verdict
struct VerifyChunkArgs {
    VerifyArgs a;
    uint32_t chunk_rows, K;                         // K = verify_chunk_count(a.M, chunk_rows)
    uint32_t *summaries;                            // [kVfyChunkFields][K][a.B] u32
};

}  // namespace hrx
