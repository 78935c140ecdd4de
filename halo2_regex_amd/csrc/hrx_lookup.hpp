// hrx_lookup.hpp — the rule of LOOKUP COUNTS (include/hrx.h: hrx_lookup_counts_device* / hrx_lookup_counts_host) that must exist once: how often the advice rows of a
// string hit each row of the three fixed tables RegexVerifyConfig::configure (src/lib.rs:206-285) looks up per def — the multiplicity column of a logUp-style
// prover, and what halo2's own lookup argument builds its permuted columns from.  No HIP dependency: the kernel (hrx_kernel_lookup.hip), the host form
// (hrx_lookup_host.cpp) and tests/host_cpp/test_lookup_host.cpp all include it.
//
// The tables are the rows RegexTableConfig::load assigns (hrx_verify.hpp's VerifyDefRows: table_transition_rows / table_endpoint_rows), never a walk's table.
// Row r is judged with row r + 1 (Rotation::next), row M - 1 with the cell nobody assigns (the dummy state, no flags), exactly as verify_def_judge does:
//   transition  (en c, en cur + (1 - en) dummy, en next + (1 - en) dummy, en sid)      en = [r < n]                          lib.rs:218-232
//   start       (se sid, se cur + (1 - se) dummy, dummy)                                se = the record's start_enable bit    lib.rs:247-257
//   end         (ee sid, dummy, ee next + (1 - ee) dummy)                               ee = the record's end_enable bit      lib.rs:273-283
// Each tuple adds 1 to the table row equal to it in every component (the lowest such row), or — in no row — 1 to the string's `misses` word.  With n == M the
// transition and end lookups of row M - 1 read a cell match_substrs never assigns: they are neither counted nor missed.  States, ids and flags outside every
// table are misses and index nothing outside the image.
//
// A string's counts are one run of W u32 words, laid out as hrx_lookup_run.hpp states it; the pad words 0.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hrx_lookup_run.hpp"  // the run's layout
#include "hrx_verify.hpp"      // HRX_XHD, RowsIn (hrx_rows.hpp), VerifyDefRows

namespace hrx {

constexpr uint32_t kLkNoRow = 0xffffffffu;          // image: no table row with this key
constexpr uint32_t kLkMiss = 0xffffffffu;           // LookupHit: the tuple is in no table row
constexpr uint32_t kLkNone = 0xfffffffeu;           // LookupHit: the lookup does not exist (row M - 1 of a string of M characters)
constexpr uint32_t kLkTooLong = 0xffffffffu;        // misses of a string with n > M

// One def inside the image (all offsets in u32 words from the image's start).  The image is [D] LookupDef, then every def's arrays:
//   tab    [ns][256] x 2 u32   transition row (char, cur): word 0 its next | substr_id << 16, word 1 its row index; both kLkNoRow where the table has none
//   start  [nsid][ns] u32      the lowest endpoint row (substr_id, state, dummy), or kLkNoRow
//   end    [nsid][ns] u32      the lowest endpoint row (substr_id, dummy, state), or kLkNoRow
struct LookupDef {
    uint32_t tab, start, end;
    uint32_t ns, nsid, dummy;
    uint32_t n_tr, n_ep;                // T_d, E_d
    uint32_t off;                       // where trans[] begins in a string's run; start[] at off + n_tr, end[] at off + n_tr + n_ep
    uint32_t pad[3];
};
constexpr uint32_t kLkDefWords = sizeof(LookupDef) / 4;
static_assert(kLkDefWords % 4 == 0, "the arrays behind the headers start 16-byte aligned");

// where the three lookups of one row land in the string's run of W words
struct LookupHit {
    uint32_t trans, start, end;         // a word index below W, kLkMiss or kLkNone
};

// c = enable[r] * char[r]; x = the def's record of row r; next_state = the state of row r + 1, the def's dummy where r + 1 == M
HRX_XHD LookupHit lookup_def_row(const uint32_t *img, const LookupDef &T, uint32_t r, uint32_t n, uint32_t M, uint32_t c, uint32_t x, uint32_t next_state) {
    const bool en = r < n, unassigned = en && r + 1u == M;
    const uint32_t state = x & 0xffffu, sid = (x >> 16) & 0xffu, se = (x >> 24) & 1u, ee = (x >> 25) & 1u;
    LookupHit h;
    // A disabled row looks (0, dummy, dummy, 0) up and a row without a flag (0, dummy, dummy): the first row of each table (build_lookup_image checks that
    // they are), whatever the record holds — no read of the image
    if (!en) {
        h.trans = T.off;
    } else {
        const bool in = state < T.ns;
        const uint32_t *e = img + T.tab + ((size_t)(in ? state : T.dummy) * 256u + (c & 0xffu)) * 2u;
        const uint32_t v = e[0], row = e[1];
        h.trans = unassigned ? kLkNone : (in && row != kLkNoRow && v == ((next_state & 0xffffu) | sid << 16) ? T.off + row : kLkMiss);
    }
    if (!se) {
        h.start = T.off + T.n_tr;
    } else {
        const bool in = sid < T.nsid && state < T.ns;
        const uint32_t row = img[T.start + (in ? sid * T.ns + state : 0u)];
        h.start = in && row != kLkNoRow ? T.off + T.n_tr + row : kLkMiss;
    }
    if (unassigned) {
        h.end = kLkNone;
    } else if (!ee) {
        h.end = T.off + T.n_tr + T.n_ep;
    } else {
        const uint32_t st = next_state & 0xffffu;
        const bool in = sid < T.nsid && st < T.ns;
        const uint32_t row = img[T.end + (in ? sid * T.ns + st : 0u)];
        h.end = in && row != kLkNoRow ? T.off + T.n_tr + T.n_ep + row : kLkMiss;
    }
    return h;
}

// words of one string's run, read back from the image: where the last def's bins end, rounded as hrx_lookup_run.hpp rounds
HRX_XHD uint32_t lookup_words(const uint32_t *img, uint32_t D) {
    const LookupDef &T = reinterpret_cast<const LookupDef *>(img)[D - 1];
    return (uint32_t)lookup_run_words(T.off + lookup_run_def_words(T.n_tr, T.n_ep));
}

// One string of n characters over verify_string's accessor — src.chr(r) (r < n only), src.rec(r, d) — into counts[W] and its misses word: the definition.
template <class Src>
inline uint32_t lookup_string(const uint32_t *img, uint32_t D, uint32_t n, uint32_t M, const Src &src, uint32_t *counts) {
    const LookupDef *defs = reinterpret_cast<const LookupDef *>(img);
    const uint32_t W = lookup_words(img, D);
    memset(counts, 0, (size_t)W * 4u);
    if (n > M) return kLkTooLong;
    uint32_t misses = 0;
    for (uint32_t r = 0; r < M; ++r) {
        const uint32_t c = r < n ? src.chr(r) : 0u;
        for (uint32_t d = 0; d < D; ++d) {
            const uint32_t next_state = r + 1u < M ? src.rec(r + 1u, d) & 0xffffu : defs[d].dummy;
            const LookupHit h = lookup_def_row(img, defs[d], r, n, M, c, src.rec(r, d), next_state);
            const uint32_t w[3] = {h.trans, h.start, h.end};
            for (uint32_t k = 0; k < 3; ++k) {
                if (w[k] == kLkMiss) ++misses;
                else if (w[k] != kLkNone) ++counts[w[k]];
            }
        }
    }
    return misses;
}

// The image of a config out of the rows RegexTableConfig::load assigns (build_verify_image's inputs).  false: rows the image cannot hold — whatever
// build_verify_image refuses (the first row of either table is not the dummy row, a value out of range, two rows with one (char, cur) key that disagree),
// or a run lookup_run_fill refuses.  Two transition rows with one key that agree: the lower row takes the counts, as with endpoint rows.
inline bool build_lookup_image(const VerifyDefRows *rows, size_t D, std::vector<uint32_t> &img) {
    if (D == 0) return false;
    LookupRun run;
    if (!lookup_run_fill(run, D, [rows](size_t d, size_t &t, size_t &e) { t = rows[d].n_tr; e = rows[d].n_ep; })) return false;
    img.assign(D * kLkDefWords, 0u);
    for (size_t d = 0; d < D; ++d) {
        const VerifyDefRows &R = rows[d];
        if (R.n_tr < 1 || R.n_ep < 1) return false;
        const uint64_t dummy = R.tr[1];
        if (R.tr[0] != 0 || R.tr[2] != dummy || R.tr[3] != 0 || R.ep[0] != 0 || R.ep[1] != dummy || R.ep[2] != dummy || dummy > 0xffffu) return false;
        LookupDef T{};
        T.dummy = (uint32_t)dummy; T.ns = T.dummy + 1u;
        uint64_t max_sid = 0;
        for (size_t k = 0; k < R.n_ep; ++k) max_sid = R.ep[3 * k] > max_sid ? R.ep[3 * k] : max_sid;
        if (max_sid > 0xffu) return false;
        T.nsid = (uint32_t)max_sid + 1u;
        T.n_tr = run.def[d].n_tr; T.n_ep = run.def[d].n_ep; T.off = run.def[d].off;
        const size_t keys = (size_t)T.nsid * T.ns;
        T.tab = (uint32_t)img.size();
        T.start = T.tab + T.ns * 512u;
        T.end = T.start + (uint32_t)keys;
        img.resize(((size_t)T.end + keys + 3u) & ~(size_t)3u, 0u);
        for (size_t k = T.tab; k < (size_t)T.end + keys; ++k) img[k] = kLkNoRow;
        for (size_t k = 0; k < R.n_tr; ++k) {
            const uint64_t ch = R.tr[4 * k], cur = R.tr[4 * k + 1], next = R.tr[4 * k + 2], sid = R.tr[4 * k + 3];
            if (ch > 0xffu || cur > dummy || next > 0xffffu || sid > 0xffu) return false;
            uint32_t *e = &img[T.tab + ((size_t)cur * 256u + ch) * 2u];
            const uint32_t v = (uint32_t)next | (uint32_t)sid << 16;
            if (e[1] != kLkNoRow && e[0] != v) return false;        // defs.rs:100 keeps (char as u8, cur) in a HashMap: one row per key
            if (e[1] == kLkNoRow) { e[0] = v; e[1] = (uint32_t)k; }
        }
        for (size_t k = 0; k < R.n_ep; ++k) {
            const uint64_t sid = R.ep[3 * k], st = R.ep[3 * k + 1], en = R.ep[3 * k + 2];
            if (st > dummy || en > dummy) return false;
            // rows whose end is the dummy serve the start lookup (its third component is the constant dummy), rows whose start is the dummy the end lookup
            if (en == dummy) { uint32_t &e = img[T.start + (size_t)sid * T.ns + st]; if (e == kLkNoRow) e = (uint32_t)k; }
            if (st == dummy) { uint32_t &e = img[T.end + (size_t)sid * T.ns + en]; if (e == kLkNoRow) e = (uint32_t)k; }
        }
        memcpy(&img[d * kLkDefWords], &T, sizeof T);
    }
    return true;
}

// ---- how the kernel cuts the work (hrx_kernel_lookup.hip): a workgroup owns G consecutive strings of the window and keeps their bins in LDS, G x pass_words
// u32.  One pass where a string's run fits (pass_words = W); otherwise G = 1 and `passes` ranges of the run, each a walk over the rows again.
constexpr uint32_t kLkThreads = 512;                // lanes of a workgroup (measured against 256 and 1024: DESIGN.md §18)
constexpr uint32_t kLkMaxGroup = 64;                // strings of a workgroup at most
constexpr size_t kLkLdsShared = 64u * 1024u;        // G > 1: what a workgroup may take, so that two fit a CU
constexpr size_t kLkLdsAll = 160u * 1024u;          // G = 1: a single workgroup may declare the whole LDS of a CU
struct LookupPlan {
    uint32_t G, pass_words, passes;
    size_t lds_bytes;                               // the bins, then G misses words (at least 16 bytes)
};
HRX_XHD size_t lookup_lds_bytes(uint32_t G, uint32_t pass_words) { return (size_t)G * pass_words * 4u + (G * 4u < 16u ? 16u : G * 4u); }
// W: lookup_words; b_count: strings of the window; num_cus: of the device.  G: the largest power of two whose bins fit kLkLdsShared, halved while fewer than
// two workgroups per CU would come of it.
inline LookupPlan plan_lookup(size_t W, size_t b_count, int num_cus) {
    LookupPlan p{1u, (uint32_t)W, 1u, 0};
    if (lookup_lds_bytes(1, (uint32_t)W) > kLkLdsAll) {
        const size_t cap = (kLkLdsAll - 16u) / 4u & ~(size_t)3u;
        p.passes = (uint32_t)((W + cap - 1) / cap);
        p.pass_words = (uint32_t)(((W + p.passes - 1) / p.passes + 3u) & ~(size_t)3u);
    } else {
        while (p.G < kLkMaxGroup && lookup_lds_bytes(2u * p.G, (uint32_t)W) <= kLkLdsShared) p.G *= 2u;
        const size_t want = 2u * (size_t)(num_cus > 0 ? num_cus : 256);
        while (p.G > 1u && (b_count + p.G - 1) / p.G < want) p.G /= 2u;
    }
    p.lds_bytes = lookup_lds_bytes(p.G, p.pass_words);
    return p;
}

// What a launch of lookup_counts_kernel reads: the rows (no masked rows: masked == NULL), and
struct LookupArgs : RowsIn {
    uint32_t b_begin, b_count;                      // the window
    const uint32_t *image;                          // build_lookup_image (on the device for the kernel)
    uint32_t W;                                     // lookup_words(image, D)
    uint32_t G, pass_words, passes;                 // plan_lookup (the kernel only)
    uint32_t *counts;                               // [b_count][W]
    uint32_t *misses;                               // [b_count], or NULL
};

}  // namespace hrx
