// hrx_compress.hpp — the rule of LOOKUP COMPRESS (include/hrx.h: hrx_lookup_compress_inputs_* / hrx_lookup_compress_table_*) that must exist once: the three
// lookup tuples of a witness row and the rows of the fixed tables, each folded with a challenge theta into one field cell — what a lookup argument works
// on (halo2's commit_permuted: acc = acc * theta + e_i from 0 over the input expressions of meta.lookup, the table columns folded the same way).  No HIP
// dependency: the kernels (hrx_kernel_compress.hip), the host forms (hrx_compress_host.cpp) and tests/host_cpp/test_compress_host.cpp all include it.
//
// The tuples are the ones lookup_def_row of hrx_lookup.hpp judges, as integers.  Row r with row r + 1 (Rotation::next), the def's dummy state behind row M - 1:
//   trans  (en c, en cur + (1 - en) dummy, en next + (1 - en) dummy, en sid)      en = [r < n]                          lib.rs:218-232
//   start  (se sid, se cur + (1 - se) dummy, dummy)                                se = the record's start_enable bit    lib.rs:247-257
//   end    (ee sid, dummy, ee next + (1 - ee) dummy)                               ee = the record's end_enable bit      lib.rs:273-283
// Nothing is left out: with n == M the trans and end cells of row M - 1 are computed from that `next` (the dummy) like any other — the cell match_substrs
// never assigns, which LOOKUP COUNTS neither counts nor misses.  Values are folded as they lie: a state, id or flag outside every table is folded as the
// integer the record holds (what the expression evaluates to), so a tampered row's cell is in no table row.  n > M: the string has no rows, every limb of
// every one of its cells is 0.
//
// Cells: [3 D][strings][M][4] u64, column 3 d + k: k = 0 trans, 1 start, 2 end of def d.  Table cells: per theta one run of W cells in the index space of
// the counts (the run of hrx_lookup_run.hpp) — the two endpoint runs of a def hold equal cells — and zero cells for the pad words.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "hrx_fr.h"
#include "hrx_lookup_run.hpp"  // the run's layout
#include "hrx_verify.hpp"     // HRX_XHD, RowsIn (hrx_rows.hpp), VerifyDefRows

namespace hrx {

// the three tuples of one row of one def as (a0, a1, a2, a3), folded a0 theta^3 + a1 theta^2 + a2 theta + a3; a tuple of three components has a0 = 0
struct CompressTuples {
    uint32_t trans[4], start[4], end[4];
};

// c = the input byte of row r (read for r < n only); x = the def's record of row r; next_state = the state of row r + 1, the def's dummy where r + 1 == M.
// Every component is below 2^16.  No value of a record is used as an index here or anywhere behind: out-of-range values are folded, never looked up.
HRX_XHD CompressTuples compress_def_row(uint32_t dummy, uint32_t r, uint32_t n, uint32_t c, uint32_t x, uint32_t next_state) {
    const uint32_t en = r < n ? 1u : 0u;
    const uint32_t state = x & 0xffffu, sid = (x >> 16) & 0xffu, se = (x >> 24) & 1u, ee = (x >> 25) & 1u, next = next_state & 0xffffu;
    CompressTuples t;
    t.trans[0] = en ? c & 0xffu : 0u; t.trans[1] = en ? state : dummy; t.trans[2] = en ? next : dummy; t.trans[3] = en ? sid : 0u;
    t.start[0] = 0u; t.start[1] = se ? sid : 0u; t.start[2] = se ? state : dummy; t.start[3] = dummy;
    t.end[0] = 0u; t.end[1] = ee ? sid : 0u; t.end[2] = dummy; t.end[3] = ee ? next : dummy;
    return t;
}

// What a compress call over rows is told: the rows, and
struct CompressArgs : RowsIn {
    uint32_t b_begin, b_count;                      // the strings of this launch
    const uint64_t *theta;                          // the challenge of the launch's first string
    uint32_t theta_stride;                          // u64 words between the strings' challenges: 4, or 0 (one for all)
    uint32_t canonical;                             // theta and the cells are plain integers (HRX_FR_CANONICAL)
    uint64_t *cells;                                // column 0 of the launch's first string
    uint64_t col_cells;                             // cells per column: strings of the whole call x M
    uint32_t tiles;                                 // the kernel only: row tiles per workgroup
    uint16_t dummy[HRX_MAX_DEFS];                   // per def its dummy state
};

// One string (the i-th of the launch) of n characters over RowsOf's accessor — src.chr(r) (r < n only), src.rec(r, d) — into its M cells of every column:
// the definition.
template <class Src>
inline void compress_string(const CompressArgs &a, size_t i, uint32_t n, const Src &src, const FrPowers &p) {
    const uint32_t M = a.M;
    for (uint32_t d = 0; d < a.D; ++d) {
        uint64_t *col[3];
        for (uint32_t k = 0; k < 3; ++k) col[k] = a.cells + ((size_t)(3u * d + k) * a.col_cells + i * M) * 4u;
        for (uint32_t r = 0; r < M; ++r) {
            if (n > M) {
                for (uint32_t k = 0; k < 3; ++k) fr_store_cell(col[k] + 4 * (size_t)r, Fr{});
                continue;
            }
            const uint32_t dummy = a.dummy[d];
            const uint32_t next_state = r + 1u < M ? src.rec(r + 1u, d) & 0xffffu : dummy;
            const CompressTuples t = compress_def_row(dummy, r, n, r < n ? src.chr(r) : 0u, src.rec(r, d), next_state);
            const uint32_t *tup[3] = {t.trans, t.start, t.end};
            for (uint32_t k = 0; k < 3; ++k) fr_store_cell(col[k] + 4 * (size_t)r, fr_fold(tup[k][0], tup[k][1], tup[k][2], tup[k][3], p));
        }
    }
}

// The rows of the fixed tables in the index space of the counts, as a flat (a0, a1, a2, a3) u32 array: 4 W words, W the run's of hrx_lookup_run.hpp.
// trans[T_d]: (char, cur, next, sid) of transition row t; start[E_d] and end[E_d]: (0, sid, start_state, end_state) of endpoint row e, both runs; the pad
// words (0, 0, 0, 0), whose fold is the zero cell.  false: a value that is no 16-bit tuple component, no rows, a run lookup_run_fill refuses, or an image
// that did not come out at the run's 4 W words.
inline bool build_compress_image(const VerifyDefRows *rows, size_t D, std::vector<uint32_t> &img) {
    if (D == 0) return false;
    LookupRun run;
    if (!lookup_run_fill(run, D, [rows](size_t d, size_t &t, size_t &e) { t = rows[d].n_tr; e = rows[d].n_ep; })) return false;
    img.clear();
    for (size_t d = 0; d < D; ++d) {      // appended in the run's order: trans, start, end of each def
        const VerifyDefRows &R = rows[d];
        if (R.n_tr < 1 || R.n_ep < 1) return false;
        for (size_t k = 0; k < 4 * R.n_tr; ++k) {
            if (R.tr[k] > 0xffffu) return false;
            img.push_back((uint32_t)R.tr[k]);
        }
        for (int run = 0; run < 2; ++run)
            for (size_t k = 0; k < R.n_ep; ++k) {
                img.push_back(0u);
                for (size_t j = 0; j < 3; ++j) {
                    if (R.ep[3 * k + j] > 0xffffu) return false;
                    img.push_back((uint32_t)R.ep[3 * k + j]);
                }
            }
    }
    img.resize(4 * (size_t)lookup_run_words(img.size() / 4), 0u);
    return img.size() == 4 * (size_t)run.W;
}

// What a compress call over the table is told
struct CompressTableArgs {
    const uint32_t *image;                          // build_compress_image (on the device for the kernel)
    uint32_t W;                                     // its tuples
    const uint64_t *theta;
    uint32_t theta_stride, n_theta, canonical;
    uint64_t *cells;                                // [n_theta][W][4]
};

// ---- how the kernels cut the work (hrx_kernel_compress.hip)
constexpr uint32_t kCzThreads = 256;                // lanes of a workgroup
constexpr uint32_t kCzRowsPerStore = 32;            // rows one store instruction of a wave writes: two lanes per 32-byte cell
constexpr uint32_t kCzStores = 4;                   // store instructions of one column before the next column's turn
constexpr uint32_t kCzRowsPerTile = (kCzThreads / 64u) * kCzRowsPerStore * kCzStores;     // rows of a workgroup's tile: 512
constexpr uint32_t kCzMaxTiles = 8;                 // tiles of one string a workgroup serves at most: the powers of theta are computed once per workgroup
constexpr uint32_t kCzTableRowsPerGroup = 4u * kCzThreads;                               // table rows of a workgroup: one lane per row, four rows in turn

}  // namespace hrx
