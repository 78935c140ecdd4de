// hrx_product.hpp — the rule of LOOKUP PRODUCT (include/hrx.h: hrx_lookup_invert_table_* / hrx_lookup_product_*) that must exist once: the grand product Z of
// halo2's lookup argument (lookup::prover::commit_product) over the compressed inputs, the compressed table and the index columns of LOOKUP PERMUTE, with
// both denominators taken from inverse TABLES — A'[i] + beta and S'[i] + gamma are table cells, so the inversions are per table row, not per witness row.
// No HIP dependency: the kernels (hrx_kernel_product.hip), the host forms (hrx_product_host.cpp) and tests/host_cpp/test_product_host.cpp include it.
//
// Inverse table, one run of W cells S[w] with `bins` words in use and a shift c (taken mod r first):
//   inv[w] = (S[w] + c)^-1 for w < bins, the zero cell where S[w] + c == 0 (halo2's batch_invert: zeros stay zero); the zero cell for w in [bins, W)
// Product, one lookup c = 3 d + k of one string of n characters, (off, T) = lookup_run_col(run, c), rows i = 0 .. n_rows - 1:
//   A[i]    = the compressed input cell of row i, or the lookup's dummy cell table[off] where product_input_is_dummy (the rows the counts do not count)
//   S[i]    = table[off + product_table_row(i, T)]: the table padded to the circuit's rows with its first row, as LOOKUP PERMUTE pads it
//   term[i] = 0 where a_idx[i] or s_idx[i] lies outside [off, off + T) (product_index_ok; no index is an address before that test),
//             else (A[i] + beta) (S[i] + gamma) inv_beta[a_idx[i]] inv_gamma[s_idx[i]]
//   Z[0] = 1, Z[i + 1] = Z[i] term[i]; entries [0, n_rows] are written; open bit c of the string's word where Z[n_rows] != 1.
// Every result is a fully reduced element of bn256::Fr, so two implementations agree limb for limb whatever their order of operations.
//
// Limb forms.  Montgomery (the default): every cell is x R; fr_mul of two cells is the cell of the product.  Canonical: every cell is the plain x; the scan
// still runs on Montgomery forms — a term is its four plain factors multiplied (x / R^3) times R^5, and a Z is taken out of Montgomery form as it is written
// (fr_from_mont).  The inverse table likewise: S + c is taken into Montgomery form (fr_to_mont), inverted, and taken out.  hrx_fr.h has the rule.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hrx_fr.h"
#include "hrx_lookup_run.hpp"  // HRX_XHD, HRX_MAX_DEFS, PermuteCol, lookup_run_col

namespace hrx {

constexpr uint32_t kPdMaxOpenCols = 32;             // lookups an open word has bits for

// A[i] is the lookup's dummy cell: rows behind the string's own (i >= M), a string without rows (n > M), and — with n == M — row M - 1 of the transition
// and the end lookup (k = 0, 2), whose `next` is the cell match_substrs never assigns and LOOKUP COUNTS leaves out
HRX_XHD bool product_input_is_dummy(uint32_t k, uint32_t i, uint32_t M, uint32_t n) { return i >= M || n > M || (n == M && i + 1u == M && k != 1u); }
HRX_XHD uint32_t product_table_row(uint32_t i, uint32_t T) { return i < T ? i : 0u; }
// an index column's word that may be used as an address into the string's run
HRX_XHD bool product_index_ok(uint32_t w, uint32_t off, uint32_t T) { return w >= off && w - off < T; }

// term[i] as a Montgomery form out of the four cells in the call's limb form: ab = A + beta, sg = S + gamma, ib = inv_beta[ia], ig = inv_gamma[is]
HRX_HD Fr product_term(const Fr &ab, const Fr &sg, const Fr &ib, const Fr &ig, bool canonical) {
    const Fr t = fr_mul(fr_mul(ab, ib), fr_mul(sg, ig));
    return canonical ? fr_mul(t, fr_R5()) : t;      // the plain product over R^3 -> its Montgomery form
}

// ---- how the kernels cut the work (hrx_kernel_product.hip): a workgroup of kPdThreads lanes walks one run (invert) or one (string, lookup) (product) in
// tiles of kPdTileRows cells, kPdRowsPerLane consecutive cells per lane, the running product carried from tile to tile
constexpr uint32_t kPdThreads = 256;
constexpr uint32_t kPdRowsPerLane = 4;
constexpr uint32_t kPdTileRows = kPdThreads * kPdRowsPerLane;
constexpr uint32_t kPdInvertLaunches = 1;           // launches of an invert call: the Fermat step runs once per workgroup, between the two passes

// What an invert call is told
struct InvertArgs {
    const uint64_t *table;                          // [n_runs][W][4]
    const uint64_t *shift;                          // the shift of the first run
    uint32_t shift_stride;                          // u64 words between the runs' shifts: 4, or 0 (one for all)
    uint32_t n_runs, W, bins, canonical;
    uint64_t *inv;                                  // [n_runs][W][4]
};

// What a product call is told
struct ProductArgs {
    const uint32_t *lens;                           // of the batch
    uint32_t M, b_begin, b_count, n_rows, idx_pitch, z_pitch, W, ncols, canonical;
    const uint64_t *in_cells;                       // [ncols][b_count][M][4]
    const uint32_t *a_idx, *s_idx;                  // [ncols][b_count][idx_pitch]
    const uint64_t *table, *inv_beta, *inv_gamma;   // [runs][W][4] each
    uint32_t table_stride;                          // u64 words between the runs of consecutive strings: 0 or 4 W
    const uint64_t *beta, *gamma;
    uint32_t challenge_stride;                      // 4 or 0
    uint64_t *z;                                    // [ncols][b_count][z_pitch][4]
    uint32_t *open;                                 // [b_count], or NULL
    PermuteCol col[3 * HRX_MAX_DEFS];               // lookup_run_col of every lookup
};

}  // namespace hrx
