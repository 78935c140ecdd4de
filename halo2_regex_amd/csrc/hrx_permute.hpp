// hrx_permute.hpp — the rule of LOOKUP PERMUTE (include/hrx.h: hrx_lookup_permute_device / hrx_lookup_permute_host) that must exist once: the permuted columns
// A', S' of halo2's lookup argument (lookup::prover::commit_permuted) out of one lookup's counts, as indices into the string's run and as table cells — no
// sort.  No HIP dependency: the kernel (hrx_kernel_permute.hip), the host form (hrx_permute_host.cpp) and tests/host_cpp/test_permute_host.cpp include it.
//
// One lookup: a table of T rows, its counts m[0 .. T) in the string's run, a circuit of n_rows usable rows.
//   1  sum = the sum of m[t], in 64 bits (the counts are caller memory: two words of 0xffffffff must not wrap)
//   2  sum > n_rows: the lookup overflows — every index kPmOverflow, every cell limb 0, its bit in the string's overflow word
//   3  m'[0] = m[0] + (n_rows - sum), m'[t] = m[t] elsewhere: the rows no string row covers look the tables' first row, the dummy tuple, up
//   4  A_idx is non-decreasing and holds row t m'[t] times
//   5  position i is a FIRST position where i == 0 or A_idx[i] != A_idx[i - 1];  6  there S_idx[i] = A_idx[i]
//   7  the j-th position that is no first position takes the j-th element of the fill list: the rows with m'[t] == 0 ascending, then row 0 n_rows - T times
// — index for index what permuted_lookup_columns of the Python package builds with numpy, which stays the yardstick.
//
// Every position stands alone: with the non-empty runs numbered k = 0 .. K - 1 in row order, run k of row nz[k] beginning at position e[k] (e[0] = 0), and
// zrow[0 .. Z) the empty rows ascending (K + Z = T), position i of run k has A_idx = nz[k]; S_idx = nz[k] where i == e[k]; otherwise j = i - (k + 1) — of the
// i + 1 positions up to i, k + 1 are first positions — and S_idx = zrow[j] where j < Z, else 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "hrx_lookup_run.hpp"  // HRX_XHD, HRX_MAX_DEFS, PermuteCol: a lookup's place in a string's run

namespace hrx {

constexpr uint32_t kPmOverflow = 0xffffffffu;       // every index of a lookup whose counts exceed the circuit's rows
constexpr uint32_t kPmMaxRows = 1u << 24;           // n_rows at most (the prefix sums of a lookup that does not overflow stay in 32 bits with room)
constexpr uint32_t kPmMaxOverflowCols = 32;         // lookups an overflow word has bits for

// rule 3: the count of row t once the rows outside the string are added to row 0 (pad = n_rows - sum)
HRX_XHD uint32_t permute_count(uint32_t t, uint32_t m, uint32_t pad) { return t == 0u ? m + pad : m; }

// rules 5 - 7 for position i of the k-th non-empty run, which begins at position e: kPmFirst — a first position — or j, the position's place in the fill list
constexpr uint32_t kPmFirst = 0xffffffffu;
HRX_XHD uint32_t permute_fill_place(uint32_t i, uint32_t e, uint32_t k) { return i == e ? kPmFirst : i - (k + 1u); }

// the fill list's element j where the list of empty rows has Z entries and row_j = zrow[j] (read by the caller only where j < Z)
HRX_XHD uint32_t permute_fill_row(uint32_t j, uint32_t Z, uint32_t row_j) { return j < Z ? row_j : 0u; }

// ---- how the kernel cuts the work (hrx_kernel_permute.hip).  A workgroup serves one (string, lookup) and one range of `group_rows` positions of it.  It
// walks the table in chunks of kPmChunkRows rows, keeps the chunk's non-empty runs (nz, e) and — where the table is one chunk — the empty rows in LDS, and
// expands the positions of the chunk's runs in tiles of kPmTileRows positions on absolute tile borders.  A table of more than one chunk keeps its empty rows
// in the caller's workspace (one u32 per word of the run) and is served by one workgroup per (string, lookup).
constexpr uint32_t kPmThreads = 256;                // lanes of a workgroup
constexpr uint32_t kPmTileRows = 4u * kPmThreads;   // positions of one expansion step: four per lane, one 16-byte store of each index column
constexpr uint32_t kPmChunkRows = 3072;             // table rows of one chunk: 8 bytes of LDS per row
struct PermutePlan {
    uint32_t tile_rows, chunk_rows;
    uint32_t group_rows;                            // positions per workgroup: a multiple of tile_rows
    uint32_t groups;                                // workgroups per (string, lookup)
    size_t workspace_bytes;                         // 0: every table is one chunk
};
// T_max: the longest table of the defs; W: words of a string's run; lookups: 3 D.  One workgroup per (string, lookup) where that gives every CU four of them
// (the scans are then done once); otherwise the positions are cut into as many ranges as reach that, none below one tile.
inline PermutePlan plan_permute(size_t T_max, size_t W, size_t lookups, size_t b_count, size_t n_rows, int num_cus) {
    PermutePlan p{kPmTileRows, kPmChunkRows, 0u, 1u, 0};
    const size_t tiles = (n_rows + kPmTileRows - 1) / kPmTileRows;
    if (T_max > kPmChunkRows) {
        p.workspace_bytes = b_count * W * 4u;
    } else {
        const size_t want = 4u * (size_t)(num_cus > 0 ? num_cus : 256), have = b_count * lookups;
        if (have && have < want) p.groups = (uint32_t)std::min<size_t>(tiles ? tiles : 1, (want + have - 1) / have);
    }
    const size_t per = tiles ? (tiles + p.groups - 1) / p.groups : 1;
    p.group_rows = (uint32_t)(per * kPmTileRows);
    p.groups = (uint32_t)(tiles ? (tiles + per - 1) / per : 1);
    return p;
}

// What a launch of the permute kernels, or the host form, reads
struct PermuteArgs {
    const uint32_t *counts;                         // [b_count][W]
    uint32_t b_count, n_rows, pitch, W, ncols;
    uint32_t *a_idx, *s_idx;                        // [ncols][b_count][pitch], or both NULL
    const uint64_t *table;                          // [runs][W][4], or NULL
    uint32_t table_stride;                          // u64 words between the runs of consecutive strings: 0 or 4 W
    uint64_t *a_cells, *s_cells;                    // [ncols][b_count][pitch][4], or both NULL
    uint32_t *overflow;                             // [b_count], or NULL
    uint32_t *zrows;                                // the workspace: [b_count][W] (the kernel only, where a table has more than one chunk)
    uint32_t groups, group_rows;                    // plan_permute (the kernel only)
    PermuteCol col[3 * HRX_MAX_DEFS];               // lookup_run_col (hrx_lookup_run.hpp) of every lookup
};

}  // namespace hrx
