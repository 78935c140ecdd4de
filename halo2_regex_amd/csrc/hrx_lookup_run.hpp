// hrx_lookup_run.hpp — the RUN of one string in the lookup argument, once: the index space LOOKUP COUNTS counts into, LOOKUP COMPRESS folds the tables into
// and LOOKUP PERMUTE reads both through.  Per def in order trans[T_d], start[E_d], end[E_d] — T_d, E_d the rows table_transition_rows / table_endpoint_rows
// give for the def — and W, the total rounded up to a multiple of 4 (the pad words hold 0 counts and zero cells).  No HIP dependency: the image builders
// (hrx_lookup.hpp, hrx_compress.hpp), the entry points (defs_lookup_run of hrx_rows_api.cpp) and the stand-alone host tests all read the layout here.
// DESIGN.md §19.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hrx.h" // HRX_MAX_DEFS
#include "hrx_rows.hpp"        // HRX_XHD

namespace hrx {

// the words of one def's bins, and of a run whose defs have `bins` words together
HRX_XHD uint64_t lookup_run_def_words(uint64_t n_tr, uint64_t n_ep) { return n_tr + 2u * n_ep; }
HRX_XHD uint64_t lookup_run_words(uint64_t bins) { return (bins + 3u) & ~(uint64_t)3u; }

struct LookupRun {
    uint32_t D, W, T_max;                           // defs; words of a run; the rows of the longest table of any def
    struct Def { uint32_t off, n_tr, n_ep; } def[HRX_MAX_DEFS];      // trans[] at off, start[] at off + n_tr, end[] at off + n_tr + n_ep
};

// rows_of(d, n_tr, n_ep) gives def d's T_d and E_d (size_t &).  false: no such layout — more defs than HRX_MAX_DEFS, or more bins than a u32 run indexes
template <class RowsOf>
inline bool lookup_run_fill(LookupRun &run, size_t D, const RowsOf &rows_of) {
    run = LookupRun{};
    if (D > HRX_MAX_DEFS) return false;
    uint64_t w = 0;
    for (size_t d = 0; d < D; ++d) {
        size_t t = 0, e = 0;
        rows_of(d, t, e);
        if (w + lookup_run_def_words(t, e) > 0x7fffffffull) return false;
        run.def[d] = {(uint32_t)w, (uint32_t)t, (uint32_t)e};
        run.T_max = run.T_max > t ? run.T_max : (uint32_t)t;
        run.T_max = run.T_max > e ? run.T_max : (uint32_t)e;
        w += lookup_run_def_words(t, e);
    }
    run.D = (uint32_t)D; run.W = (uint32_t)lookup_run_words(w);
    return true;
}

// lookup c = 3 d + k (hrx_lookup_num_columns' order: k = 0 trans, 1 start, 2 end of def d): where its counts begin in a run, and its table's rows
struct PermuteCol { uint32_t off, T; };
HRX_XHD PermuteCol lookup_run_col(const LookupRun &run, uint32_t c) {
    const LookupRun::Def &R = run.def[c / 3u];
    const uint32_t k = c % 3u;
    return k == 0u ? PermuteCol{R.off, R.n_tr} : k == 1u ? PermuteCol{R.off + R.n_tr, R.n_ep} : PermuteCol{R.off + R.n_tr + R.n_ep, R.n_ep};
}

}  // namespace hrx
