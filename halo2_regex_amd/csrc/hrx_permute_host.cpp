// hrx_permute_host.cpp — the host form of LOOKUP PERMUTE (include/hrx.h hrx_lookup_permute_host): the rule of hrx_permute.hpp over counts, table cells and
// outputs in host memory, over threads by ranges of strings.  No HIP; the host twin of hrx_kernel_permute.hip and the definition of the columns.
// tests/host_cpp/test_permute_host.cpp includes this file as it is.
#include <string.h>

#include <vector>

#include "hrx_over_threads.hpp"
#include "hrx_permute.hpp"

namespace hrx {

// lookup c of string b of the window: true where it overflows.  nz, e, zrow: the thread's lists, at least T entries each
static bool permute_lookup_host(const PermuteArgs &a, size_t b, uint32_t c, uint32_t *nz, uint32_t *e, uint32_t *zrow) {
    const PermuteCol L = a.col[c];
    const uint32_t *m = a.counts + b * a.W + L.off;
    const size_t o = ((size_t)c * a.b_count + b) * a.pitch;
    const uint64_t *run = a.table ? a.table + b * a.table_stride : nullptr;
    uint64_t sum = 0;                                   // rule 1
    for (uint32_t t = 0; t < L.T; ++t) sum += m[t];
    if (sum > a.n_rows) {                               // rule 2: no count is looked at again
        if (a.a_idx) {
            for (uint32_t i = 0; i < a.n_rows; ++i) a.a_idx[o + i] = a.s_idx[o + i] = kPmOverflow;
        }
        if (a.a_cells) {
            memset(a.a_cells + o * 4u, 0, (size_t)a.n_rows * 32u);
            memset(a.s_cells + o * 4u, 0, (size_t)a.n_rows * 32u);
        }
        return true;
    }
    const uint32_t pad = a.n_rows - (uint32_t)sum;
    uint32_t K = 0, Z = 0, pos = 0;
    for (uint32_t t = 0; t < L.T; ++t) {
        const uint32_t mt = permute_count(t, m[t], pad);
        if (mt) { nz[K] = t; e[K] = pos; ++K; pos += mt; }
        else zrow[Z++] = t;
    }
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t end = k + 1u < K ? e[k + 1u] : a.n_rows;
        for (uint32_t i = e[k]; i < end; ++i) {
            const uint32_t j = permute_fill_place(i, e[k], k);
            const uint32_t s = j == kPmFirst ? nz[k] : permute_fill_row(j, Z, j < Z ? zrow[j] : 0u);
            const uint32_t aw = L.off + nz[k], sw = L.off + s;
            if (a.a_idx) { a.a_idx[o + i] = aw; a.s_idx[o + i] = sw; }
            if (a.a_cells) {
                memcpy(a.a_cells + (o + i) * 4u, run + (size_t)aw * 4u, 32);
                memcpy(a.s_cells + (o + i) * 4u, run + (size_t)sw * 4u, 32);
            }
        }
    }
    return false;
}

// arguments checked by the caller.  threads: 0 = as many as the machine has, at most 16; never more than one per string
void permute_host(const PermuteArgs &a, unsigned threads) {
    if (a.b_count == 0) return;
    uint32_t T_max = 0;
    for (uint32_t c = 0; c < a.ncols; ++c) T_max = std::max(T_max, a.col[c].T);
    over_threads(a.b_count, rows_host_threads(threads), [&a, T_max](size_t b0, size_t b1) {
        std::vector<uint32_t> lists(3u * (size_t)T_max);
        uint32_t *nz = lists.data(), *e = nz + T_max, *zrow = e + T_max;
        for (size_t b = b0; b < b1; ++b) {
            uint32_t over = 0;
            for (uint32_t c = 0; c < a.ncols; ++c)
                if (permute_lookup_host(a, b, c, nz, e, zrow) && c < kPmMaxOverflowCols) over |= 1u << c;
            if (a.overflow) a.overflow[b] = over;
        }
    });
}

}  // namespace hrx
