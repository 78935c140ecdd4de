// hrx_product_host.cpp — the host forms of LOOKUP PRODUCT (include/hrx.h hrx_lookup_invert_table_host / hrx_lookup_product_host): the rule of
// hrx_product.hpp over cells, indices and outputs in host memory — the inverse tables over threads by ranges of runs (batch inversion per run: prefix
// products, one fr_inv, the walk back), the product over threads by ranges of strings, row after row.  No HIP; the host twins of hrx_kernel_product.hip and
// the definition of the cells.  tests/host_cpp/test_product_host.cpp includes this file as it is.
#include <vector>

#include "hrx_over_threads.hpp"
#include "hrx_product.hpp"

namespace hrx {

// arguments checked by the caller.  threads: 0 = as many as the machine has, at most 16; never more than one per run
void invert_table_host(const InvertArgs &a, unsigned threads) {
    if (a.n_runs == 0 || a.W == 0) return;
    over_threads(a.n_runs, rows_host_threads(threads), [&a](size_t r0, size_t r1) {
        const bool canonical = a.canonical != 0;
        std::vector<Fr> el(a.bins);                              // the run's elements: S + c in Montgomery form, one where that is zero
        std::vector<uint8_t> zero(a.bins);
        for (size_t run = r0; run < r1; ++run) {
            const uint64_t *S = a.table + run * a.W * 4u;
            uint64_t *out = a.inv + run * a.W * 4u;
            const Fr c = fr_challenge(a.shift + run * a.shift_stride);
            Fr acc = fr_R();
            for (uint32_t w = 0; w < a.bins; ++w) {              // out[w] = the product of the elements before w
                const Fr sc = fr_add(fr_load_cell(S + (size_t)w * 4u), c);
                zero[w] = fr_is_zero(sc);
                el[w] = zero[w] ? fr_R() : fr_to_mont(sc, canonical);
                fr_store_cell(out + (size_t)w * 4u, acc);
                acc = fr_mul(acc, el[w]);
            }
            Fr back = fr_inv(acc);                               // 1 / (the elements up to w)
            for (uint32_t w = a.bins; w-- > 0u;) {
                const Fr inv = fr_mul(back, fr_load_cell(out + (size_t)w * 4u));
                fr_store_cell(out + (size_t)w * 4u, zero[w] ? Fr{} : fr_from_mont(inv, canonical));
                back = fr_mul(back, el[w]);
            }
            for (uint32_t w = a.bins; w < a.W; ++w) fr_store_cell(out + (size_t)w * 4u, Fr{});
        }
    });
}

// lookup c of string bi of the window: true where Z[n_rows] is not one
static bool product_lookup_host(const ProductArgs &a, size_t bi, uint32_t c) {
    const PermuteCol L = a.col[c];
    const uint32_t k3 = c % 3u, M = a.M, n = a.lens[a.b_begin + bi];
    const bool canonical = a.canonical != 0;
    const uint64_t *run = a.table + bi * a.table_stride, *ib_run = a.inv_beta + bi * a.table_stride, *ig_run = a.inv_gamma + bi * a.table_stride;
    const size_t pair = (size_t)c * a.b_count + bi;
    const uint64_t *in = a.in_cells + pair * M * 4u;
    const uint32_t *a_idx = a.a_idx + pair * a.idx_pitch, *s_idx = a.s_idx + pair * a.idx_pitch;
    uint64_t *z = a.z + pair * a.z_pitch * 4u;
    const Fr beta = fr_challenge(a.beta + bi * a.challenge_stride), gamma = fr_challenge(a.gamma + bi * a.challenge_stride);
    const Fr s0 = fr_load_cell(run + (size_t)L.off * 4u), one = fr_unit(canonical);
    Fr acc = fr_R();
    fr_store_cell(z, one);
    for (uint32_t i = 0; i < a.n_rows; ++i) {
        const uint32_t ia = a_idx[i], is = s_idx[i];
        Fr t = {};
        if (product_index_ok(ia, L.off, L.T) && product_index_ok(is, L.off, L.T)) {     // no index is an address before the test
            const Fr A = product_input_is_dummy(k3, i, M, n) ? s0 : fr_load_cell(in + (size_t)i * 4u);
            const Fr S = fr_load_cell(run + (size_t)(L.off + product_table_row(i, L.T)) * 4u);
            t = product_term(fr_add(A, beta), fr_add(S, gamma), fr_load_cell(ib_run + (size_t)ia * 4u), fr_load_cell(ig_run + (size_t)is * 4u), canonical);
        }
        acc = fr_mul(acc, t);
        fr_store_cell(z + (size_t)(i + 1u) * 4u, fr_from_mont(acc, canonical));
    }
    return !fr_eq(fr_from_mont(acc, canonical), one);
}

// arguments checked by the caller.  threads: 0 = as many as the machine has, at most 16; never more than one per string
void product_host(const ProductArgs &a, unsigned threads) {
    if (a.b_count == 0) return;
    over_threads(a.b_count, rows_host_threads(threads), [&a](size_t b0, size_t b1) {
        for (size_t bi = b0; bi < b1; ++bi) {
            uint32_t open = 0;
            for (uint32_t c = 0; c < a.ncols; ++c)
                if (product_lookup_host(a, bi, c) && c < kPdMaxOpenCols) open |= 1u << c;
            if (a.open) a.open[bi] = open;
        }
    });
}

}  // namespace hrx
