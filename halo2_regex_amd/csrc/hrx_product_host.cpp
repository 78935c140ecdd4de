// hrx_product_host.cpp — the host forms of LOOKUP PRODUCT (include/hrx.h hrx_lookup_invert_table_host / hrx_lookup_product_host): the rule of
// hrx_product.hpp over cells, indices and outputs in host memory — the inverse tables over threads by ranges of runs (batch inversion per run: prefix
// products, one fr_inv, the walk back), the product over threads by ranges of strings, row after row.  No HIP; the host twins of hrx_kernel_product.hip and
// the definition of the cells.  tests/host_cpp/test_product_host.cpp includes this file as it is.
#include <vector>

#include "hrx_over_threads.hpp"
#include "hrx_product.hpp"

namespace hrx {

static void product_challenge(const uint64_t *p, uint32_t (&w)[8]) {
    product_get_cell(p, w);
    fr_reduce(w);
}

// arguments checked by the caller.  threads: 0 = as many as the machine has, at most 16; never more than one per run
void invert_table_host(const InvertArgs &a, unsigned threads) {
    if (a.n_runs == 0 || a.W == 0) return;
    over_threads(a.n_runs, rows_host_threads(threads), [&a](size_t r0, size_t r1) {
        const bool canonical = a.canonical != 0;
        std::vector<uint32_t> el((size_t)a.bins * 8u);          // the run's elements: S + c in Montgomery form, one where that is zero
        std::vector<uint8_t> zero(a.bins);
        for (size_t run = r0; run < r1; ++run) {
            const uint64_t *S = a.table + run * a.W * 4u;
            uint64_t *out = a.inv + run * a.W * 4u;
            uint32_t c[8], acc[8], t[8];
            product_challenge(a.shift + run * a.shift_stride, c);
            fr_one(false, acc);
            for (uint32_t w = 0; w < a.bins; ++w) {              // out[w] = the product of the elements before w
                uint32_t s[8], sc[8], x[8];
                product_get_cell(S + (size_t)w * 4u, s);
                fr_add(s, c, sc);
                zero[w] = fr_is_zero(sc);
                product_to_mont(sc, canonical, x);
                if (zero[w]) fr_one(false, x);
                for (int i = 0; i < 8; ++i) el[(size_t)w * 8u + i] = x[i];
                product_put_cell(out + (size_t)w * 4u, acc);
                fr_mul(acc, x, t);
                for (int i = 0; i < 8; ++i) acc[i] = t[i];
            }
            uint32_t back[8];                                    // 1 / (the elements up to w)
            fr_inv(acc, back);
            for (uint32_t w = a.bins; w-- > 0u;) {
                uint32_t pre[8], x[8], inv[8], res[8];
                product_get_cell(out + (size_t)w * 4u, pre);
                fr_mul(back, pre, inv);
                product_from_mont(inv, canonical, res);
                if (zero[w])
                    for (int i = 0; i < 8; ++i) res[i] = 0u;
                product_put_cell(out + (size_t)w * 4u, res);
                for (int i = 0; i < 8; ++i) x[i] = el[(size_t)w * 8u + i];
                fr_mul(back, x, t);
                for (int i = 0; i < 8; ++i) back[i] = t[i];
            }
            for (uint32_t w = a.bins; w < a.W; ++w) out[(size_t)w * 4u] = out[(size_t)w * 4u + 1] = out[(size_t)w * 4u + 2] = out[(size_t)w * 4u + 3] = 0;
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
    uint32_t beta[8], gamma[8], s0[8], acc[8], res[8], one[8];
    product_challenge(a.beta + bi * a.challenge_stride, beta);
    product_challenge(a.gamma + bi * a.challenge_stride, gamma);
    product_get_cell(run + (size_t)L.off * 4u, s0);
    fr_one(false, acc);
    fr_one(canonical, one);
    product_put_cell(z, one);
    for (uint32_t i = 0; i < a.n_rows; ++i) {
        uint32_t t[8];
        const uint32_t ia = a_idx[i], is = s_idx[i];
        if (!product_index_ok(ia, L.off, L.T) || !product_index_ok(is, L.off, L.T)) {     // no index is an address before the test
            for (int l = 0; l < 8; ++l) t[l] = 0u;
        } else {
            uint32_t A[8], S[8], ab[8], sg[8], ib[8], ig[8];
            if (product_input_is_dummy(k3, i, M, n)) for (int l = 0; l < 8; ++l) A[l] = s0[l];
            else product_get_cell(in + (size_t)i * 4u, A);
            product_get_cell(run + (size_t)(L.off + product_table_row(i, L.T)) * 4u, S);
            fr_add(A, beta, ab);
            fr_add(S, gamma, sg);
            product_get_cell(ib_run + (size_t)ia * 4u, ib);
            product_get_cell(ig_run + (size_t)is * 4u, ig);
            product_term(ab, sg, ib, ig, canonical, t);
        }
        uint32_t nx[8];
        fr_mul(acc, t, nx);
        for (int l = 0; l < 8; ++l) acc[l] = nx[l];
        product_from_mont(acc, canonical, res);
        product_put_cell(z + (size_t)(i + 1u) * 4u, res);
    }
    product_from_mont(acc, canonical, res);
    return !fr_eq(res, one);
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
