// hrx_ntt_host.cpp — the host form of FR NTT (include/hrx.h hrx_fr_ntt_host): the rule of hrx_ntt.hpp over columns in host memory, an iterative radix-2
// transform per column over threads by ranges of columns.  It computes its own twiddles (one chain of 2^(k-1) products per call) and takes no workspace.
// No HIP; the host twin of hrx_kernel_ntt.hip and the definition of the cells.  tests/host_cpp/test_ntt_host.cpp includes this file as it is.
#include <vector>

#include "hrx_ntt.hpp"
#include "hrx_over_threads.hpp"

namespace hrx {

static void ntt_get_cell(const uint64_t *cell, uint32_t *w) {
    for (int i = 0; i < 4; ++i) { w[2 * i] = (uint32_t)cell[i]; w[2 * i + 1] = (uint32_t)(cell[i] >> 32); }
}
static void ntt_put_cell(uint64_t *cell, const uint32_t *w) {
    for (int i = 0; i < 4; ++i) cell[i] = (uint64_t)w[2 * i] | (uint64_t)w[2 * i + 1] << 32;
}
typedef uint32_t NttCell[8];

// arguments checked by the caller.  threads: 0 = as many as the machine has, at most 16; never more than one per column
void ntt_host(const NttArgs &a, unsigned threads) {
    if (a.n_cols == 0) return;
    const uint32_t k = a.k, n = 1u << k;
    const bool inverse = a.inverse != 0;
    std::vector<uint32_t> table(ntt_table_cells(k) * 8u);           // w^e, e < 2^(k-1)
    {
        uint32_t w[8], cur[8], t[8];
        ntt_omega(k, w);
        fr_one(false, cur);
        for (size_t e = 0; e < ntt_table_cells(k); ++e) {
            for (int i = 0; i < 8; ++i) table[e * 8u + i] = cur[i];
            fr_mul(cur, w, t);
            for (int i = 0; i < 8; ++i) cur[i] = t[i];
        }
    }
    uint32_t g[8], scale[8];
    if (a.shift) ntt_shift(a.shift, a.canonical != 0, g);
    if (inverse) ntt_inv_n(k, scale);
    over_threads(a.n_cols, rows_host_threads(threads), [&](size_t c0, size_t c1) {
        std::vector<uint32_t> buf((size_t)n * 8u);
        NttCell *x = reinterpret_cast<NttCell *>(buf.data());
        for (size_t c = c0; c < c1; ++c) {
            const uint64_t *in = a.in + c * a.in_pitch * 4u;
            uint64_t *out = a.out + c * a.out_pitch * 4u;
            uint32_t pw[8], t[8];
            fr_one(false, pw);
            for (uint32_t i = 0; i < n; ++i) {                        // x[rev(i)] = g^i in[i]; entries from n_in on are zero and never read
                uint32_t *d = x[ntt_bit_reverse(i, k)];
                if (i >= a.n_in) {
                    for (int l = 0; l < 8; ++l) d[l] = 0u;
                    continue;
                }
                uint32_t v[8];
                ntt_get_cell(in + (size_t)i * 4u, v);
                if (a.shift && !inverse) {
                    fr_mul(v, pw, t);
                    for (int l = 0; l < 8; ++l) d[l] = t[l];
                    fr_mul(pw, g, t);
                    for (int l = 0; l < 8; ++l) pw[l] = t[l];
                } else {
                    for (int l = 0; l < 8; ++l) d[l] = v[l];
                }
            }
            for (uint32_t s = 0; s < k; ++s) {
                const uint32_t half = 1u << s;
                for (uint32_t j = 0; j < n / 2u; ++j) {
                    const uint32_t pos = j & (half - 1u), i0 = ((j >> s) << (s + 1u)) | pos;
                    bool neg;
                    const uint32_t e = ntt_twiddle_index(k, s, pos, inverse, neg);
                    ntt_butterfly(x[i0], x[i0 + half], *reinterpret_cast<const NttCell *>(&table[(size_t)e * 8u]), neg);
                }
            }
            if (inverse) {
                for (int l = 0; l < 8; ++l) pw[l] = scale[l];
                for (uint32_t i = 0; i < n; ++i) {                    // 2^-k g^i
                    fr_mul(x[i], pw, t);
                    for (int l = 0; l < 8; ++l) x[i][l] = t[l];
                    if (a.shift) {
                        fr_mul(pw, g, t);
                        for (int l = 0; l < 8; ++l) pw[l] = t[l];
                    }
                }
            }
            for (uint32_t i = 0; i < n; ++i) ntt_put_cell(out + (size_t)i * 4u, x[i]);
        }
    });
}

}  // namespace hrx
