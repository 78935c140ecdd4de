// hrx_ntt_host.cpp — the host form of FR NTT (include/hrx.h hrx_fr_ntt_host): the rule of hrx_ntt.hpp over columns in host memory, an iterative radix-2
// transform per column over threads by ranges of columns.  It computes its own twiddles (one chain of 2^(k-1) products per call) and takes no workspace.
// No HIP; the host twin of hrx_kernel_ntt.hip and the definition of the cells.  tests/host_cpp/test_ntt_host.cpp includes this file as it is.
#include <vector>

#include "hrx_ntt.hpp"
#include "hrx_over_threads.hpp"

namespace hrx {

// arguments checked by the caller.  threads: 0 = as many as the machine has, at most 16; never more than one per column
void ntt_host(const NttArgs &a, unsigned threads) {
    if (a.n_cols == 0) return;
    const uint32_t k = a.k, n = 1u << k;
    const bool inverse = a.inverse != 0;
    std::vector<Fr> table(ntt_table_cells(k));                      // w^e, e < 2^(k-1)
    {
        const Fr w = ntt_omega(k);
        Fr cur = fr_R();
        for (Fr &e : table) {
            e = cur;
            cur = fr_mul(cur, w);
        }
    }
    const Fr g = a.shift ? ntt_shift(a.shift, a.canonical != 0) : fr_R(), scale = ntt_inv_n(k);
    over_threads(a.n_cols, rows_host_threads(threads), [&](size_t c0, size_t c1) {
        std::vector<Fr> x(n);
        for (size_t c = c0; c < c1; ++c) {
            const uint64_t *in = a.in + c * a.in_pitch * 4u;
            uint64_t *out = a.out + c * a.out_pitch * 4u;
            Fr pw = fr_R();
            for (uint32_t i = 0; i < n; ++i) {                        // x[rev(i)] = g^i in[i]; entries from n_in on are zero and never read
                Fr &d = x[ntt_bit_reverse(i, k)];
                if (i >= a.n_in) {
                    d = Fr{};
                    continue;
                }
                d = fr_load_cell(in + (size_t)i * 4u);
                if (a.shift && !inverse) {
                    d = fr_mul(d, pw);
                    pw = fr_mul(pw, g);
                }
            }
            for (uint32_t s = 0; s < k; ++s) {
                const uint32_t half = 1u << s;
                for (uint32_t j = 0; j < n / 2u; ++j) {
                    const uint32_t pos = j & (half - 1u), i0 = ((j >> s) << (s + 1u)) | pos;
                    bool neg;
                    const uint32_t e = ntt_twiddle_index(k, s, pos, inverse, neg);
                    ntt_butterfly(x[i0], x[i0 + half], table[e], neg);
                }
            }
            if (inverse) {
                pw = scale;
                for (uint32_t i = 0; i < n; ++i) {                    // 2^-k g^i
                    x[i] = fr_mul(x[i], pw);
                    if (a.shift) pw = fr_mul(pw, g);
                }
            }
            for (uint32_t i = 0; i < n; ++i) fr_store_cell(out + (size_t)i * 4u, x[i]);
        }
    });
}

}  // namespace hrx
