// hrx_quotient_host.cpp — the host forms of LOOKUP QUOTIENT (include/hrx.h hrx_fr_vanishing_inverse_host / hrx_lookup_quotient_host): the rule of
// hrx_quotient.hpp over columns in host memory, over threads by ranges of strings, point after point, v carried across a string's lookups.  No HIP; the host
// twin of hrx_kernel_quotient.hip and the definition of the cells.  tests/host_cpp/test_quotient_host.cpp includes this file as it is.
#include "hrx_over_threads.hpp"
#include "hrx_quotient.hpp"

namespace hrx {

// arguments checked by the caller
void vanishing_inverse_host(const VanishArgs &a) {
    const Fr g = a.shift ? ntt_shift(a.shift, a.canonical != 0) : fr_R();
    for (uint32_t c = 0; c < (1u << (a.ext_k - a.k)); ++c)
        fr_store_cell(a.t_inv + (size_t)c * 4u, quotient_vanishing_inverse(g, a.k, a.ext_k, c, a.canonical != 0));
}

// the cells of one lookup at one point as quotient_lookup reads them
struct HostCells {
    const uint64_t *pz, *pz_next, *pa, *pap, *pap_prev, *ps, *psp;
    Fr z() const { return fr_load_cell(pz); }
    Fr z_next() const { return fr_load_cell(pz_next); }
    Fr a() const { return fr_load_cell(pa); }
    Fr ap() const { return fr_load_cell(pap); }
    Fr ap_prev() const { return fr_load_cell(pap_prev); }
    Fr s() const { return fr_load_cell(ps); }
    Fr sp() const { return fr_load_cell(psp); }
};

// arguments checked by the caller.  threads: 0 = as many as the machine has, at most 16; never more than one per string
void quotient_host(const QuotientArgs &a, unsigned threads) {
    if (a.b_count == 0) return;
    over_threads(a.b_count, rows_host_threads(threads), [&a](size_t b0, size_t b1) {
        const bool canonical = a.canonical != 0;
        const uint32_t N = 1u << a.ext_k, rot = 1u << (a.ext_k - a.k);
        for (size_t bi = b0; bi < b1; ++bi) {
            QuotientConsts q;
            quotient_consts(q, a.beta + bi * a.challenge_stride, a.gamma + bi * a.challenge_stride, a.y + bi * a.challenge_stride, canonical);
            const uint64_t *h_in = a.h_in ? a.h_in + bi * a.h_pitch * 4u : nullptr;
            uint64_t *h_out = a.h_out + bi * a.h_pitch * 4u;
            for (uint32_t j = 0; j < N; ++j) {
                const uint32_t jn = (j + rot) & (N - 1u), jp = (j - rot) & (N - 1u);
                const QuotientSel sel = quotient_selectors(fr_load_cell(a.selectors + (size_t)j * 4u), fr_load_cell(a.selectors + (a.sel_pitch + j) * 4u),
                                                           fr_load_cell(a.selectors + (2u * a.sel_pitch + j) * 4u), q);
                Fr v = h_in ? fr_load_cell(h_in + (size_t)j * 4u) : Fr{};
                for (uint32_t c = 0; c < a.ncols; ++c) {
                    const size_t col = ((size_t)c * a.b_count + bi) * a.pitch * 4u;
                    const uint64_t *A = a.a_ext + col, *Ap = a.ap_ext + col, *Sp = a.sp_ext + col, *Z = a.z_ext + col;
                    const uint64_t *S = a.s_ext + ((size_t)c * (a.s_stride ? a.b_count : 1u) + (a.s_stride ? bi : 0u)) * a.s_pitch * 4u;
                    const HostCells x = {Z + (size_t)j * 4u, Z + (size_t)jn * 4u, A + (size_t)j * 4u, Ap + (size_t)j * 4u, Ap + (size_t)jp * 4u, S + (size_t)j * 4u,
                                         Sp + (size_t)j * 4u};
                    v = quotient_lookup(v, x, q, sel);
                }
                if (a.divide) v = quotient_divide(v, fr_to_mont(fr_load_cell(a.t_inv + (size_t)(j & (rot - 1u)) * 4u), canonical));
                fr_store_cell(h_out + (size_t)j * 4u, v);
            }
        }
    });
}

}  // namespace hrx
