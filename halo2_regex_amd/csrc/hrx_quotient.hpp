// hrx_quotient.hpp — the rule of LOOKUP QUOTIENT (include/hrx.h: hrx_fr_vanishing_inverse_* / hrx_lookup_quotient_*) that must exist once: the lookup part
// of halo2's evaluate_h — the five constraint expressions of every lookup at every point of the extended coset, folded into the quotient accumulator with the
// challenge y, and the division by the vanishing polynomial.  No HIP dependency: the kernels (hrx_kernel_quotient.hip), the host forms
// (hrx_quotient_host.cpp), the planner (hrx_quotient_api.cpp) and tests/host_cpp/test_quotient_host.cpp include it.
//
// n = 2^k, e = ext_k - k, N = 2^ext_k, rot = 2^e.  Point j of the extended coset is g w_ext^j, so p(w X) at point j is p at point (j + rot) mod N and
// p(w^-1 X) is p at point (j - rot) mod N.  For one string, lookups c = 0 .. 3 D - 1 in hrx_lookup_num_columns' order, for every point j, v = h_in[j] (0
// without h_in), every lookup in halo2's order:
//   v = v y + (1 - Z[j]) l0[j]
//   v = v y + (Z[j]^2 - Z[j]) l_last[j]
//   v = v y + (Z[j + rot] (A'[j] + beta) (S'[j] + gamma) - Z[j] (A[j] + beta) (S[j] + gamma)) l_active[j]
//   v = v y + (A'[j] - S'[j]) l0[j]
//   v = v y + (A'[j] - S'[j]) (A'[j] - A'[j - rot]) l_active[j]
// and h_out[j] = v, or v t_inv[j mod rot] with HRX_QUOTIENT_DIVIDE: t_inv[c] = 1 / (g^n w_ext^(n c) - 1), the rot values X^n - 1 takes on the coset, the
// zero cell where that is zero.  Every cell written is a fully reduced element, so two implementations agree limb for limb.
//
// How both implementations compute a lookup (the same field element, 12 products instead of 16): with d = A' - S',
//   v y^5 + ((1 - Z) y^3 + d) [l0 y] + d (A' - A'[j - rot]) [l_active] + Z (Z - 1) [l_last y^3] + (Z[j + rot] (A' + beta)(S' + gamma) - Z (A + beta)(S + gamma)) [l_active y^2]
// where the four bracketed values depend on the point and the string only: four products per point, whatever the number of lookups.  (A fifth bracket
// [l0 y^4] saves one product a lookup and costs eight more registers a lane over the whole loop: with it the kernel keeps two waves a SIMD instead of three.)
//
// Limb forms.  The expressions are not linear in the cells, so a canonical call (plain integers) cannot run through unconverted as the NTT does.  The
// conversion is paid per POINT, not per cell: fr_mul of limbs a and b is a b / R, so a product of m plain cells is their product over R^(m-1), and the
// bracketed value it meets carries R^m — the Montgomery form times the R^(m-1) that is missing.  The four brackets come out of one fr_mul each of the
// selector's cell with a constant of the string (y^p R^q, QuotientConsts) in either form; cells, beta, gamma, v and h stay in the call's form from load to
// store.  What canonical costs: four products more where the constants are formed (once per string; per tile on the device), one per lane for t_inv, none
// per cell.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hrx_fr.h"
#include "hrx_ntt.hpp"          // ntt_omega, ntt_shift, kNttMaxK

namespace hrx {

constexpr uint32_t kQtMaxExtBits = 6;               // 1 <= ext_k - k <= 6: rot <= 64
constexpr uint32_t kQtMaxRot = 1u << kQtMaxExtBits;
// ---- how a device call cuts its work (hrx_kernel_quotient.hip): a workgroup of kQtThreads lanes takes kQtTileCells consecutive points of one string, one
// point per lane, and carries v in registers across all lookups
constexpr uint32_t kQtThreads = 256;
constexpr uint32_t kQtCellsPerLane = 1;
constexpr uint32_t kQtTileCells = kQtThreads * kQtCellsPerLane;
static_assert(kQtTileCells % kQtMaxRot == 0, "a lane's points share one t_inv entry: the tile is a multiple of every rot");

// Between the products of a lookup on the device: nothing is scheduled across.  The products are independent enough that the compiler otherwise
// interleaves them for latency and holds every operand at once — 250 VGPRs instead of 160.
#if defined(__HIP_DEVICE_COMPILE__)
#define HRX_QT_STEP() __builtin_amdgcn_sched_barrier(0)
#else
#define HRX_QT_STEP() ((void)0)
#endif

// What a string's challenges give every point: beta, gamma and one in the call's form, y^5 as a Montgomery form, and the constants the selectors meet
struct QuotientConsts {
    Fr beta, gamma, y3, y5, k_l0y, k_last, k_act3, k_act, one;
};
// Three products; canonical: seven.  Written member by member (on the device q lies in LDS: no value waits in registers for the others).
HRX_HD void quotient_consts(QuotientConsts &q, const uint64_t *beta, const uint64_t *gamma, const uint64_t *y, bool canonical) {
    q.beta = fr_challenge(beta);
    q.gamma = fr_challenge(gamma);
    q.one = fr_unit(canonical);
    // a selector cell s in the call's form times k is the bracket: s y^p R^m for the m plain cells it meets (Montgomery cells: s y^p R whatever m)
    q.k_act = fr_select(canonical, fr_R3(), fr_R());             // meets Delta, then d: two cells, the sum with [l0 y] between them
    const Fr y1 = fr_to_mont(fr_challenge(y), canonical);
    HRX_QT_STEP();
    q.k_l0y = canonical ? fr_mul(y1, fr_R2()) : y1;              // meets d, beside [l_active] Delta: one cell
    HRX_QT_STEP();
    const Fr y2 = fr_mul(y1, y1);
    HRX_QT_STEP();
    q.k_act3 = canonical ? fr_mul(y2, fr_R4()) : y2;             // meets Z (A + beta)(S + gamma): three cells
    HRX_QT_STEP();
    const Fr y3 = fr_mul(y2, y1);
    HRX_QT_STEP();
    q.y3 = y3;
    q.k_last = canonical ? fr_mul(y3, fr_R3()) : y3;             // meets Z (Z - 1): two cells
    HRX_QT_STEP();
    q.y5 = fr_mul(y3, y2);
}

// The brackets of one point
struct QuotientSel {
    Fr l0y, last, act3, act;
};
HRX_HD QuotientSel quotient_selectors(const Fr &l0, const Fr &l_last, const Fr &l_active, const QuotientConsts &q) {
    QuotientSel s;
    s.l0y = fr_mul(l0, q.k_l0y);
    HRX_QT_STEP();
    s.last = fr_mul(l_last, q.k_last);
    HRX_QT_STEP();
    s.act3 = fr_mul(l_active, q.k_act3);
    HRX_QT_STEP();
    s.act = fr_mul(l_active, q.k_act);
    HRX_QT_STEP();
    return s;
}

// The cells of one lookup at one point, in the call's form, are handed over as a type X with the members z(), z_next(), a(), ap(), ap_prev(), s(), sp() —
// Z[j], Z[j + rot], A[j], A'[j], A'[j - rot], S[j], S'[j] — each read where a product needs it: the device reads LDS, the host memory.
// v after the lookup's five steps (12 fr_mul), one product at a time
template <class X>
HRX_HD Fr quotient_lookup(const Fr &v, const X &x, const QuotientConsts &q, const QuotientSel &s) {
    Fr acc = fr_mul(v, q.y5);
    HRX_QT_STEP();
    const Fr u = fr_add(fr_mul(fr_sub(q.one, x.z()), q.y3), fr_sub(x.ap(), x.sp()));
    HRX_QT_STEP();
    acc = fr_add(acc, fr_mul(u, s.l0y));
    HRX_QT_STEP();
    const Fr t = fr_mul(fr_sub(x.ap(), x.sp()), fr_sub(x.ap(), x.ap_prev()));
    HRX_QT_STEP();
    acc = fr_add(acc, fr_mul(t, s.act));
    HRX_QT_STEP();
    const Fr w = fr_mul(x.z(), fr_sub(x.z(), q.one));
    HRX_QT_STEP();
    acc = fr_add(acc, fr_mul(w, s.last));
    HRX_QT_STEP();
    Fr left = fr_mul(x.z_next(), fr_add(x.ap(), q.beta));
    HRX_QT_STEP();
    left = fr_mul(left, fr_add(x.sp(), q.gamma));
    HRX_QT_STEP();
    Fr right = fr_mul(x.z(), fr_add(x.a(), q.beta));
    HRX_QT_STEP();
    right = fr_mul(right, fr_add(x.s(), q.gamma));
    HRX_QT_STEP();
    return fr_add(acc, fr_mul(fr_sub(left, right), s.act3));
}
// h_out's cell with HRX_QUOTIENT_DIVIDE: t_mont is the point's t_inv entry as a Montgomery form (fr_to_mont of the table's cell)
HRX_HD Fr quotient_divide(const Fr &v, const Fr &t_mont) { return fr_mul(v, t_mont); }

// t_inv[c], c < 2^(ext_k - k), in the call's form; g a Montgomery form (ntt_shift)
HRX_HD Fr quotient_vanishing_inverse(const Fr &g, uint32_t k, uint32_t ext_k, uint32_t c, bool canonical) {
    const Fr gn = fr_square_n(g, k), wn = ntt_omega(ext_k - k);          // g^n; w_ext^n: the primitive rot-th root
    return fr_from_mont(fr_inv(fr_sub(fr_mul(gn, fr_pow_u32(wn, c)), fr_R())), canonical);
}

// What a quotient call is told (pitches in cells)
struct QuotientArgs {
    const uint64_t *a_ext, *ap_ext, *sp_ext, *z_ext;        // [ncols][b_count][pitch][4] each
    const uint64_t *s_ext;                                  // [ncols][runs][s_pitch][4]
    const uint64_t *selectors;                              // [3][sel_pitch][4]: l0, l_last, l_active
    const uint64_t *beta, *gamma, *y;
    const uint64_t *h_in;                                   // [b_count][h_pitch][4], or NULL
    uint64_t *h_out;
    const uint64_t *t_inv;                                  // [rot][4]; NULL without `divide`
    size_t pitch, s_pitch, sel_pitch, h_pitch;
    uint32_t b_count, ncols, k, ext_k, s_stride, challenge_stride, canonical, divide;
};

// What a vanishing-inverse call is told
struct VanishArgs {
    const uint64_t *shift;                                  // 4 limbs, or NULL (g = 1: entry 0 the zero cell)
    uint64_t *t_inv;
    uint32_t k, ext_k, canonical;
};

}  // namespace hrx
