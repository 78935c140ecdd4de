// hrx_ntt.hpp — the rule of FR NTT (include/hrx.h: hrx_fr_ntt_*) that must exist once: the number-theoretic transform of size 2^k over columns of
// bn256::Fr cells, what halo2 does next with every Lagrange column the lookup stages write (lagrange_to_coeff, coeff_to_extended, extended_to_coeff).
// No HIP dependency: the kernels (hrx_kernel_ntt.hip), the host form (hrx_ntt_host.cpp), the planner (hrx_ntt_api.cpp) and
// tests/host_cpp/test_ntt_host.cpp include it.
//
// One column x[0 .. 2^k), natural order in and out, w = ROOT_OF_UNITY^(2^(28 - k)) (hrx_fr.h), g the call's shift (1 where there is none):
//   forward:  y[j] = sum_i (g^i x[i]) w^(i j)
//   inverse:  y[i] = g^i 2^-k sum_j x[j] w^(-i j)
// Input entries [n_in, 2^k) are zero and never read; output entries [0, 2^k) are written and none above.  Every cell written is a fully reduced element, so
// two implementations agree limb for limb whatever their order of operations.
//
// Limb forms.  The transform is linear and its twiddles are Montgomery forms: fr_mul of a cell with a twiddle w R is the cell times w in WHATEVER form the
// cell is, so a plain integer x — the Montgomery form of x / R — goes through unconverted and comes out plain.  Only the shift is read by its form: a plain
// g is taken into Montgomery form (times R^2) before its powers are formed.  HRX_FR_CANONICAL costs one fr_mul per call, none per cell.
//
// How both implementations compute it: x g^i (forward), the bit-reversal permutation, then k radix-2 decimation-in-time stages s = 0 .. k - 1 — stage s
// pairs entries 2^s apart, (a, b) -> (a + t b, a - t b) with t = w^((index mod 2^s) 2^(k - 1 - s)) — then 2^-k g^i (inverse).  The inverse direction reads
// the same table: w^-e = -w^(2^(k-1) - e) for 0 < e < 2^(k-1), so its butterfly is (a - t' b, a + t' b) with t' = w^(2^(k-1) - e), and e = 0 is 1.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hrx_fr.h"

namespace hrx {

constexpr uint32_t kNttMaxK = 24;
// ---- how a device call cuts its work (hrx_kernel_ntt.hip) ---------------------------------------------------------------------------------------------
// A workgroup of kNttThreads lanes holds a tile of cells in LDS and runs a range of stages on it.  k <= kNttTileBits: one launch, a whole column per
// workgroup — below kNttPackBits, 2^(kNttPackBits - k) columns per workgroup.  Above: one launch that permutes (bit reversal: an involution, so the in-place
// form is swaps of block pairs), then one launch per pass: stages [0, kNttTileBits) on contiguous tiles, the others kNttStridedBits or fewer at a time on
// tiles of 2^bits rows 2^s0 cells apart and 2^(kNttTileBits - bits) adjacent cells wide (whole lines: at least 64 cells, 2 KiB).
constexpr uint32_t kNttThreadBits = 9, kNttThreads = 1u << kNttThreadBits;   // 512 lanes
constexpr uint32_t kNttTileBits = 12;               // 4096 cells, 128 KiB of LDS
constexpr uint32_t kNttPackBits = 10;               // the smallest tile: 1024 cells, 32 KiB
constexpr uint32_t kNttStridedBits = 6;
constexpr uint32_t kNttMaxPasses = 3;
constexpr uint32_t kNttPermuteBits = 4;             // the permuting launch moves blocks of 16 runs of 16 cells

struct NttPlan {
    uint32_t n_passes, pass_bits[kNttMaxPasses], cols_per_group, launches;
};
HRX_HD NttPlan ntt_plan(uint32_t k) {
    NttPlan p = {1u, {k, 0u, 0u}, 1u, 1u};
    if (k <= kNttTileBits) {
        if (k < kNttPackBits) p.cols_per_group = 1u << (kNttPackBits - k);
        return p;
    }
    const uint32_t rem = k - kNttTileBits, n = (rem + kNttStridedBits - 1u) / kNttStridedBits;
    p.n_passes = 1u + n;
    p.pass_bits[0] = kNttTileBits;
    for (uint32_t j = 0; j < n; ++j) p.pass_bits[1u + j] = rem / n + (j < rem % n ? 1u : 0u);
    p.launches = 1u + p.n_passes;
    return p;
}

// The workspace of size 2^k: the table w^e, e < max(1, 2^(k-1)), then 2^-k; Montgomery forms, 8 u32 limbs a cell.  Written by one launch, read-only after.
HRX_HD size_t ntt_table_cells(uint32_t k) { return k > 1u ? (size_t)1 << (k - 1u) : 1u; }
HRX_HD size_t ntt_workspace_bytes(uint32_t k) { return ((ntt_table_cells(k) + 1u) * 32u + 255u) & ~(size_t)255; }

// w = ROOT_OF_UNITY^(2^(28 - k)), the primitive 2^k-th root (Montgomery form)
HRX_HD Fr ntt_omega(uint32_t k) { return fr_square_n(fr_root_of_unity(), kFrS - k); }
// 2^-k (Montgomery form)
HRX_HD Fr ntt_inv_n(uint32_t k) { return fr_pow_u32(fr_half(), k); }
// the shift as the Montgomery form its powers are formed from: 4 u64 limbs of any 256-bit value in the call's limb form, taken mod r first
HRX_HD Fr ntt_shift(const uint64_t *p, bool canonical) { return fr_to_mont(fr_challenge(p), canonical); }
// one butterfly: (a, b) -> (a + t b, a - t b), the two swapped where `neg` (the inverse direction's -t)
HRX_HD void ntt_butterfly(Fr &a, Fr &b, const Fr &t, bool neg) {
    const Fr tb = fr_mul(b, t), s = fr_add(a, tb), d = fr_sub(a, tb);
    a = fr_select(neg, d, s);
    b = fr_select(neg, s, d);
}
// which table entry stage s reads for the entry whose index mod 2^s is `pos`, and whether it stands for its negative
HRX_HD uint32_t ntt_twiddle_index(uint32_t k, uint32_t s, uint32_t pos, bool inverse, bool &neg) {
    const uint32_t e = pos << (k - 1u - s);
    neg = inverse && e != 0u;
    return neg ? (1u << (k - 1u)) - e : e;
}
HRX_HD uint32_t ntt_bit_reverse(uint32_t i, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t b = 0; b < bits; ++b) r |= ((i >> b) & 1u) << (bits - 1u - b);
    return r;
}

// What a transform call is told (pitches in cells)
struct NttArgs {
    const uint64_t *in;                             // [n_cols][in_pitch][4]
    uint64_t *out;                                  // [n_cols][out_pitch][4]
    size_t in_pitch, out_pitch;
    uint32_t n_cols, k, n_in, inverse, canonical;
    const uint64_t *shift;                          // 4 limbs, or NULL (g = 1)
    const uint32_t *ws;                             // the device form's workspace
};

}  // namespace hrx
