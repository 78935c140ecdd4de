// hrx_fr.h — F::from(u64) for F = halo2curves bn256::Fr, the field the reference's circuits are instantiated with
// (src/lib.rs:896, examples/regex.rs:9), as 4 little-endian u64 limbs in Montgomery form.
//
// halo2curves (pulled in through halo2-base v0.2.2, Cargo.toml:12-15; not vendored in the reference) represents an
// element x as the limbs of x * R mod r with R = 2^256, and `From<u64>` is `Fr([v,0,0,0]) * R2` = v * R mod r:
//   r  = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001     (BN254 scalar field)
//   R  = 2^256 mod r  = [ac96341c4ffffffb, 36fc76959f60cd29, 666ea36f7879462e, 0e0a77c19a07df2f]  (= Fr::one()'s limbs)
// Here v * R mod r is computed directly: q' = floor(v * K / 2^64) with K = floor(R * 2^64 / r) underestimates
// q = floor(v * R / r) by at most 2, so v * R - q' * r needs at most two corrective subtractions.  Plain C++ (unsigned
// __int128) so that hipcc compiles it for the kernel and g++/hipcc for the host-side known-answer tests.
// Below F::from: Fr, an element as a value of eight u32 limbs, and everything the stages compute with one — LOOKUP COMPRESS (hrx_compress.hpp), LOOKUP
// PRODUCT (hrx_product.hpp), FR NTT (hrx_ntt.hpp), LOOKUP QUOTIENT (hrx_quotient.hpp) and the field cells (hrx_kernel.hip).  Every function takes and returns Fr by value:
//   constants   fr_R (the Montgomery one), fr_R2, fr_R3, fr_R4, fr_R5, fr_half, fr_root_of_unity
//   arithmetic  fr_add, fr_sub, fr_mul (the Montgomery product), fr_reduce (any 256-bit value mod r), fr_inv (Fermat), fr_pow_u32, fr_square_n,
//               fr_select, fr_is_zero, fr_eq; fr_powers and fr_fold, the fold of a lookup tuple with a challenge's powers
//   limb forms  fr_unit, fr_to_mont, fr_from_mont — the one of a call's form, into and out of Montgomery form
//   memory      fr_load_cell (4 u64, below r by contract, NOT reduced), fr_store_cell, fr_challenge (4 u64, any 256-bit value, reduced)
// This file is the one place those rules live; hrx_fr_device.h adds the device's 16-byte loads and stores, shuffles and scalar broadcast.
#pragma once
#include <stdint.h>

#include "hrx_lane.h"

namespace hrx {

constexpr uint64_t kFrModulus[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
constexpr uint64_t kFrR[4] = {0xac96341c4ffffffbull, 0x36fc76959f60cd29ull, 0x666ea36f7879462eull, 0x0e0a77c19a07df2full};
constexpr uint64_t kFrK = 0x4a47462623a04a7aull;  // floor(R * 2^64 / r)

// out = v * R mod r (Montgomery form of v); canonical = true: out = v (the plain little-endian integer)
HRX_HD void fr_from_u64(uint64_t v, uint64_t (&out)[4], bool canonical = false) {
    if (canonical || v == 0) { out[0] = v; out[1] = out[2] = out[3] = 0; return; }
    typedef unsigned __int128 u128;
    // p = v * R (5 limbs), s = q' * r (5 limbs)
    const uint64_t q = (uint64_t)(((u128)v * kFrK) >> 64);
    uint64_t p[5], s[5];
    u128 c = 0, d = 0;
    for (int i = 0; i < 4; ++i) {
        c += (u128)v * kFrR[i];
        p[i] = (uint64_t)c;
        c >>= 64;
        d += (u128)q * kFrModulus[i];
        s[i] = (uint64_t)d;
        d >>= 64;
    }
    p[4] = (uint64_t)c;
    s[4] = (uint64_t)d;
    // t = p - s  (0 <= t < 3r)
    uint64_t t[5];
    uint64_t borrow = 0;
    for (int i = 0; i < 5; ++i) {
        const u128 x = (u128)p[i] - s[i] - borrow;
        t[i] = (uint64_t)x;
        borrow = (uint64_t)(x >> 64) & 1u;
    }
    for (int round = 0; round < 2; ++round) {  // t -= r while t >= r
        uint64_t u[5];
        uint64_t b = 0;
        for (int i = 0; i < 5; ++i) {
            const u128 x = (u128)t[i] - (i < 4 ? kFrModulus[i] : 0) - b;
            u[i] = (uint64_t)x;
            b = (uint64_t)(x >> 64) & 1u;
        }
        if (!b) { t[0] = u[0]; t[1] = u[1]; t[2] = u[2]; t[3] = u[3]; t[4] = u[4]; }
    }
    out[0] = t[0]; out[1] = t[1]; out[2] = t[2]; out[3] = t[3];
}

// The same for v < 2^32 on 32-bit limbs (every value of the compact witness is 16 bits or less): v_mad_u64_u32 chains,
// ~4x fewer instructions than the 64-bit form.  K32 = floor(R * 2^32 / r); q' underestimates q by at most 2.
constexpr uint32_t kFrR32[8] = {0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u};
constexpr uint32_t kFrModulus32[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
constexpr uint32_t kFrK32 = 0x4a474626u;

// An element: eight little-endian u32 limbs (the device's form; the host runs the same code).  Passed and returned by value.  Whether the limbs are
// the plain integer or its Montgomery form is the caller's knowledge — see "Limb forms" below.
struct Fr {
    uint32_t w[8];
};

// The loops index register arrays: every index is a constant once they are unrolled.
#if defined(__clang__)
#define HRX_FR_UNROLL _Pragma("unroll")
#define HRX_FR_NOUNROLL _Pragma("nounroll")
#else
#define HRX_FR_UNROLL
#define HRX_FR_NOUNROLL
#endif

HRX_HD Fr fr_from_u32(uint32_t v, bool canonical = false) {
    Fr out = {};
    if (canonical || v == 0) {
        out.w[0] = v;
        return out;
    }
    const uint32_t q = (uint32_t)(((uint64_t)v * kFrK32) >> 32);
    uint32_t t[9];
    uint64_t c = 0, d = 0;
    uint32_t borrow = 0;
    for (int i = 0; i < 8; ++i) {   // t = v * R - q * r, limb by limb
        c += (uint64_t)v * kFrR32[i];
        d += (uint64_t)q * kFrModulus32[i];
        const uint64_t x = (uint64_t)(uint32_t)c - (uint32_t)d - borrow;
        t[i] = (uint32_t)x;
        borrow = (uint32_t)(x >> 32) & 1u;
        c >>= 32;
        d >>= 32;
    }
    t[8] = (uint32_t)c - (uint32_t)d - borrow;
    for (int round = 0; round < 2; ++round) {  // t -= r while t >= r
        uint32_t u[9], b = 0;
        for (int i = 0; i < 9; ++i) {
            const uint64_t x = (uint64_t)t[i] - (i < 8 ? kFrModulus32[i] : 0u) - b;
            u[i] = (uint32_t)x;
            b = (uint32_t)(x >> 32) & 1u;
        }
        if (!b)
            for (int i = 0; i < 9; ++i) t[i] = u[i];
    }
    for (int i = 0; i < 8; ++i) out.w[i] = t[i];
    return out;
}

// ---- constants as elements.  Functions, not objects: device code may read the elements of a host constexpr array but not bind a reference to one.
constexpr uint32_t kFrInv32 = 0xefffffffu;          // -r^-1 mod 2^32
constexpr uint32_t kFrR2_32[8] = {0xae216da7u, 0x1bb8e645u, 0xe35c59e3u, 0x53fe3ab1u, 0x53bb8085u, 0x8c49833du, 0x7f4e44a5u, 0x0216d0b1u};   // R^2 mod r
constexpr uint32_t kFrR5_32[8] = {0xa17a2cefu, 0x00915951u, 0x9fd7425cu, 0xbf25f2ddu, 0xa7eeefb8u, 0xfb6cfdc4u, 0xb32c8ec9u, 0x06eaaa4fu};   // R^5 mod r
constexpr uint32_t kFrR3_32[8] = {0xb4bf0040u, 0x5e94d8e1u, 0x1cfbb6b8u, 0x2a489cbeu, 0xa19fcfedu, 0x893cc664u, 0x7fcc657cu, 0x0cf8594bu};   // R^3 mod r
constexpr uint32_t kFrR4_32[8] = {0x00bf2c45u, 0xabbc9482u, 0x4e532f3du, 0x48c48498u, 0xed8c1dd1u, 0x3adf4b7eu, 0xeceb8b73u, 0x1c022fc8u};   // R^4 mod r
constexpr uint32_t kFrRm2_32[8] = {0xefffffffu, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};  // r - 2 (254 bits)
constexpr uint32_t kFrFoldK = 0xa948e8c4u;          // floor(2^285 / r): the quotient estimate of fr_fold
// The two-adic subgroup, halo2curves' constants for bn256::Fr: r - 1 = 2^S * odd with S = 28, the multiplicative generator 7, and
// ROOT_OF_UNITY = 7^((r - 1) / 2^28) = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c of order exactly 2^28 (its 2^27-th power is r - 1).
// Both 32-bit limb arrays are Montgomery forms (x R mod r).
constexpr uint32_t kFrS = 28;
constexpr uint64_t kFrRootOfUnity[4] = {0xd34f1ed960c37c9cull, 0x3215cf6dd39329c8ull, 0x98865ea93dd31f74ull, 0x03ddb9f5166d18b7ull};   // the plain integer
constexpr uint32_t kFrRootOfUnity32[8] = {0xb639feb8u, 0x9632c7c5u, 0x0d0ff299u, 0x985ce340u, 0x01b0ecd8u, 0xb2dd8800u, 0x6d98ce29u, 0x1d69070du};
constexpr uint32_t kFrInv2_32[8] = {0x1ffffffeu, 0x783c14d8u, 0x0c8d1eddu, 0xaf982f6fu, 0xfcfd4f45u, 0x8f5f7492u, 0x3d9cbfacu, 0x1f37631au};         // 1 / 2

#define HRX_FR_CONSTANT(name, k) \
    HRX_HD constexpr Fr name() { return Fr{{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]}}; }
HRX_FR_CONSTANT(fr_R, kFrR32)                               // R: the Montgomery form of 1
HRX_FR_CONSTANT(fr_R2, kFrR2_32)                            // R^2: times it, a plain integer becomes its Montgomery form
HRX_FR_CONSTANT(fr_R3, kFrR3_32)                            // R^3, R^4: times them, a Montgomery form gains R^2, R^3 (LOOKUP QUOTIENT's selector constants)
HRX_FR_CONSTANT(fr_R4, kFrR4_32)
HRX_FR_CONSTANT(fr_R5, kFrR5_32)                            // R^5: times it, a product of four plain integers (x / R^3) becomes its Montgomery form
HRX_FR_CONSTANT(fr_half, kFrInv2_32)                        // 1 / 2, Montgomery form
HRX_FR_CONSTANT(fr_root_of_unity, kFrRootOfUnity32)         // ROOT_OF_UNITY, Montgomery form
#undef HRX_FR_CONSTANT

// ---- arithmetic on elements ----------------------------------------------------------------------------------------------------------------------
// c ? a : b, limb by limb (selects, no branch)
HRX_HD Fr fr_select(bool c, const Fr &a, const Fr &b) {
    Fr out;
HRX_FR_UNROLL
    for (int i = 0; i < 8; ++i) out.w[i] = c ? a.w[i] : b.w[i];
    return out;
}

// t -= m when t >= m; m = r << shift
template <int SHIFT>
HRX_HD void fr_sub_if_ge(Fr &t) {
    Fr u;
    uint32_t b = 0;
HRX_FR_UNROLL
    for (int i = 0; i < 8; ++i) {
        uint32_t m = kFrModulus32[i];
        if constexpr (SHIFT != 0) m = m << SHIFT | (i ? kFrModulus32[i ? i - 1 : 0] >> (32 - SHIFT) : 0u);
        const uint64_t x = (uint64_t)t.w[i] - m - b;
        u.w[i] = (uint32_t)x;
        b = (uint32_t)(x >> 32) & 1u;
    }
    if (!b) t = u;
}

// x mod r for any 256-bit x: 2^256 < 6 r and 4 r < 2^256, so x - [x >= 4r] 4r < 4r, then 2r and r are taken off where they fit
HRX_HD Fr fr_reduce(Fr x) {
    fr_sub_if_ge<2>(x);
    fr_sub_if_ge<1>(x);
    fr_sub_if_ge<0>(x);
    return x;
}

// a + b mod r, a and b below r (the sum is below 2^255: no carry out of the eight limbs)
HRX_HD Fr fr_add(const Fr &a, const Fr &b) {
    Fr out;
    uint64_t c = 0;
HRX_FR_UNROLL
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)a.w[i] + b.w[i];
        out.w[i] = (uint32_t)c;
        c >>= 32;
    }
    fr_sub_if_ge<0>(out);
    return out;
}

// a - b mod r, a and b below r: the difference, and r added back where it borrowed
HRX_HD Fr fr_sub(const Fr &a, const Fr &b) {
    Fr d, out;
    uint32_t borrow = 0;
HRX_FR_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint64_t x = (uint64_t)a.w[i] - b.w[i] - borrow;
        d.w[i] = (uint32_t)x;
        borrow = (uint32_t)(x >> 32) & 1u;
    }
    uint64_t c = 0;
HRX_FR_UNROLL
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)d.w[i] + (borrow ? kFrModulus32[i] : 0u);
        out.w[i] = (uint32_t)c;
        c >>= 32;
    }
    return out;
}

// a * b / R mod r — the Montgomery product: of two Montgomery forms the Montgomery form of the product; of a plain integer and a Montgomery form the
// plain product.  a, b below r.  Word-by-word (CIOS) over 32-bit limbs: per limb of b one row of a * b[i] and one of m * r that clears the lowest limb,
// 128 v_mad_u64_u32 in all; the running value stays below 2 r < 2^255, so one subtraction finishes.
HRX_HD Fr fr_mul(const Fr &a, const Fr &b) {
    uint32_t t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
HRX_FR_UNROLL
    for (int i = 0; i < 8; ++i) {
        uint64_t c = 0;
HRX_FR_UNROLL
        for (int j = 0; j < 8; ++j) {      // t += a * b[i]   (a[j] b[i] + t[j] + c <= 2^64 - 1)
            c += (uint64_t)a.w[j] * b.w[i] + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t[8];
        const uint32_t top = (uint32_t)(c >> 32);
        t[8] = (uint32_t)c;
        const uint32_t m = t[0] * kFrInv32;
        c = ((uint64_t)m * kFrModulus32[0] + t[0]) >> 32;      // the lowest limb of t + m r is 0
HRX_FR_UNROLL
        for (int j = 1; j < 8; ++j) {      // t = (t + m r) / 2^32
            c += (uint64_t)m * kFrModulus32[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t[8];
        t[7] = (uint32_t)c;
        t[8] = top + (uint32_t)(c >> 32);
    }
    Fr out;
HRX_FR_UNROLL
    for (int i = 0; i < 8; ++i) out.w[i] = t[i];      // (t[8] == 0: t < 2 r)
    fr_sub_if_ge<0>(out);
    return out;
}

HRX_HD bool fr_is_zero(const Fr &a) { return (a.w[0] | a.w[1] | a.w[2] | a.w[3] | a.w[4] | a.w[5] | a.w[6] | a.w[7]) == 0u; }
HRX_HD bool fr_eq(const Fr &a, const Fr &b) {
    uint32_t d = 0;
HRX_FR_UNROLL
    for (int i = 0; i < 8; ++i) d |= a.w[i] ^ b.w[i];
    return d == 0u;
}

// x^-1 in Montgomery form (x R -> x^-1 R), 0 -> 0: Fermat, x^(r - 2) by square-and-multiply from the top bit of the CONSTANT exponent — 253 squarings
// and 126 products, about 380 dependent fr_mul.  The one data-dependent branch is x == 0; which steps multiply is a property of r.  Not unrolled: the
// loop's body is two fr_mul.
HRX_HD Fr fr_inv(const Fr &x) {
    if (fr_is_zero(x)) return Fr{};
    Fr acc = x;                                                 // bit 253 of the exponent
HRX_FR_NOUNROLL
    for (int bit = 252; bit >= 0; --bit) {
        acc = fr_mul(acc, acc);
        uint32_t limb = 0;                                      // limb bit / 32 of the exponent, without a variable index into a constant array
HRX_FR_UNROLL
        for (int i = 0; i < 8; ++i) limb = (bit >> 5) == i ? kFrRm2_32[i] : limb;
        if ((limb >> (bit & 31)) & 1u) acc = fr_mul(acc, x);
    }
    return acc;
}

// x^(2^n): n squarings
HRX_HD Fr fr_square_n(Fr x, uint32_t n) {
HRX_FR_NOUNROLL
    for (uint32_t i = 0; i < n; ++i) x = fr_mul(x, x);
    return x;
}

// x^e for a Montgomery form x and a plain exponent below 2^32 (x^0 = one): square-and-multiply from the lowest bit; the loop ends with e's top bit.
HRX_HD Fr fr_pow_u32(const Fr &x, uint32_t e) {
    Fr sq = x, out = fr_R();
HRX_FR_NOUNROLL
    for (; e; e >>= 1) {
        if (e & 1u) out = fr_mul(out, sq);
        sq = fr_mul(sq, sq);
    }
    return out;
}

// ---- limb forms: the one place each rule lives -------------------------------------------------------------------------------------------------------
// A call's cells are Montgomery forms (x R, the default) or, where the call is `canonical` (HRX_FR_CANONICAL), the plain integers.  Multiplication runs on
// Montgomery forms either way; these take a value across.  include/hrx.h: cells read must be below r; only shift, beta, gamma and theta are reduced.

// the one of the call's form: R, or the plain 1
HRX_HD Fr fr_unit(bool canonical) { return fr_select(canonical, Fr{{1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}}, fr_R()); }
// a value in the call's form as the Montgomery form the products run on: itself, or x R where the call is canonical
HRX_HD Fr fr_to_mont(const Fr &x, bool canonical) { return canonical ? fr_mul(x, fr_R2()) : x; }
// a Montgomery form as the call's form: itself, or x R / R (a product by the plain 1) where the call is canonical
HRX_HD Fr fr_from_mont(const Fr &x, bool canonical) { return canonical ? fr_mul(x, fr_unit(true)) : x; }

// a cell: 4 u64 limbs, below r by contract — NOT reduced
HRX_HD Fr fr_load_cell(const uint64_t *cell) {
    Fr x;
HRX_FR_UNROLL
    for (int i = 0; i < 4; ++i) { x.w[2 * i] = (uint32_t)cell[i]; x.w[2 * i + 1] = (uint32_t)(cell[i] >> 32); }
    return x;
}
HRX_HD void fr_store_cell(uint64_t *cell, const Fr &x) {
HRX_FR_UNROLL
    for (int i = 0; i < 4; ++i) cell[i] = (uint64_t)x.w[2 * i] | (uint64_t)x.w[2 * i + 1] << 32;
}
// a challenge or shift (theta, beta, gamma, a run's shift, the NTT's g; the operands of hrx_fr_sub): 4 u64 limbs of ANY 256-bit value, taken mod r
HRX_HD Fr fr_challenge(const uint64_t *p) { return fr_reduce(fr_load_cell(p)); }

// ---- the fold of a lookup tuple with a challenge's powers ----------------------------------------------------------------------------------------------
// What a fold needs of one challenge theta: its powers and `one`, in the call's form — plain integers where the call is canonical (one = 1), otherwise
// Montgomery forms (one = R).  Two fr_mul (canonical: three).
struct FrPowers {
    Fr t1, t2, t3, one;
};
HRX_HD FrPowers fr_powers(const uint64_t *theta, bool canonical) {
    FrPowers p;
    p.t1 = fr_challenge(theta);
    if (canonical) {
        const Fr m = fr_to_mont(p.t1, true);       // theta R: a plain integer times it is the plain product
        p.t2 = fr_mul(p.t1, m);
        p.t3 = fr_mul(p.t2, m);
    } else {                                       // (a branch of its own: the square is cheaper than a product, and a workgroup of LOOKUP COMPRESS waits for it)
        p.t2 = fr_mul(p.t1, p.t1);
        p.t3 = fr_mul(p.t2, p.t1);
    }
    p.one = fr_unit(canonical);
    return p;
}

// a0 t3 + a1 t2 + a2 t1 + a3 one mod r for components a0 .. a3 below 2^16 and t3, t2, t1, one below r.
// With t_k = theta^k R mod r and one = R that is the Montgomery form of a0 theta^3 + a1 theta^2 + a2 theta + a3 — halo2's
// acc = acc * theta + e_i from 0 over (a0, a1, a2, a3); with t_k = theta^k mod r and one = 1 the plain integer.  A tuple of three components is (0, e0, e1, e2).
// Four small-scalar products, one sum S < 4 * 2^16 * r < 2^272 (nine limbs), one reduction: q' = floor(floor(S / 2^240) * K / 2^45) with
// K = floor(2^285 / r).  S / r - floor(S / 2^240) K / 2^45 < 2^240 / r + 2^32 / 2^45 < 2^-12, so q' underestimates q = floor(S / r) by at most 1 and
// S - q' r < 2 r < 2^255: the difference needs the low eight limbs only and at most ONE corrective subtraction.
HRX_HD Fr fr_fold(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, const FrPowers &p) {
    uint32_t s[9];
    uint64_t c = 0;
HRX_FR_UNROLL
    for (int i = 0; i < 8; ++i) {          // each product below 2^48, the four and the carry below 2^51
        c += (uint64_t)a0 * p.t3.w[i] + (uint64_t)a1 * p.t2.w[i] + (uint64_t)a2 * p.t1.w[i] + (uint64_t)a3 * p.one.w[i];
        s[i] = (uint32_t)c;
        c >>= 32;
    }
    s[8] = (uint32_t)c;
    const uint32_t top = s[7] >> 16 | s[8] << 16;              // floor(S / 2^240) < 2^32
    const uint32_t q = (uint32_t)(((uint64_t)top * kFrFoldK) >> 45);
    Fr out;
    uint64_t d = 0;
    uint32_t borrow = 0;
HRX_FR_UNROLL
    for (int i = 0; i < 8; ++i) {          // out = S - q r mod 2^256
        d += (uint64_t)q * kFrModulus32[i];
        const uint64_t x = (uint64_t)s[i] - (uint32_t)d - borrow;
        out.w[i] = (uint32_t)x;
        borrow = (uint32_t)(x >> 32) & 1u;
        d >>= 32;
    }
    fr_sub_if_ge<0>(out);
    return out;
}

}  // namespace hrx
