// test_ntt_host.cpp — csrc/hrx_fr.h (fr_sub, fr_pow_u32, the root of unity) + csrc/hrx_ntt.hpp + csrc/hrx_ntt_host.cpp as a program of their own
// (tests/test_ntt_cpu.py builds it with the address and undefined-behaviour sanitizers): the host twin at k = 1 .. 6 against the two sums of the rule
// written out over an arithmetic that shares nothing with hrx_fr.h — a schoolbook 256 x 256 product reduced by shift and subtract — in both directions and
// both limb forms, with and without a shift, n_in below 2^k, in place and out of place, pitches above 2^k; every buffer is a heap block of its exact
// size, so a read of an entry from n_in on or a write above 2^k that leaves the block is reported.  Prints "ntt host: ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_ntt_host.cpp"

using namespace hrx;

static int failures = 0;
#define CHECK(cond, ...)                                                                                    \
    do {                                                                                                    \
        if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (++failures > 20) exit(1); } \
    } while (0)

// ---- the independent arithmetic: 256-bit integers as 4 u64 limbs
struct U { uint64_t w[4]; };
static const U kR = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
static const U kOne = {{1, 0, 0, 0}};
static bool eq(const U &a, const U &b) { return !memcmp(a.w, b.w, 32); }
static int cmp(const U &a, const U &b) {
    for (int i = 3; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
static void sub_from(U &a, const U &b) {
    uint64_t borrow = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned __int128 x = (unsigned __int128)a.w[i] - b.w[i] - borrow;
        a.w[i] = (uint64_t)x;
        borrow = (uint64_t)(x >> 64) & 1u;
    }
}
static U addmod(U a, const U &b) {      // a, b < r < 2^254: no carry
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; ++i) { c += (unsigned __int128)a.w[i] + b.w[i]; a.w[i] = (uint64_t)c; c >>= 64; }
    if (cmp(a, kR) >= 0) sub_from(a, kR);
    return a;
}
static U submod(const U &a, const U &b) {
    U nb = kR;
    sub_from(nb, b);                    // r - b in (0, r]
    if (cmp(nb, kR) >= 0) sub_from(nb, kR);
    return addmod(a, nb);
}
static U mulmod(const U &a, const U &b) {
    uint64_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // schoolbook
    for (int i = 0; i < 4; ++i) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; ++j) { c += (unsigned __int128)a.w[i] * b.w[j] + p[i + j]; p[i + j] = (uint64_t)c; c >>= 64; }
        p[i + 4] = (uint64_t)c;
    }
    U rem = {{0, 0, 0, 0}};             // shift and subtract from the top bit: rem < r < 2^254, so 2 rem + 1 fits
    for (int bit = 511; bit >= 0; --bit) {
        for (int i = 3; i > 0; --i) rem.w[i] = rem.w[i] << 1 | rem.w[i - 1] >> 63;
        rem.w[0] = rem.w[0] << 1 | ((p[bit / 64] >> (bit % 64)) & 1u);
        if (cmp(rem, kR) >= 0) sub_from(rem, kR);
    }
    return rem;
}
static U powmod(U b, uint64_t e) {
    U acc = kOne;
    for (; e; e >>= 1) {
        if (e & 1u) acc = mulmod(acc, b);
        b = mulmod(b, b);
    }
    return acc;
}
static const U kMont = {{0xac96341c4ffffffbull, 0x36fc76959f60cd29ull, 0x666ea36f7879462eull, 0x0e0a77c19a07df2full}};      // 2^256 mod r
static const U kHalf = {{0xa1f0fac9f8000001ull, 0x9419f4243cdcb848ull, 0xdc2822db40c0ac2eull, 0x183227397098d014ull}};      // (r + 1) / 2

static U random_element(std::mt19937_64 &rng) {
    U a = {{rng(), rng(), rng(), rng() >> 3}};
    while (cmp(a, kR) >= 0) sub_from(a, kR);
    return a;
}
static U cell_of(const U &v, bool canonical) { return canonical ? v : mulmod(v, kMont); }

// the root of unity from the generator: 7^((r - 1) / 2^28) by repeated multiplication of the independent arithmetic
static U root_of_unity() {
    U e = kR;                            // (r - 1) >> 28, as limbs
    e.w[0] -= 1;
    for (int s = 0; s < 28; ++s)
        for (int i = 0; i < 4; ++i) e.w[i] = e.w[i] >> 1 | (i < 3 ? e.w[i + 1] : 0) << 63;
    U acc = kOne, b = {{7, 0, 0, 0}};
    for (int bit = 0; bit < 256; ++bit) {
        if ((e.w[bit / 64] >> (bit % 64)) & 1u) acc = mulmod(acc, b);
        b = mulmod(b, b);
    }
    return acc;
}

static void run_case(unsigned k, bool inverse, bool canonical, bool shifted, size_t n_in, size_t n_cols, size_t extra_pitch, bool in_place, const U &root,
                     std::mt19937_64 &rng) {
    const size_t n = (size_t)1 << k, out_pitch = ((n + 3) & ~(size_t)3) + extra_pitch, in_pitch = in_place ? out_pitch : (n_in + 3) & ~(size_t)3;
    U w = root;
    for (unsigned s = k; s < 28; ++s) w = mulmod(w, w);
    const U g = shifted ? random_element(rng) : kOne;
    U ninv = kOne;
    for (unsigned s = 0; s < k; ++s) ninv = mulmod(ninv, kHalf);
    // the input: exactly the cells the call may read — the last column's block ends at its n_in-th cell
    const size_t in_cells = (n_cols - 1) * in_pitch + (in_place ? n : n_in), out_cells = (n_cols - 1) * out_pitch + n;
    uint64_t *in = (uint64_t *)malloc(in_cells * 32), *out = in_place ? in : (uint64_t *)malloc(out_cells * 32);
    memset(in, 0x5a, in_cells * 32);
    if (!in_place) memset(out, 0x5a, out_cells * 32);
    std::vector<std::vector<U>> x(n_cols, std::vector<U>(n, U{{0, 0, 0, 0}}));
    for (size_t c = 0; c < n_cols; ++c)
        for (size_t i = 0; i < n_in; ++i) {
            x[c][i] = i == 0 ? U{{0, 0, 0, 0}} : i == 1 ? kOne : i == 2 ? submod(U{{0, 0, 0, 0}}, kOne) : random_element(rng);
            const U cell = cell_of(x[c][i], canonical);
            memcpy(in + (c * in_pitch + i) * 4, cell.w, 32);
        }
    uint64_t *shift = nullptr;
    if (shifted) {
        shift = (uint64_t *)malloc(32);
        const U cell = cell_of(g, canonical);
        memcpy(shift, cell.w, 32);
    }
    NttArgs a = {};
    a.in = in; a.out = out; a.in_pitch = in_pitch; a.out_pitch = out_pitch; a.n_cols = (uint32_t)n_cols; a.k = k; a.n_in = (uint32_t)n_in;
    a.inverse = inverse; a.canonical = canonical; a.shift = shift;
    ntt_host(a, 2);
    std::vector<U> wpow(n, kOne), gpow(n, kOne);       // the powers of w (of its inverse: w^(n - 1)) and of g
    const U wd = inverse ? powmod(w, n - 1) : w;
    for (size_t t = 1; t < n; ++t) { wpow[t] = mulmod(wpow[t - 1], wd); gpow[t] = mulmod(gpow[t - 1], g); }
    for (size_t c = 0; c < n_cols; ++c) {
        for (size_t j = 0; j < n; ++j) {
            U acc = {{0, 0, 0, 0}};
            for (size_t i = 0; i < n_in; ++i) acc = addmod(acc, mulmod(inverse ? x[c][i] : mulmod(x[c][i], gpow[i]), wpow[(i * j) % n]));
            if (inverse) acc = mulmod(mulmod(acc, ninv), gpow[j]);
            const U want = cell_of(acc, canonical);
            U got;
            memcpy(got.w, out + (c * out_pitch + j) * 4, 32);
            CHECK(eq(got, want), "k %u inverse %d canonical %d shifted %d n_in %zu column %zu entry %zu", k, (int)inverse, (int)canonical, (int)shifted, n_in, c, j);
        }
        if (c + 1 < n_cols)
            for (size_t j = n; j < out_pitch; ++j)
                for (int l = 0; l < 4; ++l) CHECK(out[(c * out_pitch + j) * 4 + l] == 0x5a5a5a5a5a5a5a5aull, "entry %zu above 2^k was written", j);
    }
    free(in);
    if (!in_place) free(out);
    free(shift);
}

int main() {
    std::mt19937_64 rng(20231);
    const U root = root_of_unity();
    {   // the constants of hrx_fr.h against the independent arithmetic
        U c;
        memcpy(c.w, kFrRootOfUnity, 32);
        CHECK(eq(c, root), "kFrRootOfUnity is not 7^((r - 1) / 2^28)");
        U m = mulmod(root, kMont), got;
        fr_store_cell(got.w, fr_root_of_unity());
        CHECK(eq(got, m), "kFrRootOfUnity32 is not its Montgomery form");
        fr_store_cell(got.w, fr_half());
        CHECK(eq(got, mulmod(kHalf, kMont)), "kFrInv2_32 is not the Montgomery form of 1 / 2");
        CHECK(eq(addmod(kHalf, kHalf), kOne), "(r + 1) / 2");
        CHECK(eq(powmod(root, 1ull << 28), kOne) && !eq(powmod(root, 1ull << 27), kOne), "the root's order is not 2^28");
    }
    for (int t = 0; t < 2000; ++t) {     // fr_sub
        const U a = t == 0 ? U{{0, 0, 0, 0}} : random_element(rng), b = t == 1 ? a : t == 2 ? submod(U{{0, 0, 0, 0}}, kOne) : random_element(rng);
        U got;
        fr_store_cell(got.w, fr_sub(fr_load_cell(a.w), fr_load_cell(b.w)));
        CHECK(eq(got, submod(a, b)), "fr_sub, sample %d", t);
    }
    for (unsigned k = 1; k <= 6; ++k) {
        const size_t n = (size_t)1 << k;
        for (int inverse = 0; inverse < 2; ++inverse)
            for (int canonical = 0; canonical < 2; ++canonical)
                for (int shifted = 0; shifted < 2; ++shifted) {
                    run_case(k, inverse, canonical, shifted, n, 3, 0, false, root, rng);
                    run_case(k, inverse, canonical, shifted, n, 2, 4, true, root, rng);
                    run_case(k, inverse, canonical, shifted, n - 1, 2, 8, false, root, rng);
                    run_case(k, inverse, canonical, shifted, 1, 1, 0, false, root, rng);
                    if (k >= 2) run_case(k, inverse, canonical, shifted, n >> 2, 5, 0, false, root, rng);
                    if (k >= 2) run_case(k, inverse, canonical, shifted, n >> 2, 2, 0, true, root, rng);
                }
    }
    if (failures) return 1;
    printf("ntt host: ok\n");
    return 0;
}
