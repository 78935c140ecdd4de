// test_product_host.cpp — csrc/hrx_product.hpp + csrc/hrx_product_host.cpp (and hrx_fr.h's fr_inv) as a program of their own (tests/test_product_cpu.py builds
// it with the address and undefined-behaviour sanitizers): the host twins against the rule of the header written out over an arithmetic that shares nothing
// with hrx_fr.h — a schoolbook 256 x 256 product reduced by shift and subtract, and an inversion by the binary extended Euclid — in both limb forms; tables,
// inputs, index columns and every output are heap blocks of their exact size, so a read or write one element outside is reported.  Prints "product host: ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_product_host.cpp"

using namespace hrx;

static int failures = 0;
#define CHECK(cond, ...)                                                                                    \
    do {                                                                                                    \
        if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (++failures > 20) exit(1); } \
    } while (0)

// ---- the independent arithmetic: 256-bit integers as 4 u64 limbs
struct U { uint64_t w[4]; };
static const U kR = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
static bool is_zero(const U &a) { return !(a.w[0] | a.w[1] | a.w[2] | a.w[3]); }
static bool eq(const U &a, const U &b) { return !memcmp(a.w, b.w, 32); }
static int cmp(const U &a, const U &b) {
    for (int i = 3; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
static uint64_t add_to(U &a, const U &b) {
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; ++i) { c += (unsigned __int128)a.w[i] + b.w[i]; a.w[i] = (uint64_t)c; c >>= 64; }
    return (uint64_t)c;
}
static void sub_from(U &a, const U &b) {
    uint64_t borrow = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned __int128 x = (unsigned __int128)a.w[i] - b.w[i] - borrow;
        a.w[i] = (uint64_t)x;
        borrow = (uint64_t)(x >> 64) & 1u;
    }
}
static void shr1(U &a, uint64_t top = 0) {
    for (int i = 0; i < 4; ++i) a.w[i] = a.w[i] >> 1 | (i < 3 ? a.w[i + 1] : top) << 63;
}
static U addmod(U a, const U &b) {      // a, b < r < 2^254: no carry
    add_to(a, b);
    if (cmp(a, kR) >= 0) sub_from(a, kR);
    return a;
}
static U reduce(U a) {                  // any 256-bit value
    while (cmp(a, kR) >= 0) sub_from(a, kR);
    return a;
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
// a^-1 mod r for 0 < a < r by the binary extended Euclid (r odd): u x1 = a (mod r) and v x2 = a (mod r) ... kept as x1 a^-1-multiples; returns x with a x = 1
static U invmod(const U &a) {
    U u = a, v = kR, x1 = {{1, 0, 0, 0}}, x2 = {{0, 0, 0, 0}};
    const U one = {{1, 0, 0, 0}};
    auto halve = [](U &x) {             // x / 2 mod r
        if (x.w[0] & 1u) { const uint64_t c = add_to(x, kR); shr1(x, c); }
        else shr1(x);
    };
    while (!eq(u, one) && !eq(v, one)) {
        while (!(u.w[0] & 1u)) { shr1(u); halve(x1); }
        while (!(v.w[0] & 1u)) { shr1(v); halve(x2); }
        if (cmp(u, v) >= 0) { sub_from(u, v); if (cmp(x1, x2) < 0) add_to(x1, kR); sub_from(x1, x2); }
        else { sub_from(v, u); if (cmp(x2, x1) < 0) add_to(x2, kR); sub_from(x2, x1); }
    }
    return reduce(eq(u, one) ? x1 : x2);
}

static U kMont, kMontInv;               // 2^256 mod r and its inverse (the inverse: checked in main, not used by the cases)
static U cell_of(const U &v, bool canonical) { return canonical ? v : mulmod(v, kMont); }

struct Heap {          // a block of exactly n elements
    template <class X> static X *make(size_t n, X fill) { X *p = (X *)malloc(n ? n * sizeof(X) : 1); for (size_t i = 0; i < n; ++i) p[i] = fill; return p; }
};
static std::mt19937_64 rng(20240607);
static U random_element() {
    U x = {{rng(), rng(), rng(), rng() >> 2}};
    return reduce(x);
}
static const uint64_t kPoison = 0x5A5A5A5A5A5A5A5Aull;

static void run_case(bool canonical, bool per_string, unsigned threads) {
    const std::vector<uint32_t> Ts = {7, 3, 3, 5, 2, 2};                // two defs
    const uint32_t M = 5, n_rows = 9, idx_pitch = 12, z_pitch = 12, b_count = 4, b_begin = 1;
    const uint32_t lens_of[5] = {99, 2, 5, 6, 0};                       // of the batch; the window: n < M, n == M, n > M, n == 0
    ProductArgs a{};
    uint32_t bins = 0;
    for (size_t c = 0; c < Ts.size(); ++c) { a.col[c] = PermuteCol{bins, Ts[c]}; bins += Ts[c]; }
    const uint32_t W = (bins + 3u) & ~3u, ncols = (uint32_t)Ts.size(), runs = per_string ? b_count : 1;
    CHECK(W > bins, "the case wants pad words");
    uint32_t *lens = Heap::make<uint32_t>(5, 0u);
    memcpy(lens, lens_of, sizeof lens_of);
    uint64_t *table = Heap::make<uint64_t>((size_t)runs * W * 4, 0ull), *inv_b = Heap::make<uint64_t>((size_t)runs * W * 4, kPoison),
             *inv_g = Heap::make<uint64_t>((size_t)runs * W * 4, kPoison), *chal = Heap::make<uint64_t>((size_t)2 * runs * 4, 0ull);
    uint64_t *in = Heap::make<uint64_t>((size_t)ncols * b_count * M * 4, 0ull), *z = Heap::make<uint64_t>((size_t)ncols * b_count * z_pitch * 4, kPoison);
    uint32_t *ai = Heap::make<uint32_t>((size_t)ncols * b_count * idx_pitch, 0u), *si = Heap::make<uint32_t>((size_t)ncols * b_count * idx_pitch, 0u);
    uint32_t *open = Heap::make<uint32_t>(b_count, 0x5A5A5A5Au);
    std::vector<U> S((size_t)runs * W), beta(runs), gamma(runs);
    for (uint32_t r = 0; r < runs; ++r) {
        for (uint32_t w = 0; w < bins; ++w) {
            S[(size_t)r * W + w] = random_element();
            const U c = cell_of(S[(size_t)r * W + w], canonical);
            memcpy(table + ((size_t)r * W + w) * 4, c.w, 32);
        }
        beta[r] = random_element();
        gamma[r] = random_element();
        if (r == 0) { gamma[0] = kR; sub_from(gamma[0], S[3]); }                                // gamma = -S[3] of run 0: a zero denominator
        U bl = cell_of(beta[r], canonical), gl = cell_of(gamma[r], canonical);
        if (r == 0) add_to(bl, kR);                                                             // limbs of beta + r: taken mod r first
        memcpy(chal + (size_t)r * 4, bl.w, 32);
        memcpy(chal + ((size_t)runs + r) * 4, gl.w, 32);
    }
    std::vector<U> A((size_t)ncols * b_count * M);
    for (size_t k = 0; k < A.size(); ++k) {
        A[k] = random_element();
        const U c = cell_of(A[k], canonical);
        memcpy(in + k * 4, c.w, 32);
    }
    for (uint32_t c = 0; c < ncols; ++c)
        for (uint32_t b = 0; b < b_count; ++b)
            for (uint32_t i = 0; i < idx_pitch; ++i) {
                const size_t k = ((size_t)c * b_count + b) * idx_pitch + i;
                ai[k] = a.col[c].off + (uint32_t)(rng() % Ts[c]);
                si[k] = a.col[c].off + (uint32_t)(rng() % Ts[c]);
                if (i >= n_rows) ai[k] = si[k] = 0x5A5A5A5Au;                                   // the pitch tail: never read as an address
            }
    ai[((size_t)1 * b_count + 0) * idx_pitch + 4] = 0xffffffffu;                                // permute's overflow pattern
    si[((size_t)3 * b_count + 2) * idx_pitch + 0] = a.col[3].off + Ts[3];                       // one behind the lookup's range
    si[((size_t)4 * b_count + 1) * idx_pitch + 8] = a.col[4].off - 1u;                          // one before it
    InvertArgs ia{};
    ia.table = table; ia.n_runs = runs; ia.W = W; ia.bins = bins; ia.canonical = canonical; ia.shift_stride = per_string ? 4u : 0u;
    ia.shift = chal; ia.inv = inv_b;
    invert_table_host(ia, threads);
    ia.shift = chal + (size_t)runs * 4; ia.inv = inv_g;
    invert_table_host(ia, threads);
    for (uint32_t r = 0; r < runs; ++r)
        for (uint32_t w = 0; w < W; ++w)
            for (int which = 0; which < 2; ++which) {
                const uint64_t *cell = (which ? inv_g : inv_b) + ((size_t)r * W + w) * 4;
                U want = {{0, 0, 0, 0}};
                if (w < bins) {
                    const U s = addmod(S[(size_t)r * W + w], which ? gamma[r] : beta[r]);
                    if (!is_zero(s)) want = invmod(s);
                    else CHECK(which == 1 && r == 0 && w == 3, "an unplanned zero");
                }
                const U cw = cell_of(want, canonical);
                CHECK(!memcmp(cell, cw.w, 32), "inverse table: run %u word %u table %d canonical %d", r, w, which, (int)canonical);
            }
    a.lens = lens; a.M = M; a.b_begin = b_begin; a.b_count = b_count; a.n_rows = n_rows; a.idx_pitch = idx_pitch; a.z_pitch = z_pitch; a.W = W; a.ncols = ncols;
    a.canonical = canonical; a.in_cells = in; a.a_idx = ai; a.s_idx = si; a.table = table; a.inv_beta = inv_b; a.inv_gamma = inv_g;
    a.table_stride = per_string ? 4u * W : 0u; a.beta = chal; a.gamma = chal + (size_t)runs * 4; a.challenge_stride = per_string ? 4u : 0u; a.z = z; a.open = open;
    product_host(a, threads);
    const U one = {{1, 0, 0, 0}};
    for (uint32_t b = 0; b < b_count; ++b) {
        const uint32_t r = per_string ? b : 0u, n = lens_of[b_begin + b];
        uint32_t want_open = 0;
        for (uint32_t c = 0; c < ncols; ++c) {
            const uint32_t off = a.col[c].off, T = Ts[c], k = c % 3u;
            const U *Sr = S.data() + (size_t)r * W;
            U Z = one;
            const uint64_t *zc = z + ((size_t)c * b_count + b) * z_pitch * 4;
            for (uint32_t i = 0; i <= n_rows; ++i) {
                const U cw = cell_of(Z, canonical);
                CHECK(!memcmp(zc + (size_t)i * 4, cw.w, 32), "Z: string %u lookup %u entry %u canonical %d per_string %d", b, c, i, (int)canonical, (int)per_string);
                if (i == n_rows) break;
                const uint32_t x = ai[((size_t)c * b_count + b) * idx_pitch + i], y = si[((size_t)c * b_count + b) * idx_pitch + i];
                U term = {{0, 0, 0, 0}};
                if (x >= off && x < off + T && y >= off && y < off + T) {
                    const bool dummy = i >= M || n > M || (n == M && i == M - 1 && (k == 0 || k == 2));
                    const U Ai = dummy ? Sr[off] : A[((size_t)c * b_count + b) * M + i], Si = i < T ? Sr[off + i] : Sr[off];
                    const U db = addmod(Sr[x], beta[r]), dg = addmod(Sr[y], gamma[r]);
                    term = mulmod(addmod(Ai, beta[r]), addmod(Si, gamma[r]));
                    term = mulmod(term, is_zero(db) ? db : invmod(db));
                    term = mulmod(term, is_zero(dg) ? dg : invmod(dg));
                }
                Z = mulmod(Z, term);
            }
            if (!eq(Z, one)) want_open |= 1u << c;
            for (uint32_t i = (n_rows + 1) * 4; i < z_pitch * 4; ++i) CHECK(zc[i] == kPoison, "an entry above n_rows was written");
        }
        CHECK(open[b] == want_open, "open: string %u: %x, want %x", b, open[b], want_open);
    }
    free(lens); free(table); free(inv_b); free(inv_g); free(chal); free(in); free(z); free(ai); free(si); free(open);
}

int main() {
    kMont = U{{0xac96341c4ffffffbull, 0x36fc76959f60cd29ull, 0x666ea36f7879462eull, 0x0e0a77c19a07df2full}};
    {   // 2^256 mod r, by doubling 1
        U x = {{1, 0, 0, 0}};
        for (int i = 0; i < 256; ++i) x = addmod(x, x);
        CHECK(eq(x, kMont), "2^256 mod r");
    }
    kMontInv = invmod(kMont);
    const U one = {{1, 0, 0, 0}};
    CHECK(eq(mulmod(kMont, kMontInv), one), "invmod");
    for (int k = 0; k < 50; ++k) {      // fr_inv against the Euclid inverse, Montgomery form in and out
        const U v = k == 0 ? one : k == 1 ? U{{kR.w[0] - 1, kR.w[1], kR.w[2], kR.w[3]}} : random_element();
        const U c = cell_of(v, false);
        uint64_t out[4];
        fr_store_cell(out, fr_inv(fr_load_cell(c.w)));
        const U want = cell_of(invmod(v), false);
        CHECK(!memcmp(out, want.w, 32), "fr_inv, sample %d", k);
    }
    CHECK(fr_is_zero(fr_inv(Fr{})), "fr_inv(0) = 0");
    for (int canonical = 0; canonical < 2; ++canonical)
        for (int per_string = 0; per_string < 2; ++per_string)
            for (unsigned threads : {1u, 3u}) run_case(canonical != 0, per_string != 0, threads);
    if (failures) { printf("product host: %d failures\n", failures); return 1; }
    printf("product host: ok\n");
    return 0;
}
