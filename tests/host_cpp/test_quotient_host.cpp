// test_quotient_host.cpp — csrc/hrx_fr.h + csrc/hrx_quotient.hpp + csrc/hrx_quotient_host.cpp as a program of their own (tests/test_quotient_cpu.py builds it
// with the address and undefined-behaviour sanitizers): the host twin at k = 1 .. 4, e = 1 .. 3 against the five steps of the rule written out, in halo2's
// order and without regrouping, over an arithmetic that shares nothing with hrx_fr.h — a schoolbook 256 x 256 product reduced by shift and subtract — in
// both limb forms, with h_in absent, apart and in place, one table run and one per string, challenges per call and per string, with and without the
// division, and the vanishing inverse against Fermat's power; every buffer is a heap block of its exact size, so a read or a write past the last column's
// 2^ext_k-th cell is reported.  Prints "quotient host: ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_quotient_host.cpp"

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


// a heap block of exactly `cells` cells holding `vals` at the given pitch (the last column ends at its N-th cell), poison between
static uint64_t *block(const std::vector<std::vector<U>> &vals, size_t pitch, size_t N, bool canonical) {
    const size_t cells = (vals.size() - 1) * pitch + N;
    uint64_t *p = (uint64_t *)malloc(cells * 32);
    memset(p, 0x5a, cells * 32);
    for (size_t c = 0; c < vals.size(); ++c)
        for (size_t j = 0; j < N; ++j) {
            const U cell = cell_of(vals[c][j], canonical);
            memcpy(p + (c * pitch + j) * 4, cell.w, 32);
        }
    return p;
}
static std::vector<std::vector<U>> random_columns(size_t count, size_t N, std::mt19937_64 &rng) {
    std::vector<std::vector<U>> v(count, std::vector<U>(N));
    for (size_t c = 0; c < count; ++c)
        for (size_t j = 0; j < N; ++j) {
            const size_t e = (j + c) % N;
            v[c][j] = e == 0 ? U{{0, 0, 0, 0}} : e == 1 ? kOne : e == 2 ? submod(U{{0, 0, 0, 0}}, kOne) : random_element(rng);
        }
    return v;
}

static void run_case(unsigned k, unsigned e, uint32_t ncols, uint32_t b_count, bool canonical, bool per_string, bool s_per_string, int h_mode, bool divide,
                     const U &root, std::mt19937_64 &rng) {
    const unsigned ext_k = k + e;
    const size_t N = (size_t)1 << ext_k, n = (size_t)1 << k, rot = (size_t)1 << e, pitch = N + 4, s_pitch = N + 8, sel_pitch = N, h_pitch = N + 12;
    const size_t runs = s_per_string ? b_count : 1, n_ch = per_string ? b_count : 1;
    const auto A = random_columns(ncols * b_count, N, rng), Ap = random_columns(ncols * b_count, N, rng), Sp = random_columns(ncols * b_count, N, rng),
               Z = random_columns(ncols * b_count, N, rng), S = random_columns(ncols * runs, N, rng), sel = random_columns(3, N, rng),
               H = random_columns(b_count, N, rng);
    std::vector<U> beta(n_ch), gamma(n_ch), y(n_ch);
    uint64_t *pb = (uint64_t *)malloc(n_ch * 32), *pg = (uint64_t *)malloc(n_ch * 32), *py = (uint64_t *)malloc(n_ch * 32);
    for (size_t i = 0; i < n_ch; ++i) {
        beta[i] = random_element(rng); gamma[i] = random_element(rng); y[i] = random_element(rng);
        const U cb = cell_of(beta[i], canonical), cg = cell_of(gamma[i], canonical), cy = cell_of(y[i], canonical);
        memcpy(pb + 4 * i, cb.w, 32); memcpy(pg + 4 * i, cg.w, 32); memcpy(py + 4 * i, cy.w, 32);
    }
    // the vanishing inverse: the library's table against Fermat's power in the independent arithmetic
    const U g = random_element(rng);
    U w = root;
    for (unsigned s = ext_k; s < 28; ++s) w = mulmod(w, w);
    uint64_t *pshift = (uint64_t *)malloc(32), *pt = (uint64_t *)malloc(rot * 32);
    { const U c = cell_of(g, canonical); memcpy(pshift, c.w, 32); }
    vanishing_inverse_host(VanishArgs{pshift, pt, k, ext_k, canonical ? 1u : 0u});
    std::vector<U> t(rot);
    for (size_t c = 0; c < rot && (divide || h_mode == 0); ++c) {      // (Fermat's power over the shift-and-subtract product is the slow part: where it is used, and in a third of the others)
        const U d = submod(mulmod(powmod(g, n), powmod(w, n * c)), kOne);
        U e2 = kR, inv = kOne, b = d;                // d^(r - 2)
        e2.w[0] -= 2;
        for (int bit = 0; bit < 256; ++bit) {
            if ((e2.w[bit / 64] >> (bit % 64)) & 1u) inv = mulmod(inv, b);
            b = mulmod(b, b);
        }
        t[c] = inv;
        U got;
        memcpy(got.w, pt + 4 * c, 32);
        CHECK(eq(got, cell_of(inv, canonical)) && eq(mulmod(inv, d), kOne), "vanishing inverse k %u e %u entry %zu", k, e, c);
    }
    uint64_t *pa = block(A, pitch, N, canonical), *pap = block(Ap, pitch, N, canonical), *psp = block(Sp, pitch, N, canonical), *pz = block(Z, pitch, N, canonical),
             *ps = block(S, s_pitch, N, canonical), *psel = block(sel, sel_pitch, N, canonical), *ph = h_mode ? block(H, h_pitch, N, canonical) : nullptr;
    const size_t h_cells = (b_count - 1) * h_pitch + N;
    uint64_t *pout = h_mode == 2 ? ph : (uint64_t *)malloc(h_cells * 32);
    if (h_mode != 2) memset(pout, 0x5a, h_cells * 32);
    QuotientArgs a = {};
    a.a_ext = pa; a.ap_ext = pap; a.sp_ext = psp; a.z_ext = pz; a.s_ext = ps; a.selectors = psel; a.beta = pb; a.gamma = pg; a.y = py; a.h_in = ph; a.h_out = pout;
    a.t_inv = divide ? pt : nullptr; a.pitch = pitch; a.s_pitch = s_pitch; a.sel_pitch = sel_pitch; a.h_pitch = h_pitch; a.b_count = b_count; a.ncols = ncols;
    a.k = k; a.ext_k = ext_k; a.s_stride = s_per_string; a.challenge_stride = per_string ? 4u : 0u; a.canonical = canonical; a.divide = divide;
    quotient_host(a, 2);
    for (size_t b = 0; b < b_count; ++b) {
        const U be = beta[per_string ? b : 0], ga = gamma[per_string ? b : 0], yy = y[per_string ? b : 0];
        for (size_t j = 0; j < N; ++j) {
            const size_t jn = (j + rot) % N, jp = (j + N - rot) % N;
            U v = h_mode ? H[b][j] : U{{0, 0, 0, 0}};
            for (size_t c = 0; c < ncols; ++c) {
                const size_t i = c * b_count + b, si = c * runs + (s_per_string ? b : 0);
                const U z = Z[i][j], d = submod(Ap[i][j], Sp[i][j]);
                v = addmod(mulmod(v, yy), mulmod(submod(kOne, z), sel[0][j]));
                v = addmod(mulmod(v, yy), mulmod(submod(mulmod(z, z), z), sel[1][j]));
                const U left = mulmod(mulmod(Z[i][jn], addmod(Ap[i][j], be)), addmod(Sp[i][j], ga));
                const U right = mulmod(mulmod(z, addmod(A[i][j], be)), addmod(S[si][j], ga));
                v = addmod(mulmod(v, yy), mulmod(submod(left, right), sel[2][j]));
                v = addmod(mulmod(v, yy), mulmod(d, sel[0][j]));
                v = addmod(mulmod(v, yy), mulmod(mulmod(d, submod(Ap[i][j], Ap[i][jp])), sel[2][j]));
            }
            if (divide) v = mulmod(v, t[j % rot]);
            U got;
            memcpy(got.w, pout + (b * h_pitch + j) * 4, 32);
            CHECK(eq(got, cell_of(v, canonical)), "k %u e %u lookups %u canonical %d h_mode %d divide %d string %zu point %zu", k, e, ncols, (int)canonical, h_mode,
                  (int)divide, b, j);
        }
        if (b + 1 < b_count && h_mode != 2)
            for (size_t j = N; j < h_pitch; ++j)
                for (int l = 0; l < 4; ++l) CHECK(pout[(b * h_pitch + j) * 4 + l] == 0x5a5a5a5a5a5a5a5aull, "entry %zu above 2^ext_k was written", j);
    }
    free(pa); free(pap); free(psp); free(pz); free(ps); free(psel); free(ph); free(pb); free(pg); free(py); free(pshift); free(pt);
    if (h_mode != 2) free(pout);
}

int main() {
    std::mt19937_64 rng(20241);
    const U root = root_of_unity();
    {   // the constants LOOKUP QUOTIENT added to hrx_fr.h
        U got;
        fr_store_cell(got.w, fr_R3());
        CHECK(eq(got, mulmod(mulmod(kMont, kMont), kMont)), "kFrR3_32 is not R^3");
        fr_store_cell(got.w, fr_R4());
        CHECK(eq(got, mulmod(mulmod(kMont, kMont), mulmod(kMont, kMont))), "kFrR4_32 is not R^4");
    }
    int t = 0;
    for (unsigned k = 1; k <= 4; ++k)
        for (unsigned e = 1; e <= 3; ++e)
            for (int canonical = 0; canonical < 2; ++canonical)
                for (int h_mode = 0; h_mode < 3; ++h_mode, ++t) {
                    run_case(k, e, 3, 1 + 2 * (t & 1), canonical, (t >> 1) & 1, (t >> 2) & 1, h_mode, (t >> 3) & 1, root, rng);
                    if (e == 2) run_case(k, e, 6, 2, canonical, !((t >> 1) & 1), !((t >> 2) & 1), h_mode, !((t >> 3) & 1), root, rng);
                }
    if (failures) return 1;
    printf("quotient host: ok\n");
    return 0;
}
