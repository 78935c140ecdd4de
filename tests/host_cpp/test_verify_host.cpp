// test_verify_host.cpp — csrc/hrx_verify.hpp and csrc/hrx_verify_host.cpp (the rules and the host form of VERIFY, include/hrx.h) as a program of their own,
// built with -fsanitize=address,undefined by tests/test_verify_cpu.py.  Every array is a heap block of exactly its size, so one element too far is a sanitizer
// error.  The rows are hand-made: three small DFAs over {a, b} whose table rows are written out below, a walk of them in the words of src/lib.rs (states,
// substr ids, start / end flags, padding), and the masked rows from the two "last event wins" scans of lib.rs:593-764 as arrays, forward and backward — not
// from the one-pass rule under test.  Checked: clean rows give 0 (or exactly the accept chain at row n), every tampered cell its check and its row, values
// outside every table (in one to five defs, with the image a heap block of exactly its size) the check that pins them and no read outside the image, the
// string-major, pitched and position-major images of the same rows the same words, and the kernel's tile loop (verify_lane, every instantiation the
// kernel uses) the same words as the row-by-row loop.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_verify_host.cpp"

using namespace hrx;

static int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #c);               \
            ++failures;                                               \
        }                                                             \
    } while (0)

// A hand-made def: DFA transitions (cur, char, next), one optional substring definition (id, tagged (cur, next) pairs, start states, end states)
struct Def {
    uint64_t first, accepted, largest;
    std::vector<std::vector<uint64_t>> trans;      // {cur, char, next}
    uint64_t sid;                                   // 0: no substring definition
    std::vector<std::pair<uint64_t, uint64_t>> tagged;
    std::vector<uint64_t> starts, ends;
    uint64_t dummy() const { return largest + 1; }
    bool is_tagged(uint64_t c, uint64_t n) const {
        for (auto &p : tagged)
            if (p.first == c && p.second == n) return true;
        return false;
    }
    static bool in(const std::vector<uint64_t> &v, uint64_t x) {
        for (uint64_t y : v)
            if (y == x) return true;
        return false;
    }
    // the rows RegexTableConfig::load assigns (table.rs:68-196)
    std::vector<uint64_t> transition_rows() const {
        std::vector<uint64_t> r = {0, dummy(), dummy(), 0};
        for (auto &t : trans) { r.push_back(t[1]); r.push_back(t[0]); r.push_back(t[2]); r.push_back(is_tagged(t[0], t[2]) ? sid : 0); }
        return r;
    }
    std::vector<uint64_t> endpoint_rows() const {
        std::vector<uint64_t> r = {0, dummy(), dummy()};
        if (sid) {
            for (uint64_t s : starts) { r.push_back(sid); r.push_back(s); r.push_back(dummy()); }
            for (uint64_t e : ends) { r.push_back(sid); r.push_back(dummy()); r.push_back(e); }
        }
        return r;
    }
};

// a* b+ a*: substring 1 = the run of b (several end flags in a row); accepted once an a follows the run
static const Def kDef1 = {0, 2, 2, {{0, 'a', 0}, {0, 'b', 1}, {1, 'b', 1}, {1, 'a', 2}, {2, 'a', 2}}, 1, {{0, 1}, {1, 1}}, {0}, {1}};
// anything: substring 2 = the first a; accepted once there was an a
static const Def kDef2 = {0, 1, 1, {{0, 'b', 0}, {0, 'a', 1}, {1, 'a', 1}, {1, 'b', 1}}, 2, {{0, 1}}, {0}, {1}};
// the same DFA without a substring definition
static const Def kDef3 = {0, 1, 1, {{0, 'b', 0}, {0, 'a', 1}, {1, 'a', 1}, {1, 'b', 1}}, 0, {}, {}, {}};

struct Rows {      // one string's rows, string-major
    uint32_t n, M, D;
    std::vector<uint8_t> chars;          // [n]
    std::vector<uint32_t> rec;           // [M][D]
    std::vector<uint16_t> msk;           // [M]
    bool accepted_all;
};

// match_substrs in plain words (lib.rs:387-519, 593-764) for a string every def has transitions for
static Rows make_rows(const std::vector<Def> &defs, const std::string &s, uint32_t M) {
    Rows R;
    R.n = (uint32_t)s.size(); R.M = M; R.D = (uint32_t)defs.size();
    R.chars.assign(s.begin(), s.end());
    R.rec.assign((size_t)M * R.D, 0);
    R.msk.assign(M, 0);
    R.accepted_all = true;
    const uint32_t n = R.n, D = R.D;
    std::vector<uint32_t> SID(M + 1, 0), ST(M + 1, 0), EN(M + 1, 0);
    for (uint32_t d = 0; d < D; ++d) {
        const Def &F = defs[d];
        std::vector<uint64_t> st(n + 1);
        st[0] = F.first;
        for (uint32_t i = 0; i < n; ++i) {
            bool found = false;
            for (auto &t : F.trans)
                if (t[0] == st[i] && t[1] == (uint8_t)s[i]) { st[i + 1] = t[2]; found = true; }
            if (!found) { std::printf("make_rows: no transition\n"); std::exit(2); }
        }
        if (st[n] != F.accepted) R.accepted_all = false;
        for (uint32_t r = 0; r < M; ++r) {
            uint32_t x;
            if (r < n) {
                const uint32_t sid = F.sid && F.is_tagged(st[r], st[r + 1]) ? (uint32_t)F.sid : 0;
                const uint32_t se = sid && Def::in(F.starts, st[r]), ee = r + 1 < M && sid && Def::in(F.ends, st[r + 1]);
                x = (uint32_t)st[r] | sid << 16 | se << 24 | ee << 25;
                SID[r] += sid; ST[r] += se; EN[r + 1] += ee;
            } else {
                x = r == n ? (uint32_t)st[n] : (uint32_t)F.dummy();
            }
            R.rec[(size_t)r * D + d] = x;
        }
    }
    std::vector<uint32_t> sm(M, 0), em(M, 0);
    uint32_t cur = 0;
    for (uint32_t r = 0; r < M; ++r) {
        const bool chg = (r ? SID[r - 1] : 0) != SID[r];
        if (chg && ST[r]) cur = 1;
        else if (chg && EN[r]) cur = 0;
        sm[r] = cur;
    }
    cur = 0;
    for (uint32_t p = M; p-- > 0;) {
        const bool chg = SID[p + 1] != SID[p];     // SID[M] = ST[M] = EN[M] = 0
        if (chg && EN[p + 1]) cur = 1;
        else if (chg && ST[p + 1]) cur = 0;
        em[p] = cur;
    }
    for (uint32_t r = 0; r < M; ++r)
        if (sm[r] && em[r]) R.msk[r] = (uint16_t)((r < n ? (uint8_t)s[r] : 0) | SID[r] << 8);
    return R;
}

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T> &v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

// one string's rows behind the accessor verify_string takes, each array a heap block of exactly its size
struct OneString {
    std::unique_ptr<uint8_t[]> c;
    std::unique_ptr<uint32_t[]> r;
    std::unique_ptr<uint16_t[]> m;
    uint32_t D;
    explicit OneString(const Rows &R) : c(exact(R.chars)), r(exact(R.rec)), m(exact(R.msk)), D(R.D) {}
    uint32_t chr(size_t i) const { return c[i]; }
    uint32_t rec(size_t row, size_t d) const { return r[row * D + d]; }
    uint32_t msk(size_t row) const { return m[row]; }
};

// whole tiles out of an accessor: rows >= M hold garbage (they must never be judged), bytes >= n are never read
template <int T>
struct SrcTiles {
    const OneString &s;
    uint32_t n, M;
    void chars(uint32_t base, uint32_t (&c)[T]) const {
        for (int j = 0; j < T; ++j) c[j] = base + j < n ? s.chr(base + j) : 0u;
    }
    void masked(uint32_t base, uint32_t (&mk)[T]) const {
        for (int j = 0; j < T; ++j) mk[j] = base + j < M ? s.msk(base + j) : 0xdeadu;
    }
    void records(uint32_t d, uint32_t base, uint32_t (&x)[T]) const {
        for (int j = 0; j < T; ++j) x[j] = base + j < M ? s.rec(base + j, d) : 0xdeadbeefu;
    }
    uint32_t record(uint32_t d, uint32_t r) const { return s.rec(r, d); }
};

static std::vector<uint32_t> image_of(const std::vector<Def> &defs) {
    std::vector<std::vector<uint64_t>> tr, ep;
    std::vector<VerifyDefRows> rows;
    for (const Def &F : defs) { tr.push_back(F.transition_rows()); ep.push_back(F.endpoint_rows()); }
    for (size_t d = 0; d < defs.size(); ++d) rows.push_back({tr[d].data(), tr[d].size() / 4, ep[d].data(), ep[d].size() / 3, defs[d].first, defs[d].accepted});
    std::vector<uint32_t> img;
    if (!build_verify_image(rows.data(), rows.size(), img)) { std::printf("build_verify_image failed\n"); std::exit(2); }
    return img;
}

// the word of one string: the row-by-row loop, and the tile loop in every instantiation the kernel uses for this number of defs
static uint64_t word_of(const std::vector<uint32_t> &image, const Rows &R) {
    const std::unique_ptr<uint32_t[]> img = exact(image);
    const OneString s(R);
    const uint64_t v = verify_string(img.get(), R.D, R.n, R.M, s);
    EXPECT((verify_lane<0, 8>(img.get(), R.D, R.n, R.M, SrcTiles<8>{s, R.n, R.M}) == v));
    if (R.D == 1) EXPECT((verify_lane<1, 32>(img.get(), R.D, R.n, R.M, SrcTiles<32>{s, R.n, R.M}) == v));
    if (R.D == 2) EXPECT((verify_lane<2, 16>(img.get(), R.D, R.n, R.M, SrcTiles<16>{s, R.n, R.M}) == v));
    if (R.D == 3) EXPECT((verify_lane<3, 16>(img.get(), R.D, R.n, R.M, SrcTiles<16>{s, R.n, R.M}) == v));
    if (R.D == 4) EXPECT((verify_lane<4, 8>(img.get(), R.D, R.n, R.M, SrcTiles<8>{s, R.n, R.M}) == v));
    return v;
}

static uint32_t bits_of(uint64_t v) { return (uint32_t)v; }
static uint32_t row_of(uint64_t v) { return (uint32_t)(v >> 32); }
static std::string abba(uint32_t i, uint32_t j, uint32_t k) { return std::string(i, 'a') + std::string(j, 'b') + std::string(k, 'a'); }

// clean rows at M = 1, 7, 64, 65, n = 0 .. M: 0, or exactly the accept chain at row n
static void clean_rows(const std::vector<Def> &defs) {
    const std::vector<uint32_t> img = image_of(defs);
    for (uint32_t M : {1u, 7u, 64u, 65u})
        for (uint32_t n = 0; n <= M; ++n)
            for (uint32_t shape = 0; shape < 4; ++shape) {
                // a^i b^j a^k with i + j + k = n: all a; a leading run of b; b in the middle; b up to the end
                uint32_t i = 0, j = 0;
                if (shape == 1) j = n / 2;
                if (shape == 2) { i = n / 3; j = n / 3; }
                if (shape == 3) { i = n / 2; j = n - i; }
                const Rows R = make_rows(defs, abba(i, j, n - i - j), M);
                const uint64_t v = word_of(img, R);
                const uint64_t want = n == M || R.accepted_all ? 0 : (uint64_t)kVfyAccept | (uint64_t)n << 32;
                if (v != want) std::printf("clean: M %u n %u shape %u D %zu: %llx, expected %llx\n", M, n, shape, defs.size(), (unsigned long long)v, (unsigned long long)want);
                EXPECT(v == want);
            }
    Rows R = make_rows(defs, "ab", 7);
    R.n = 8;                                                   // n > M: no rows
    EXPECT(verify_string(exact(img).get(), R.D, R.n, R.M, OneString(R)) == ~0ull);
}

// one cell changed: the check that pins it, at its row
static void tampered_rows() {
    const std::vector<Def> defs = {kDef1, kDef2};
    const std::vector<uint32_t> img = image_of(defs);
    for (uint32_t M : {64u, 65u}) {
        // rows 0..4 a, 5..20 b (revealed by def 1; row 0 by def 2), 21..29 a; n = 30: every def accepts
        const Rows clean = make_rows(defs, abba(5, 16, 9), M);
        EXPECT(word_of(img, clean) == 0);
        EXPECT(clean.msk[0] == ('a' | 2 << 8) && clean.msk[5] == ('b' | 1 << 8) && clean.msk[20] == ('b' | 1 << 8) && clean.msk[4] == 0 && clean.msk[21] == 0);
        const uint32_t n = clean.n;
        auto rec = [](Rows &R, uint32_t r, uint32_t d) -> uint32_t & { return R.rec[(size_t)r * R.D + d]; };
        uint64_t v;
        Rows R = clean;
        rec(R, 10, 0) = (rec(R, 10, 0) & 0xffff0000u) | 2u;        // a wrong state: the pair (9, 10) leaves the transition table
        v = word_of(img, R);
        EXPECT((bits_of(v) & kVfyTransition) && row_of(v) == 9);
        R = clean;
        rec(R, 0, 1) = (rec(R, 0, 1) & 0xffff0000u) | 1u;          // def 2 does not start in its first state
        v = word_of(img, R);
        EXPECT((bits_of(v) & kVfyFirstState) && row_of(v) == 0);
        R = clean;
        rec(R, 25, 0) |= 1u << 16;                                  // a substr id the table does not hold for (2, a, 2)
        v = word_of(img, R);
        EXPECT((bits_of(v) & kVfyTransition) && row_of(v) == 25);
        R = clean;
        rec(R, 23, 0) |= 1u << 24;                                  // a start flag on an untagged row
        v = word_of(img, R);
        EXPECT((bits_of(v) & kVfyStartLookup) && (bits_of(v) & kVfyFlags) && !(bits_of(v) & kVfyTransition) && row_of(v) == 23);
        R = clean;
        rec(R, 23, 0) |= 1u << 25;                                  // an end flag on an untagged row
        v = word_of(img, R);
        EXPECT((bits_of(v) & kVfyEndLookup) && (bits_of(v) & kVfyFlags) && row_of(v) == 23);
        R = clean;
        rec(R, 5, 0) &= ~(1u << 24);                                // verify() cannot see a dropped start flag; the completeness check does
        v = word_of(img, R);
        EXPECT((bits_of(v) & kVfyFlags) && !(bits_of(v) & (kVfyFirstState | kVfyTransition | kVfyStartLookup | kVfyEndLookup | kVfyAccept)) && row_of(v) == 5);
        R = clean;
        rec(R, n, 0) = 1u;                                          // the state where enable drops: the pair (n - 1, n) and the accept chain
        v = word_of(img, R);
        EXPECT((bits_of(v) & kVfyAccept) && (bits_of(v) & kVfyTransition) && row_of(v) == n - 1);
        R = clean;
        rec(R, n + 3, 1) = 0;                                       // padding rows hold the dummy state
        v = word_of(img, R);
        EXPECT(bits_of(v) == kVfyPadding && row_of(v) == n + 3);
        R = clean;
        rec(R, M - 1, 0) |= 1u << 16;                               // ... and no tag, up to the last row
        v = word_of(img, R);
        EXPECT(bits_of(v) == kVfyPadding && row_of(v) == M - 1);
        R = clean;
        rec(R, 7, 1) |= 4u << 24;                                   // a flag bit that does not exist
        v = word_of(img, R);
        EXPECT(bits_of(v) == kVfyPadding && row_of(v) == 7);
        for (uint32_t r : {0u, 5u, 12u, 20u}) {                     // a revealed cell blanked
            R = clean;
            R.msk[r] = 0;
            v = word_of(img, R);
            EXPECT(bits_of(v) == kVfyMask && row_of(v) == r);
        }
        for (uint32_t r : {1u, 4u, 21u, n, M - 1}) {                // a cell revealed outside every range
            R = clean;
            R.msk[r] = 'a' | 1 << 8;
            v = word_of(img, R);
            EXPECT(bits_of(v) == kVfyMask && row_of(v) == r);
        }
        R = clean;
        R.msk[9] = 'a' | 1 << 8;                                    // the wrong byte inside a range
        v = word_of(img, R);
        EXPECT(bits_of(v) == kVfyMask && row_of(v) == 9);
        R = clean;
        rec(R, 0, 0) |= 1u << 24;                                   // two defs flag row 0: the masked rows are out of contract, their check is not reported
        R.msk[12] = 0;
        v = word_of(img, R);
        EXPECT(!(bits_of(v) & kVfyMask) && (bits_of(v) & kVfyStartLookup) && row_of(v) == 0);
    }
    // n == M: the transition and end lookups of row M - 1 read a cell nobody assigns and are left out; everything else of that row is judged
    Rows R = make_rows(defs, abba(5, 16, 43), 64);
    EXPECT(word_of(img, R) == 0);
    R.rec[(size_t)63 * 2] = (R.rec[(size_t)63 * 2] & 0xffff0000u) | 1u;        // state of row 63: the pair (62, 63) breaks, the pair (63, 64) is not looked at
    uint64_t v = word_of(img, R);
    EXPECT(bits_of(v) == kVfyTransition && row_of(v) == 62);
}

// values outside every table — the state 0xffff, the tag 0xff, flag bit 31, each alone, with a start and an end flag beside it, and all of them at once — in every def
// of one to five defs, at rows on both sides of the borders of every tile size, of n and of M.  The image is a heap block of exactly its size (word_of), so a lookup
// that verify_def_look did not clamp is a sanitizer error; the tile loop of every instantiation the kernel uses must give the row-by-row loop's word, and the word the
// check that pins the cell: the pair (r - 1, r) or the first-state gate for a state at r <= n, the padding rule behind n and for the flag bit, the transition lookup
// for a tag below n.
static void out_of_range_rows(const std::vector<Def> &defs) {
    const std::vector<uint32_t> img = image_of(defs);
    const uint32_t D = (uint32_t)defs.size();
    for (uint32_t M : {33u, 64u, 65u}) {
        const Rows clean = make_rows(defs, abba(5, 16, 9), M);
        const uint32_t n = clean.n;
        const uint64_t v0 = word_of(img, clean);
        EXPECT(v0 == (clean.accepted_all ? 0 : (uint64_t)kVfyAccept | (uint64_t)n << 32));
        for (uint32_t d = 0; d < D; ++d)
            for (uint32_t r : {0u, 1u, 5u, 7u, 8u, 15u, 16u, 17u, 20u, n - 1, n, 31u, 32u, M - 2, M - 1})
                for (int kind = 0; kind < 6; ++kind) {
                    Rows R = clean;
                    uint32_t &x = R.rec[(size_t)r * D + d];
                    uint32_t bit = 0;
                    if (kind == 0 || kind == 3) { x = (x & 0xffff0000u) | 0xffffu; bit = r == 0 ? kVfyFirstState : r <= n ? kVfyTransition : kVfyPadding; }
                    if (kind == 1 || kind == 4) { x |= 0xffu << 16; bit = r < n ? kVfyTransition : kVfyPadding; }
                    if (kind == 2) { x |= 1u << 31; bit = kVfyPadding; }
                    if (kind == 3 || kind == 4) x |= 3u << 24;          // the start and the end lookup run on the value that is out of range
                    if (kind == 5) { x = 0xffffffffu; bit = kVfyPadding; }
                    const uint64_t v = word_of(img, R);
                    if (!(bits_of(v) & bit) || (v >> 57) != 0 || row_of(v) > r)
                        std::printf("out of range: M %u D %u def %u row %u kind %d: %llx\n", M, D, d, r, kind, (unsigned long long)v);
                    EXPECT((bits_of(v) & bit) && (v >> 57) == 0 && row_of(v) <= r);
                }
        for (uint32_t r : {0u, 7u, 8u, 31u, 32u, M - 1}) {             // a masked cell of all ones
            Rows R = clean;
            R.msk[r] = 0xffffu;
            const uint64_t v = word_of(img, R);
            EXPECT((bits_of(v) & kVfyMask) && row_of(v) <= r);
        }
    }
}

// the same rows as a string-major, a pitched and a position-major image through verify_rows_host (threads included), B strings of every length class
static void images(const std::vector<Def> &defs, uint32_t M, size_t B) {
    const std::vector<uint32_t> image = image_of(defs);
    const std::unique_ptr<uint32_t[]> img = exact(image);
    const uint32_t D = (uint32_t)defs.size();
    const size_t stride = ((size_t)M + 15) / 16 * 16, rp = M + 3, mp = M + 5, q4 = ((size_t)M + 3) / 4, q8 = ((size_t)M + 7) / 8;
    std::vector<uint32_t> lens(B);
    std::vector<uint8_t> c_sm(B * stride, 0), c_pm(B * stride, 0);
    std::vector<uint32_t> r_sm(B * M * D), r_pit(B * rp * D, 0xdeadbeefu), r_pm(q4 * 4 * D * B, 0xdeadbeefu);
    std::vector<uint16_t> m_sm(B * M), m_pit(B * mp, 0xdead), m_pm(q8 * 8 * B, 0xdead);
    std::vector<uint64_t> want(B);
    for (size_t b = 0; b < B; ++b) {
        const uint32_t n = b % 5 == 0 ? 0 : b % 5 == 1 ? M : (uint32_t)((b * 7) % (M + 1));
        Rows R = make_rows(defs, abba(n / 4, n / 2, n - n / 4 - n / 2), M);
        if (b % 3 == 2 && M > 2) R.msk[M / 2] ^= 0x0101;          // some strings carry a wrong masked cell
        lens[b] = n;
        want[b] = verify_string(img.get(), D, n, M, OneString(R));
        const size_t k = b / HRX_PM_BLOCK, bl = b % HRX_PM_BLOCK, nb = std::min<size_t>(HRX_PM_BLOCK, B - k * HRX_PM_BLOCK);
        for (uint32_t i = 0; i < n; ++i) {
            c_sm[b * stride + i] = R.chars[i];
            c_pm[k * HRX_PM_BLOCK * stride + ((i / 16) * nb + bl) * 16 + i % 16] = R.chars[i];
        }
        for (uint32_t r = 0; r < M; ++r) {
            for (uint32_t d = 0; d < D; ++d) {
                const uint32_t x = R.rec[(size_t)r * D + d];
                r_sm[(b * M + r) * D + d] = x;
                r_pit[(b * rp + r) * D + d] = x;
                r_pm[k * HRX_PM_BLOCK * q4 * D * 4 + ((r / 4 * D + d) * nb + bl) * 4 + r % 4] = x;
            }
            m_sm[b * M + r] = m_pit[b * mp + r] = R.msk[r];
            m_pm[k * HRX_PM_BLOCK * q8 * 8 + (r / 8 * nb + bl) * 8 + r % 8] = R.msk[r];
        }
    }
    const auto lens_x = exact(lens);
    const auto c_sm_x = exact(c_sm), c_pm_x = exact(c_pm);
    const auto r_sm_x = exact(r_sm), r_pit_x = exact(r_pit), r_pm_x = exact(r_pm);
    const auto m_sm_x = exact(m_sm), m_pit_x = exact(m_pit), m_pm_x = exact(m_pm);
    for (int form = 0; form < 4; ++form) {
        std::unique_ptr<uint64_t[]> out(new uint64_t[B]);
        for (size_t b = 0; b < B; ++b) out[b] = 0x5555555555555555ull;
        VerifyArgs a{};
        a.lens = lens_x.get(); a.stride = stride; a.B = (uint32_t)B; a.M = M; a.D = D; a.image = img.get(); a.verdict = out.get();
        a.rec_pitch = a.msk_pitch = M;
        if (form == 0) { a.layout = 0; a.chars = c_sm_x.get(); a.records = r_sm_x.get(); a.masked = m_sm_x.get(); }
        if (form == 1) { a.layout = 0; a.chars = c_sm_x.get(); a.records = r_pit_x.get(); a.masked = m_pit_x.get(); a.rec_pitch = rp; a.msk_pitch = mp; }
        if (form == 2) { a.layout = 1; a.chars = c_sm_x.get(); a.records = r_pm_x.get(); a.masked = m_pm_x.get(); }
        if (form == 3) { a.layout = 3; a.chars = c_pm_x.get(); a.records = r_pm_x.get(); a.masked = m_pm_x.get(); }
        verify_rows_host(a, form == 0 ? 1u : 3u);
        size_t bad = 0;
        for (size_t b = 0; b < B; ++b) bad += out[b] != want[b];
        if (bad) std::printf("images: M %u B %zu D %u form %d: %zu words differ\n", M, B, D, form, bad);
        EXPECT(bad == 0);
    }
}

int main() {
    const std::vector<Def> one = {kDef1}, two = {kDef1, kDef2}, three = {kDef1, kDef2, kDef3}, four = {kDef3, kDef1, kDef3, kDef2},
                           five = {kDef1, kDef3, kDef2, kDef3, kDef3};
    for (const auto *defs : {&one, &two, &three, &four, &five}) clean_rows(*defs);
    tampered_rows();
    for (const auto *defs : {&one, &two, &three, &four, &five}) out_of_range_rows(*defs);
    for (uint32_t M : {1u, 7u, 64u, 65u}) {
        images(one, M, 11);
        images(two, M, 130);
        images(five, M, 7);
    }
    images(one, 7, HRX_PM_BLOCK + 3);          // a second block of three strings
    // tables a dense array cannot hold are refused
    std::vector<uint64_t> tr = kDef1.transition_rows(), ep = kDef1.endpoint_rows();
    std::vector<uint32_t> img;
    tr[1] = 7;                                 // the first row is not the dummy row
    VerifyDefRows bad{tr.data(), tr.size() / 4, ep.data(), ep.size() / 3, 0, 2};
    EXPECT(!build_verify_image(&bad, 1, img));
    if (failures) {
        std::printf("verify host: %d failures\n", failures);
        return 1;
    }
    std::printf("verify host: ok\n");
    return 0;
}
