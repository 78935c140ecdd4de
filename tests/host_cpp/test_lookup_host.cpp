// test_lookup_host.cpp — csrc/hrx_lookup.hpp and csrc/hrx_lookup_host.cpp (the rule and the host form of LOOKUP COUNTS, include/hrx.h) as a program of their own,
// built with -fsanitize=address,undefined by tests/test_lookup_cpu.py.  Every array is a heap block of exactly its size, so one element too far is a sanitizer
// error.  The rows are hand-made: two small DFAs over {a, b} whose table rows are written out below and a walk of them in the words of src/lib.rs.  The
// yardstick forms each row's three tuples as lib.rs:218-283 writes them and searches the table rows for the whole tuple, lowest row first — no image.
// Checked: every n = 0 .. M at M = 1, 4, 5, 9; the sums; a duplicate endpoint row; states, ids and flags outside every table (misses, no read outside the
// image); the string-major, pitched and position-major images of the same rows the same words through lookup_counts_host, windows included; n > M; what
// build_lookup_image refuses; plan_lookup's bounds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_lookup_host.cpp"

using namespace hrx;

static int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #c);               \
            ++failures;                                               \
        }                                                             \
    } while (0)

struct Def {
    uint64_t first, accepted, largest;
    std::vector<std::vector<uint64_t>> trans;      // {cur, char, next}
    uint64_t sid;
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
    std::vector<uint64_t> transition_rows() const {     // table.rs:68-125
        std::vector<uint64_t> r = {0, dummy(), dummy(), 0};
        for (auto &t : trans) { r.push_back(t[1]); r.push_back(t[0]); r.push_back(t[2]); r.push_back(is_tagged(t[0], t[2]) ? sid : 0); }
        return r;
    }
    std::vector<uint64_t> endpoint_rows() const {       // table.rs:126-196
        std::vector<uint64_t> r = {0, dummy(), dummy()};
        for (uint64_t s : starts) { r.push_back(sid); r.push_back(s); r.push_back(dummy()); }
        for (uint64_t e : ends) { r.push_back(sid); r.push_back(dummy()); r.push_back(e); }
        return r;
    }
    uint64_t step(uint64_t cur, uint8_t c) const {
        for (auto &t : trans)
            if (t[0] == cur && t[1] == c) return t[2];
        std::abort();
    }
};

// a* b+ a*: substring 1 = the run of b; the start state is named twice: two endpoint rows hold (1, 0, dummy)
static const Def kDef1 = {0, 2, 2, {{0, 'a', 0}, {0, 'b', 1}, {1, 'b', 1}, {1, 'a', 2}, {2, 'a', 2}}, 1, {{0, 1}, {1, 1}}, {0, 0}, {1}};
// anything: substring 2 = the first a
static const Def kDef2 = {0, 1, 1, {{0, 'b', 0}, {0, 'a', 1}, {1, 'a', 1}, {1, 'b', 1}}, 2, {{0, 1}}, {0}, {1}};

// match_substrs in plain words (lib.rs:387-519): records [M][D]
static std::vector<uint32_t> make_rows(const std::vector<Def> &defs, const std::string &s, uint32_t M) {
    const uint32_t D = (uint32_t)defs.size(), n = (uint32_t)s.size();
    std::vector<uint32_t> rec((size_t)M * D);
    for (uint32_t d = 0; d < D; ++d) {
        const Def &F = defs[d];
        std::vector<uint64_t> st(n + 1);
        st[0] = F.first;
        for (uint32_t i = 0; i < n; ++i) st[i + 1] = F.step(st[i], (uint8_t)s[i]);
        for (uint32_t r = 0; r < M; ++r) {
            uint32_t state = r <= n ? (uint32_t)st[r] : (uint32_t)F.dummy(), sid = 0, se = 0, ee = 0;
            if (r < n && F.is_tagged(st[r], st[r + 1])) {
                sid = (uint32_t)F.sid;
                se = Def::in(F.starts, st[r]);
                ee = r + 1 < M && Def::in(F.ends, st[r + 1]);
            }
            rec[(size_t)r * D + d] = state | sid << 16 | se << 24 | ee << 25;
        }
    }
    return rec;
}

struct Expected {
    std::vector<uint32_t> run;
    uint32_t misses;
};

// the yardstick: tuples as lib.rs writes them, a linear search over the table rows
static Expected brute(const std::vector<Def> &defs, const std::string &s, uint32_t M, const uint32_t *rec) {
    const uint32_t D = (uint32_t)defs.size(), n = (uint32_t)s.size();
    size_t W = 0;
    for (auto &F : defs) W += F.transition_rows().size() / 4 + 2 * (F.endpoint_rows().size() / 3);
    Expected e{std::vector<uint32_t>((W + 3) / 4 * 4, 0u), 0u};
    size_t off = 0;
    for (uint32_t d = 0; d < D; ++d) {
        const std::vector<uint64_t> tr = defs[d].transition_rows(), ep = defs[d].endpoint_rows();
        const size_t T = tr.size() / 4, E = ep.size() / 3;
        const uint64_t dm = defs[d].dummy();
        auto find3 = [&](uint64_t a, uint64_t b, uint64_t c, size_t base) {
            for (size_t k = 0; k < E; ++k)
                if (ep[3 * k] == a && ep[3 * k + 1] == b && ep[3 * k + 2] == c) { ++e.run[base + k]; return; }
            ++e.misses;
        };
        for (uint32_t r = 0; r < M; ++r) {
            const uint32_t x = rec[(size_t)r * D + d];
            const uint64_t en = r < n, cur = x & 0xffffu, sid = (x >> 16) & 0xffu, se = (x >> 24) & 1u, ee = (x >> 25) & 1u;
            const uint64_t nxt = r + 1 < M ? rec[(size_t)(r + 1) * D + d] & 0xffffu : dm, c = en ? (uint8_t)s[r] : 0;
            const bool unassigned = r + 1 == M && n == M;
            if (!unassigned) {
                const uint64_t t[4] = {en * c, en * cur + (1 - en) * dm, en * nxt + (1 - en) * dm, en * sid};
                bool hit = false;
                for (size_t k = 0; k < T && !hit; ++k)
                    if (tr[4 * k] == t[0] && tr[4 * k + 1] == t[1] && tr[4 * k + 2] == t[2] && tr[4 * k + 3] == t[3]) { ++e.run[off + k]; hit = true; }
                if (!hit) ++e.misses;
            }
            find3(se * sid, se * cur + (1 - se) * dm, dm, off + T);
            if (!unassigned) find3(ee * sid, dm, ee * nxt + (1 - ee) * dm, off + T + E);
        }
        off += T + 2 * E;
    }
    return e;
}

struct Image {
    std::unique_ptr<uint32_t[]> words;      // exactly the image's size
    size_t size;
};
static bool image_of(const std::vector<Def> &defs, Image &out) {
    std::vector<std::vector<uint64_t>> tr, ep;
    std::vector<VerifyDefRows> rows;
    for (auto &F : defs) { tr.push_back(F.transition_rows()); ep.push_back(F.endpoint_rows()); }
    for (size_t d = 0; d < defs.size(); ++d) rows.push_back(VerifyDefRows{tr[d].data(), tr[d].size() / 4, ep[d].data(), ep[d].size() / 3, defs[d].first, defs[d].accepted});
    std::vector<uint32_t> img;
    if (!build_lookup_image(rows.data(), rows.size(), img)) return false;
    out.size = img.size();
    out.words.reset(new uint32_t[img.size()]);
    memcpy(out.words.get(), img.data(), img.size() * 4);
    return true;
}

// one string's rows as lookup_string reads them
struct Acc {
    const std::string &s;
    const uint32_t *r_;
    uint32_t D;
    uint32_t chr(size_t i) const { return (uint8_t)s[i]; }
    uint32_t rec(size_t r, size_t d) const { return r_[r * D + d]; }
};

static void check_string(const std::vector<Def> &defs, const Image &img, const std::string &s, uint32_t M, const uint32_t *rec, bool clean) {
    const uint32_t D = (uint32_t)defs.size(), W = lookup_words(img.words.get(), D);
    const Expected want = brute(defs, s, M, rec);
    EXPECT(W == want.run.size());
    std::unique_ptr<uint32_t[]> got(new uint32_t[W]);
    const uint32_t misses = lookup_string(img.words.get(), D, (uint32_t)s.size(), M, Acc{s, rec, D}, got.get());
    EXPECT(misses == want.misses);
    EXPECT(memcmp(got.get(), want.run.data(), (size_t)W * 4) == 0);
    if (clean) {
        EXPECT(misses == 0);
        const LookupDef *L = reinterpret_cast<const LookupDef *>(img.words.get());
        for (uint32_t d = 0; d < D; ++d) {
            uint32_t t = 0, st = 0, en = 0;
            for (uint32_t k = 0; k < L[d].n_tr; ++k) t += got[L[d].off + k];
            for (uint32_t k = 0; k < L[d].n_ep; ++k) { st += got[L[d].off + L[d].n_tr + k]; en += got[L[d].off + L[d].n_tr + L[d].n_ep + k]; }
            const uint32_t full = M - (s.size() == M ? 1u : 0u);
            EXPECT(t == full && st == M && en == full);
        }
    }
}

int main() {
    const std::vector<Def> two = {kDef1, kDef2}, one = {kDef1};
    Image img2, img1;
    EXPECT(image_of(two, img2) && image_of(one, img1));
    // clean rows, every n
    const std::string text = "aabbbaaaa";      // every piece of it is a string def 1 has transitions for
    for (uint32_t M : {1u, 4u, 5u, 9u})
        for (uint32_t n = 0; n <= M && n <= text.size(); ++n) {
            const std::string s = text.substr(0, n);
            const std::vector<uint32_t> r2 = make_rows(two, s, M), r1 = make_rows(one, s, M);
            std::unique_ptr<uint32_t[]> h2(new uint32_t[r2.size()]), h1(new uint32_t[r1.size()]);
            memcpy(h2.get(), r2.data(), r2.size() * 4);
            memcpy(h1.get(), r1.data(), r1.size() * 4);
            check_string(two, img2, s, M, h2.get(), true);
            check_string(one, img1, s, M, h1.get(), true);
        }
    {   // the duplicate endpoint row: "abba" raises def 1's start flag once, at row 1 (state 0 -> 1 is the first tagged pair)
        const std::string s = "abba";
        const std::vector<uint32_t> r = make_rows(one, s, 8);
        std::unique_ptr<uint32_t[]> got(new uint32_t[lookup_words(img1.words.get(), 1)]);
        EXPECT(lookup_string(img1.words.get(), 1, 4, 8, Acc{s, r.data(), 1}, got.get()) == 0);
        const LookupDef *L = reinterpret_cast<const LookupDef *>(img1.words.get());
        EXPECT(L[0].n_ep == 4 && got[L[0].n_tr + 0] == 7 && got[L[0].n_tr + 1] == 1 && got[L[0].n_tr + 2] == 0 && got[L[0].n_tr + 3] == 0);
    }
    // values outside every table, every row and def in turn: states, ids, flags, everything
    for (uint32_t M : {5u, 9u}) {
        const std::string s = text.substr(0, 5);
        const std::vector<uint32_t> clean = make_rows(two, s, M);
        for (size_t cell = 0; cell < clean.size(); ++cell)
            for (uint32_t bits : {0x0000ffffu, 0x00ff0000u, 0x01ff0000u, 0x02ff0000u, 0xfc000000u, 0xffffffffu, 0x00000001u, 0x03000000u}) {
                std::unique_ptr<uint32_t[]> h(new uint32_t[clean.size()]);
                memcpy(h.get(), clean.data(), clean.size() * 4);
                h[cell] ^= bits;
                check_string(two, img2, s, M, h.get(), false);
            }
    }
    {   // a batch through lookup_counts_host: string-major, pitched, position-major (records and input), windows, n > M
        const uint32_t M = 9, D = 2, B = 7, stride = 16, pitch = M + 3, Q = (M + 3) / 4;
        const uint32_t W = lookup_words(img2.words.get(), D);
        std::unique_ptr<uint8_t[]> chars(new uint8_t[B * stride]()), chars_pm(new uint8_t[B * stride]());
        std::unique_ptr<uint32_t[]> lens(new uint32_t[B]), sm(new uint32_t[B * M * D]), pit(new uint32_t[B * pitch * D]), pm(new uint32_t[Q * D * B * 4]());
        std::vector<Expected> want;
        for (uint32_t i = 0; i < B * pitch * D; ++i) pit[i] = 0xffffffffu;
        for (uint32_t b = 0; b < B; ++b) {
            const std::string s = text.substr(b % 3, b);
            lens[b] = (uint32_t)s.size();
            memcpy(&chars[b * stride], s.data(), s.size());
            memcpy(&chars_pm[b * 16], s.data(), s.size());       // one 16-byte chunk per string: chunk 0 of a block of B strings
            const std::vector<uint32_t> r = make_rows(two, s, M);
            want.push_back(brute(two, s, M, r.data()));
            for (uint32_t row = 0; row < M; ++row)
                for (uint32_t d = 0; d < D; ++d) {
                    sm[(b * M + row) * D + d] = pit[(b * pitch + row) * D + d] = r[row * D + d];
                    pm[((row / 4 * D + d) * B + b) * 4 + row % 4] = r[row * D + d];
                }
        }
        for (int form = 0; form < 4; ++form)
            for (uint32_t b_begin : {0u, 2u, 6u}) {
                const uint32_t b_count = b_begin == 0 ? B : b_begin == 2 ? 3u : 1u;
                std::unique_ptr<uint32_t[]> counts(new uint32_t[b_count * W]), misses(new uint32_t[b_count]);
                LookupArgs a{};
                a.chars = form == 3 ? chars_pm.get() : chars.get(); a.stride = stride; a.lens = lens.get();
                a.records = form == 0 ? sm.get() : form == 1 ? pit.get() : pm.get();
                a.rec_pitch = form == 1 ? pitch : M;
                a.layout = form < 2 ? 0u : form == 2 ? 1u : 3u;
                a.n_stripes = 1; a.B = B; a.M = M; a.D = D; a.b_begin = b_begin; a.b_count = b_count;
                a.image = img2.words.get(); a.W = W; a.counts = counts.get(); a.misses = form == 1 ? nullptr : misses.get();
                lookup_counts_host(a, 3);
                for (uint32_t i = 0; i < b_count; ++i) {
                    EXPECT(memcmp(&counts[i * W], want[b_begin + i].run.data(), (size_t)W * 4) == 0);
                    if (a.misses) EXPECT(misses[i] == want[b_begin + i].misses && misses[i] == 0);
                }
            }
        lens[4] = M + 1;
        std::unique_ptr<uint32_t[]> counts(new uint32_t[B * W]), misses(new uint32_t[B]);
        LookupArgs a{};
        a.chars = chars.get(); a.stride = stride; a.lens = lens.get(); a.records = sm.get(); a.rec_pitch = M; a.n_stripes = 1;
        a.B = B; a.M = M; a.D = D; a.b_count = B; a.image = img2.words.get(); a.W = W; a.counts = counts.get(); a.misses = misses.get();
        lookup_counts_host(a, 1);
        EXPECT(misses[4] == kLkTooLong && misses[3] == 0);
        for (uint32_t k = 0; k < W; ++k) EXPECT(counts[4 * W + k] == 0);
        EXPECT(memcmp(&counts[5 * W], want[5].run.data(), (size_t)W * 4) == 0);
    }
    {   // what the builder refuses
        Def bad = kDef1;
        bad.trans.push_back({0, 'a', 1});                   // a second row with the key (a, 0) that disagrees
        Image x;
        EXPECT(!image_of({bad}, x));
        Def same = kDef1;
        same.trans.push_back({0, 'a', 0});                  // ... that agrees: the lower row takes the counts
        EXPECT(image_of({same}, x));
        const std::string s = "aab";
        const std::vector<uint32_t> r = make_rows({same}, s, 4);
        std::unique_ptr<uint32_t[]> h(new uint32_t[r.size()]);
        memcpy(h.get(), r.data(), r.size() * 4);
        check_string({same}, x, s, 4, h.get(), true);
        std::vector<uint32_t> img;
        EXPECT(!build_lookup_image(nullptr, 0, img));
    }
    {   // the planner: powers of two, within the LDS of a CU, whole passes
        for (size_t W : {4u, 2860u, 16384u, 16388u, 40956u, 40960u, 66004u, 1000000u})
            for (size_t b : {1u, 3u, 300u, 65536u}) {
                const LookupPlan p = plan_lookup(W, b, 256);
                EXPECT(p.G >= 1 && (p.G & (p.G - 1)) == 0 && p.G <= kLkMaxGroup && p.pass_words % 4 == 0 && p.passes >= 1);
                EXPECT(p.lds_bytes == lookup_lds_bytes(p.G, p.pass_words) && p.lds_bytes <= kLkLdsAll && (p.G == 1 || p.lds_bytes <= kLkLdsShared));
                EXPECT((size_t)p.pass_words * p.passes >= W && (p.passes == 1 ? p.pass_words == W : p.G == 1 && (size_t)p.pass_words * (p.passes - 1) < W));
            }
        EXPECT(plan_lookup(2860, 65536, 256).G == 4 && plan_lookup(2860, 600, 256).G == 1 && plan_lookup(66004, 3, 256).passes == 2);
    }
    if (failures) {
        std::printf("lookup host: %d failures\n", failures);
        return 1;
    }
    std::printf("lookup host: ok\n");
    return 0;
}
