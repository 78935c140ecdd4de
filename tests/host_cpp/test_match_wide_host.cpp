// test_match_wide_host.cpp — the lane core of the fused-wide match (csrc/hrx_match_wide.h: MatchLaneWide, WideAcc, wide_status) as a program of its own on
// the host, built with -fsanitize=address,undefined by tests/test_match_wide_cpu.py.  The table reader is the CLASS-WIDE image in memory (a heap block of
// exactly its size); the loop around the tiles is the kernel's (only the string's own tiles, FULL where the tile allows it); the expectation is
// hrx_match_batch_host's native walk (csrc/hrx_host_walk.cpp), which tests/test_match_cpu.py pins to the oracle.
//   argv[1]: a batch file — u32 B, stride, M, n_defs; per def: u32 n_substrs, then n_substrs + 1 texts (u32 length + bytes: the allstr text, the substr texts);
//            lens [B] u32; chars [B][stride]
// Every def set in the file's order, then the same set twice over (two defs flag one row: the overlap status), each at every sweep width G.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_defs.cpp"
#include "../../halo2_regex_amd/csrc/hrx_host_walk.cpp"
#include "../../halo2_regex_amd/csrc/hrx_match_wide.h"

using namespace hrx;

static int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #c);               \
            ++failures;                                               \
        }                                                             \
    } while (0)

struct ImageMem {       // the image in memory: a heap block of exactly cw_image's size
    const uint8_t *img;
    uint32_t lo(uint32_t off) const { uint32_t v; std::memcpy(&v, img + off, 4); return v; }
    uint32_t lut(uint32_t off) const { return img[off]; }
};

struct Batch {
    uint32_t B = 0, stride = 0, M = 0;
    std::vector<std::vector<std::string>> defs;     // per def: the allstr text, then the substr texts
    std::vector<uint32_t> lens;
    std::vector<uint8_t> chars;
};

static bool read_batch(const char *path, Batch &b) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    auto u32 = [&](uint32_t &v) { return std::fread(&v, 4, 1, f) == 1; };
    uint32_t nd = 0;
    bool ok = u32(b.B) && u32(b.stride) && u32(b.M) && u32(nd);
    for (uint32_t d = 0; ok && d < nd; ++d) {
        uint32_t ns = 0;
        ok = u32(ns);
        b.defs.emplace_back();
        for (uint32_t k = 0; ok && k <= ns; ++k) {
            uint32_t len = 0;
            ok = u32(len);
            std::string t(len, '\0');
            ok = ok && (len == 0 || std::fread(&t[0], 1, len, f) == len);
            b.defs.back().push_back(t);
        }
    }
    b.lens.resize(b.B);
    b.chars.resize((size_t)b.B * b.stride);
    ok = ok && std::fread(b.lens.data(), 4, b.B, f) == b.B && std::fread(b.chars.data(), 1, b.chars.size(), f) == b.chars.size();
    std::fclose(f);
    return ok;
}

static DefsSet make_set(const std::vector<std::vector<std::string>> &defs) {
    DefsSet s;
    for (const auto &t : defs) {
        RegexDefs rd;
        if (parse_allstr_text(t[0].data(), t[0].size(), rd.allstr)) { std::printf("allstr text does not parse\n"); ++failures; }
        for (size_t k = 1; k < t.size(); ++k) {
            SubstrRegexDef sd;
            if (parse_substr_text(t[k].data(), t[k].size(), sd)) { std::printf("substr text does not parse\n"); ++failures; }
            rd.substrs.push_back(sd);
        }
        s.defs.push_back(rd);
    }
    std::string err;
    if (finalize_defs(s, err)) { std::printf("finalize: %s\n", err.c_str()); ++failures; }
    return s;
}

// the kernel's walk of one string (hrx_kernel_match_wide.hip): its own tiles only, the tile's bytes zero past n
template <int D, int G>
static void walk_string(const ImageMem &tab, const MatchWideArgs &a, const uint8_t *p, uint32_t n, size_t b, bool allow_full) {
    MatchLaneWide<D, G> lane{};
    lane.reset(a, b);
    const uint32_t M = a.M, nt = std::min(n, M - 1u) / 64u + 1u;
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t t0 = t * 64u;
        uint8_t bytes[64] = {};
        for (uint32_t i = 0; i < 64u && t0 + i < n; ++i) bytes[i] = p[t0 + i];
        uint32_t cw[16];
        std::memcpy(cw, bytes, 64);
        lane.tile(tab, a, cw, t0, n, t + 1 == nt, allow_full && t0 + 64u <= n && t0 + 64u < M, [&](uint32_t i) { return (uint32_t)p[i]; });
    }
    lane.finish(a, b);
}

template <int D, int G>
static void check(const char *name, const DefsSet &s, const Batch &bt, uint32_t max_spans, bool allow_full, uint32_t *n_overlap, uint32_t *n_runs) {
    const size_t B = bt.B;
    EXPECT(s.defs.size() == (size_t)D && !s.cw_image.empty() && s.cw_consts.size() == (size_t)D);
    if (s.cw_image.empty()) return;
    std::unique_ptr<uint8_t[]> img(new uint8_t[s.cw_image.size()]);
    std::memcpy(img.get(), s.cw_image.data(), s.cw_image.size());
    // outputs: heap blocks of exactly their sizes
    std::unique_ptr<uint64_t[]> st(new uint64_t[B]), want_st(new uint64_t[B]), sp(new uint64_t[B * max_spans + 1]), want_sp(new uint64_t[B * max_spans + 1]);
    std::unique_ptr<uint32_t[]> cnt(new uint32_t[B]), want_cnt(new uint32_t[B]);
    host_match_batch(s, bt.chars.data(), bt.stride, bt.lens.data(), B, bt.M, want_st.get(), want_cnt.get(), max_spans ? want_sp.get() : nullptr, max_spans, 1);
    MatchWideArgs a{};
    a.cw_image = img.get(); a.image_bytes = (uint32_t)s.cw_image.size(); a.cw_lut_off = s.cw_lut_off;
    a.B = (uint32_t)B; a.M = bt.M; a.D = D; a.max_spans = max_spans;
    a.status = st.get(); a.span_counts = cnt.get(); a.spans = max_spans ? sp.get() : nullptr;
    for (int d = 0; d < D; ++d) a.dc[d] = s.cw_consts[d];
    const ImageMem tab{img.get()};
    uint32_t bad = 0;
    for (size_t b = 0; b < B; ++b) {
        const uint32_t n = bt.lens[b];
        if (n > bt.M) { st[b] = kStatusBadLength; cnt[b] = 0; }        // (the kernel's shell: nothing read)
        else walk_string<D, G>(tab, a, bt.chars.data() + b * bt.stride, n, b, allow_full);
        bool same = st[b] == want_st[b] && cnt[b] == want_cnt[b];
        for (uint32_t k = 0; same && k < std::min(cnt[b], max_spans); ++k) same = sp[b * max_spans + k] == want_sp[b * max_spans + k];
        if (!same && bad++ < 5)
            std::printf("%s G=%d full=%d string %zu (n = %u): status %llx count %u, the host walk says %llx / %u\n", name, G, (int)allow_full, b, n,
                        (unsigned long long)st[b], cnt[b], (unsigned long long)want_st[b], want_cnt[b]);
        if ((want_st[b] & 0xff) == kStatusFlagOverlap) ++*n_overlap;
        *n_runs += want_cnt[b];
    }
    failures += bad;
}

template <int D>
static void check_all(const char *name, const DefsSet &s, const Batch &bt, uint32_t *n_overlap, uint32_t *n_runs) {
    check<D, 1>(name, s, bt, 8, true, n_overlap, n_runs);
    check<D, 2>(name, s, bt, 8, true, n_overlap, n_runs);
    check<D, 4>(name, s, bt, 8, true, n_overlap, n_runs);
    check<D, 2>(name, s, bt, 8, false, n_overlap, n_runs);      // the general walk on full tiles gives the same bits
    check<D, 2>(name, s, bt, 1, true, n_overlap, n_runs);       // truncation
    check<D, 1>(name, s, bt, 0, true, n_overlap, n_runs);       // status and counts only
}

int main(int argc, char **argv) {
    Batch bt;
    if (argc < 2 || !read_batch(argv[1], bt) || bt.defs.size() != 4) { std::printf("usage: test_match_wide_host BATCH_FILE (four defs)\n"); return 2; }
    uint32_t ov4 = 0, runs4 = 0, ov8 = 0, runs8 = 0;
    check_all<4>("four defs", make_set(bt.defs), bt, &ov4, &runs4);
    auto twice = bt.defs;
    twice.insert(twice.end(), bt.defs.begin(), bt.defs.end());
    check_all<8>("eight defs", make_set(twice), bt, &ov8, &runs8);
    auto six = bt.defs;
    six.insert(six.end(), bt.defs.begin() + 1, bt.defs.begin() + 3);
    uint32_t ov6 = 0, runs6 = 0;
    check_all<6>("six defs", make_set(six), bt, &ov6, &runs6);
    EXPECT(runs4 > 100 && ov4 == 0);        // the batch reveals something, and the plain set never overlaps
    EXPECT(ov8 > 100 && ov6 > 100);         // the doubled sets do
    if (failures) return 1;
    std::printf("match wide host: ok (%u strings, %u runs, %u overlaps at eight defs)\n", bt.B, runs4 / 6, ov8 / 6);
    return 0;
}
