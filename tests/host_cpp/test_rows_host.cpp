// test_rows_host.cpp — csrc/hrx_rows.hpp as a program of its own (tests/test_rows_cpu.py builds it with the address and undefined-behaviour sanitizers):
// every row form of include/hrx.h built INDEX BY INDEX from the formulas written out below, each cell a hash of (string, row, def), every buffer a heap
// block of its exact size; then the shared place (rows_place) must return exactly that cell through the single-cell accessors (RowsOf, chr_cell / rec_cell
// / msk_cell) and through the addresses of the kernels' vector loads (chr_chunk, msk_octet, rec_quad), for the first strings, both sides of the block
// border and the last string, every row and every def — with the masked rows and without them (masked == NULL).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_over_threads.hpp"
#include "../../halo2_regex_amd/csrc/hrx_rows.hpp"

using namespace hrx;

static int failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            if (++failures <= 20) std::printf("line %d: %s\n", __LINE__, #c); \
        }                                                              \
    } while (0)

static uint32_t cell(uint64_t b, uint64_t r, uint64_t d) {
    uint64_t x = (b + 1) * 0x9E3779B97F4A7C15ull ^ (r + 1) * 0xC2B2AE3D27D4EB4Full ^ (d + 1) * 0x165667B19E3779F9ull;
    x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
    return (uint32_t)x;
}
constexpr uint64_t kChr = 100, kMsk = 101;      // the "def" of an input byte / a masked cell
static uint8_t chr_of(size_t b, size_t i) { return (uint8_t)cell(b, i, kChr); }
static uint16_t msk_of(size_t b, size_t r) { return (uint16_t)cell(b, r, kMsk); }

template <class T>
static std::unique_ptr<T[]> block(size_t n, T fill) {
    std::unique_ptr<T[]> p(new T[n]);
    for (size_t i = 0; i < n; ++i) p[i] = fill;
    return p;
}

enum Form { kSm, kPm, kPlanes, kStripes };

struct Batch {
    RowsIn a{};
    std::unique_ptr<uint8_t[]> chars;
    std::unique_ptr<uint32_t[]> rec;
    std::unique_ptr<uint16_t[]> msk;
    std::vector<std::unique_ptr<uint32_t[]>> planes;
};

// include/hrx.h, "Output layouts" and "RECORD PLANES": with k = b / HRX_PM_BLOCK, b' = b % HRX_PM_BLOCK, nb = min(HRX_PM_BLOCK, B - k HRX_PM_BLOCK)
//   string-major     byte i at b stride + i; record (b, r, d) at (b rec_pitch + r) D + d; masked (b, r) at b msk_pitch + r
//   position-major   record at k HRX_PM_BLOCK ceil(M/4) D 4 + ((r/4 D + d) nb + b') 4 + r%4; masked at k HRX_PM_BLOCK ceil(M/8) 8 + (r/8 nb + b') 8 + r%8
//   input pos.-major byte i at k HRX_PM_BLOCK stride + ((i/16) nb + b') 16 + i%16
//   planes           record (b, r) of def d at plane[d][k HRX_PM_BLOCK ceil(M/4) 4 + ((r/4) nb + b') 4 + r%4]
//   two stripes      record (b, r) at stripe[(r/4) % 2][k HRX_PM_BLOCK ceil(ceil(M/4)/2) 4 + ((r/8) nb + b') 4 + r%4]
static Batch build(Form form, bool in_pm, size_t B, size_t M, size_t D, size_t stride, size_t rec_pitch, size_t msk_pitch) {
    Batch t;
    const size_t P = HRX_PM_BLOCK, q4 = (M + 3) / 4, q8 = (M + 7) / 8, last0 = (B - 1) / P * P, nb_last = B - last0;
    const size_t n_bufs = form == kPlanes ? D : form == kStripes ? 2 : 0, slots = form == kStripes ? (q4 + 1) / 2 : q4;
    t.chars = block<uint8_t>(B * stride, 0xEE);
    if (form == kSm) {
        t.rec = block<uint32_t>(B * rec_pitch * D, 0xdeadbeefu);
        t.msk = block<uint16_t>(B * msk_pitch, 0xdead);
    } else {
        if (form == kPm) t.rec = block<uint32_t>(B * q4 * 4 * D, 0xdeadbeefu);
        t.msk = block<uint16_t>(B * q8 * 8, 0xdead);
        // a stripe ends with its last used slot of the last block: stripe 1 of an odd number of quads holds one slot less than stripe 0
        for (size_t p = 0; p < n_bufs; ++p) {
            const size_t used = form == kStripes ? (q4 - p + 1) / 2 : q4;
            t.planes.push_back(block<uint32_t>(last0 * slots * 4 + used * nb_last * 4, 0xdeadbeefu));
        }
    }
    for (size_t b = 0; b < B; ++b) {
        const size_t k = b / P, bl = b % P, nb = B - k * P < P ? B - k * P : P;
        for (size_t i = 0; i < (in_pm ? stride : M); ++i)
            t.chars[in_pm ? k * P * stride + ((i / 16) * nb + bl) * 16 + i % 16 : b * stride + i] = chr_of(b, i);
        for (size_t r = 0; r < M; ++r) {
            for (size_t d = 0; d < D; ++d) {
                const uint32_t x = cell(b, r, d);
                if (form == kSm) t.rec[(b * rec_pitch + r) * D + d] = x;
                if (form == kPm) t.rec[k * P * q4 * D * 4 + ((r / 4 * D + d) * nb + bl) * 4 + r % 4] = x;
                if (form == kPlanes) t.planes[d][k * P * q4 * 4 + ((r / 4) * nb + bl) * 4 + r % 4] = x;
                if (form == kStripes) t.planes[(r / 4) % 2][k * P * slots * 4 + ((r / 8) * nb + bl) * 4 + r % 4] = x;
            }
            if (form == kSm) t.msk[b * msk_pitch + r] = msk_of(b, r);
            else t.msk[k * P * q8 * 8 + (r / 8 * nb + bl) * 8 + r % 8] = msk_of(b, r);
        }
    }
    RowsIn &a = t.a;
    a.chars = t.chars.get(); a.stride = stride; a.records = t.rec.get(); a.masked = t.msk.get();
    for (size_t p = 0; p < n_bufs; ++p) a.planes[p] = t.planes[p].get();
    a.n_stripes = form == kStripes ? 2u : 1u;
    a.B = (uint32_t)B; a.M = (uint32_t)M; a.D = (uint32_t)D;
    a.layout = (uint32_t)((form == kSm ? HRX_LAYOUT_STRING_MAJOR : HRX_LAYOUT_POSITION_MAJOR) | (in_pm ? HRX_LAYOUT_INPUT_POSITION_MAJOR : 0));
    a.rec_pitch = rec_pitch; a.msk_pitch = msk_pitch;
    return t;
}

// string b through the vector-load addresses and the compile-time single cells
template <int REC>
static void check_place(const RowsIn &a, size_t b, bool in_pm) {
    const RowsPlace s = a.masked ? rows_place<true>(a, (uint32_t)b) : rows_place<false>(a, (uint32_t)b);
    const uint32_t M = a.M, D = a.D;
    for (uint32_t i = 0; i < M; ++i) {
        EXPECT(chr_chunk(s, i)[i & 15u] == chr_of(b, i));
        EXPECT(chr_cell(s, i) == chr_of(b, i));
    }
    if (in_pm)      // the kernels read whole 16-byte chunks there
        for (uint32_t i = 0; i < a.stride; i += 16)
            for (uint32_t j = 0; j < 16; ++j) EXPECT(chr_chunk(s, i)[j] == chr_of(b, i + j));
    for (uint32_t d = 0; d < D; ++d) {
        for (uint32_t r = 0; r < M; ++r) EXPECT(rec_cell<REC>(a, s, r, d) == cell(b, r, d));
        if constexpr (REC != kRecSm) {
            for (uint32_t q = 0; q < (M + 3u) / 4u; ++q) {
                uint32_t x[4];
                memcpy(x, rec_quad<REC>(a, s, q, d), 16);      // (a whole quad is there, rows >= M of the last one unspecified)
                for (uint32_t j = 0; j < 4 && 4 * q + j < M; ++j) EXPECT(x[j] == cell(b, 4 * q + j, d));
            }
        }
    }
    if (!a.masked) {
        EXPECT(s.msk == nullptr);
        return;
    }
    for (uint32_t r = 0; r < M; ++r) EXPECT(msk_cell<REC != kRecSm>(s, r) == msk_of(b, r));
    if constexpr (REC != kRecSm) {
        for (uint32_t o = 0; o < (M + 7u) / 8u; ++o) {
            uint16_t x[8];
            memcpy(x, msk_octet(s, o), 16);
            for (uint32_t j = 0; j < 8 && 8 * o + j < M; ++j) EXPECT(x[j] == msk_of(b, 8 * o + j));
        }
    }
}

static void check(const Batch &t, const char *what) {
    const int before = failures;
    const size_t B = t.a.B;
    const bool in_pm = (t.a.layout & HRX_LAYOUT_INPUT_POSITION_MAJOR) != 0;
    for (int with_masked = 1; with_masked >= 0; --with_masked) {
        RowsIn a = t.a;
        if (!with_masked) { a.masked = nullptr; a.msk_pitch = 0; }
        for (size_t b : {(size_t)0, (size_t)1, (size_t)65535, (size_t)65536, B - 1}) {
            if (b >= B) continue;
            with_rows_form(a, [&](auto form) {          // the form taken at run time, once: what the host readers walk over
                const RowsOf<decltype(form)::value> src(a, b);
                for (uint32_t r = 0; r < a.M; ++r) {
                    EXPECT(src.chr(r) == chr_of(b, r));
                    for (uint32_t d = 0; d < a.D; ++d) EXPECT(src.rec(r, d) == cell(b, r, d));
                    if (with_masked) EXPECT(src.msk(r) == msk_of(b, r));
                }
            });
            switch (rows_form(a)) {
                case kRecSm: check_place<kRecSm>(a, b, in_pm); break;
                case kRecPm: check_place<kRecPm>(a, b, in_pm); break;
                default: check_place<kRecPlanes>(a, b, in_pm); break;
            }
        }
    }
    if (failures != before) std::printf("%s: %d cells differ\n", what, failures - before);
}

int main() {
    const size_t B2 = HRX_PM_BLOCK + 300, M = 19;      // a second block of 300 strings; 5 quads, 3 octets
    check(build(kPm, true, B2, M, 2, 32, M, M), "second block, interleaved, position-major input");
    check(build(kPm, false, B2, M, 2, 32, M, M), "second block, interleaved, string-major input");
    check(build(kPlanes, true, B2, M, 3, 32, M, M), "second block, three planes");
    check(build(kStripes, true, B2, M, 1, 32, M, M), "second block, two row stripes (3 and 2 slots)");
    check(build(kSm, false, 70, M, 2, 32, M, M), "string-major, tight");
    check(build(kSm, false, 70, M, 2, 40, M + 5, M + 3), "string-major, pitched");
    check(build(kPm, true, 70, M, 2, 32, M, M), "one block, interleaved");
    // the layouts a reader takes
    for (int layout = -1; layout < 9; ++layout) EXPECT(rows_layout_known(layout) == (layout == 0 || layout == 1 || layout == 3));
    // the split over threads covers [0, count) once, whatever the number of threads
    for (unsigned threads : {0u, 1u, 3u, 16u, 100u}) {
        std::vector<int> hit(1000, 0);
        over_threads(hit.size(), rows_host_threads(threads), [&hit](size_t i0, size_t i1) { for (size_t i = i0; i < i1; ++i) ++hit[i]; });
        size_t bad = 0;
        for (int h : hit) bad += h != 1;
        EXPECT(bad == 0);
    }
    EXPECT(rows_host_threads(0) >= 1 && rows_host_threads(0) <= 16 && rows_host_threads(5) == 5);
    if (failures) {
        std::printf("rows host: %d failures\n", failures);
        return 1;
    }
    std::printf("rows host: ok\n");
    return 0;
}
