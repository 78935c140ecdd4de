// test_verify_chunk_host.cpp — the chunked rule of csrc/hrx_verify.hpp (verify_chunk_string / verify_chunk_lane, verify_fold_chunk) and its host form
// (verify_rows_chunked_host of csrc/hrx_verify_host.cpp) as a program of their own, built with -fsanitize=address,undefined by
// tests/test_verify_chunked_cpu.py.  The yardstick is verify_string — the unchunked rule — never the chunked code: for every string below and every
// chunk_rows in 32, 64, 96, ... up to beyond M, the fold of the chunks' summaries must be verify_string's word, bit for bit, from the accessor walk and from
// the kernel's tile walk in every instantiation the kernel uses.  The summaries live in a heap block of exactly hrx_verify_chunked_workspace_bytes, laid
// out as the kernel lays them out, so one summary too far is a sanitizer error.  The hand-made defs, make_rows and the exact-size blocks are
// test_verify_host.cpp's (included with its main renamed).
#define main test_verify_host_main
#include "test_verify_host.cpp"
#undef main

static const uint32_t kMs[] = {33u, 64u, 65u, 139u, 264u};

// the fold of one string's chunks, summaries through a workspace of exactly the stated size; Walk(k, r0, r1) -> VerifyChunk
template <class Walk>
static uint64_t fold_of(const Rows &R, uint32_t C, const Walk &walk) {
    if (R.n > R.M) return ~0ull;
    const size_t bytes = verify_chunked_workspace_bytes(1, R.M, C);
    const uint32_t K = verify_chunk_count(R.M, C);
    EXPECT(bytes == (size_t)32 * K);
    std::unique_ptr<uint32_t[]> ws(new uint32_t[bytes / 4]);
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t r0 = k * C, r1 = std::min(R.M, r0 + C);
        const VerifyChunk v = walk(r0, r1);
        const uint32_t w[kVfyChunkFields] = {v.flags, v.row, v.mask_row[0], v.mask_row[1], v.need1[0], v.need1[1], v.need0[0], v.need0[1]};
        for (uint32_t f = 0; f < kVfyChunkFields; ++f) ws[(size_t)f * K + k] = w[f];
    }
    VerifyAcc acc;
    verify_begin(acc);
    for (uint32_t k = 0; k < K; ++k) {
        uint32_t w[kVfyChunkFields];
        for (uint32_t f = 0; f < kVfyChunkFields; ++f) w[f] = ws[(size_t)f * K + k];
        verify_fold_chunk(acc, VerifyChunk{w[0], w[1], {w[2], w[3]}, {w[4], w[5]}, {w[6], w[7]}});
    }
    return verify_finish(acc);
}

static size_t checked = 0;

// every chunk size against verify_string, through every walk
static uint64_t check_all_chunkings(const std::vector<uint32_t> &image, const Rows &R, const char *what) {
    const std::unique_ptr<uint32_t[]> img = exact(image);
    const OneString s(R);
    const uint64_t want = verify_string(img.get(), R.D, R.n, R.M, s);
    for (uint32_t C = 32; C <= R.M + 64; C += 32) {
        const uint32_t *im = img.get();
        uint64_t got[6];
        int m = 0;
        got[m++] = fold_of(R, C, [&](uint32_t r0, uint32_t r1) { return verify_chunk_string(im, R.D, R.n, R.M, r0, r1, s); });
        got[m++] = fold_of(R, C, [&](uint32_t r0, uint32_t r1) { return verify_chunk_lane<0, 8>(im, R.D, R.n, R.M, r0, r1, SrcTiles<8>{s, R.n, R.M}); });
        if (R.D == 1) got[m++] = fold_of(R, C, [&](uint32_t r0, uint32_t r1) { return verify_chunk_lane<1, 32>(im, R.D, R.n, R.M, r0, r1, SrcTiles<32>{s, R.n, R.M}); });
        if (R.D == 2) got[m++] = fold_of(R, C, [&](uint32_t r0, uint32_t r1) { return verify_chunk_lane<2, 16>(im, R.D, R.n, R.M, r0, r1, SrcTiles<16>{s, R.n, R.M}); });
        if (R.D == 3) got[m++] = fold_of(R, C, [&](uint32_t r0, uint32_t r1) { return verify_chunk_lane<3, 16>(im, R.D, R.n, R.M, r0, r1, SrcTiles<16>{s, R.n, R.M}); });
        if (R.D == 4) got[m++] = fold_of(R, C, [&](uint32_t r0, uint32_t r1) { return verify_chunk_lane<4, 8>(im, R.D, R.n, R.M, r0, r1, SrcTiles<8>{s, R.n, R.M}); });
        for (int i = 0; i < m; ++i) {
            if (got[i] != want)
                std::printf("%s: M %u n %u D %u chunk_rows %u walk %d: %llx, verify_string %llx\n", what, R.M, R.n, R.D, C, i, (unsigned long long)got[i],
                            (unsigned long long)want);
            EXPECT(got[i] == want);
            ++checked;
        }
    }
    return want;
}

// a^i b^j a^k: def 1 reveals the run of b — a forward set at row i (the start flag), a backward set at row i + j - 1 (the end flags of the run land on
// EN[i + 1 .. i + j]; the tag changes behind row i + j - 1) — def 2 reveals row 0 where the string begins with a.  i and i + j walk over both sides of every
// border of a 32-row chunk: each kind of event at the first and the last row of a chunk and on each side of a border; a run that spans one, two, three borders
static void events_at_borders(const std::vector<Def> &defs) {
    const std::vector<uint32_t> img = image_of(defs);
    for (uint32_t M : kMs) {
        std::vector<uint32_t> pos;
        for (uint32_t b = 32; b < M + 2 && b <= 128; b += 32)
            for (uint32_t p : {b - 2, b - 1, b, b + 1})
                if (p + 2 <= M) pos.push_back(p);
        pos.push_back(0);
        for (uint32_t i : pos)
            for (uint32_t e : pos) {            // the run of b is rows i .. e - 1
                if (e <= i) continue;
                const uint32_t tail = std::min(M - e, 3u);
                const Rows clean = make_rows(defs, abba(i, e - i, tail), M);
                const uint64_t v = check_all_chunkings(img, clean, "events clean");
                EXPECT(v == (clean.n == M || clean.accepted_all ? 0 : (uint64_t)kVfyAccept | (uint64_t)clean.n << 32));
                // a revealed cell blanked at the run's first, middle and last row; a cell revealed before and behind the run; the wrong byte inside
                for (uint32_t r : {i, (i + e) / 2, e - 1}) {
                    Rows R = clean;
                    R.msk[r] = 0;
                    const uint64_t w = check_all_chunkings(img, R, "events blanked");
                    EXPECT((bits_of(w) & kVfyMask) && row_of(w) <= r);
                }
                for (uint32_t r : {i ? i - 1 : M - 1, e < M ? e : M - 1}) {
                    if (r >= i && r < e) continue;
                    Rows R = clean;
                    R.msk[r] = 'b' | 1 << 8;
                    const uint64_t w = check_all_chunkings(img, R, "events revealed outside");
                    EXPECT((bits_of(w) & kVfyMask) && row_of(w) <= r);
                }
                // the end flags dropped: the run is never confirmed (no backward set; the rows pend to the end of the rows), the flag check fails too
                Rows R = clean;
                for (uint32_t r = i; r < e; ++r) R.rec[(size_t)r * R.D] &= ~(1u << 25);
                check_all_chunkings(img, R, "events unconfirmed");
                // the start flag dropped: no forward set, every revealed cell of the run is wrong
                R = clean;
                R.rec[(size_t)i * R.D] &= ~(1u << 24);
                check_all_chunkings(img, R, "events no start");
            }
    }
}

// a string with no event at all (no tagged row), clean and with one cell filled in; n = 0 and n = M; n at a border and at border +- 1
static void lengths_and_no_events(const std::vector<Def> &defs) {
    const std::vector<uint32_t> img = image_of(defs);
    for (uint32_t M : kMs) {
        std::vector<uint32_t> ns = {0u, 1u, M - 1, M};
        for (uint32_t b = 32; b < M; b += 32)
            for (uint32_t n : {b - 1, b, b + 1})
                if (n <= M) ns.push_back(n);
        for (uint32_t n : ns) {
            const Rows plain = make_rows(defs, std::string(n, 'a'), M);         // all a: def 1 tags nothing
            check_all_chunkings(img, plain, "no event");
            for (uint32_t r : {0u, 31u, 32u, M - 1}) {
                Rows R = plain;
                R.msk[r] = 'a' | 1 << 8;
                const uint64_t w = check_all_chunkings(img, R, "no event, one cell");
                EXPECT(bits_of(w) & kVfyMask);
            }
            const Rows runs = make_rows(defs, abba(n / 3, n / 3, n - 2 * (n / 3)), M);
            check_all_chunkings(img, runs, "lengths");
            // the accept chain's row n, the padding behind it and the state of row n tampered: def checks at and beside the border
            for (uint32_t r : {n, n + 1 < M ? n + 1 : n, n ? n - 1 : 0u}) {
                if (r >= M) continue;
                Rows R = runs;
                R.rec[(size_t)r * R.D] ^= 1u;
                check_all_chunkings(img, R, "lengths, state moved");
                R = runs;
                R.rec[(size_t)r * R.D + (R.D - 1)] |= 1u << 16;
                check_all_chunkings(img, R, "lengths, tag set");
            }
        }
        Rows R = make_rows(defs, "ab", M);
        R.n = M + 1;                                                        // no rows
        EXPECT(fold_of(R, 32, [&](uint32_t, uint32_t) { EXPECT(false); return VerifyChunk{}; }) == ~0ull);
    }
}

// an overlap row (two defs flag one row: the masked rows are not reported) in a chunk other than the one whose mask is wrong, either order
static void overlap_elsewhere() {
    const std::vector<Def> defs = {kDef1, kDef2};
    const std::vector<uint32_t> img = image_of(defs);
    for (uint32_t M : kMs) {
        if (M < 100) continue;
        const Rows clean = make_rows(defs, abba(40, 30, 20), M);
        for (uint32_t bad : {5u, 45u, 69u, 98u})
            for (uint32_t ov : {0u, 33u, 64u, 97u}) {
                Rows R = clean;
                R.msk[bad] ^= 0x0101;
                uint64_t w = check_all_chunkings(img, R, "mask wrong");
                EXPECT(bits_of(w) & kVfyMask);
                R.rec[(size_t)ov * 2] |= 1u << 24;
                R.rec[(size_t)ov * 2 + 1] |= 1u << 24;                     // both defs flag row ov
                w = check_all_chunkings(img, R, "overlap elsewhere");
                EXPECT(!(bits_of(w) & kVfyMask) && w != 0);
            }
    }
}

// every def count's instantiation: one cell of every kind changed at the rows around each border
static void one_cell_changes(const std::vector<Def> &defs) {
    const std::vector<uint32_t> img = image_of(defs);
    const uint32_t D = (uint32_t)defs.size();
    for (uint32_t M : {65u, 139u}) {
        const Rows clean = make_rows(defs, M == 65 ? abba(20, 30, 10) : abba(30, 36, 20), M);
        check_all_chunkings(img, clean, "cells clean");
        for (uint32_t r : {0u, 30u, 31u, 32u, 33u, 63u, 64u, 65u, 66u, 85u, 86u, 95u, 96u, 97u, 127u, 128u, 129u, M - 1}) {
            if (r >= M) continue;
            for (uint32_t d = 0; d < D; ++d)
                for (uint32_t flip : {1u, 1u << 16, 1u << 24, 1u << 25, 1u << 26}) {
                    Rows R = clean;
                    R.rec[(size_t)r * D + d] ^= flip;
                    check_all_chunkings(img, R, "cells rec");
                }
            Rows R = clean;
            R.msk[r] ^= 0x0101;
            check_all_chunkings(img, R, "cells msk");
        }
    }
}

// verify_rows_chunked_host against verify_rows_host: threads over (string, chunk) pairs, every image of the rows, a string with no rows among them
static void host_form(const std::vector<Def> &defs, uint32_t M, size_t B) {
    const std::vector<uint32_t> image = image_of(defs);
    const std::unique_ptr<uint32_t[]> img = exact(image);
    const uint32_t D = (uint32_t)defs.size();
    const size_t stride = ((size_t)M + 15) / 16 * 16, q4 = ((size_t)M + 3) / 4, q8 = ((size_t)M + 7) / 8;
    std::vector<uint32_t> lens(B);
    std::vector<uint8_t> c_sm(B * stride, 0);
    std::vector<uint32_t> r_sm(B * M * D), r_pm(q4 * 4 * D * B, 0xdeadbeefu);
    std::vector<uint16_t> m_sm(B * M), m_pm(q8 * 8 * B, 0xdead);
    for (size_t b = 0; b < B; ++b) {
        const uint32_t n = b % 5 == 0 ? 0 : b % 5 == 1 ? M : (uint32_t)((b * 7) % (M + 1));
        Rows R = make_rows(defs, abba(n / 4, n / 2, n - n / 4 - n / 2), M);
        if (b % 3 == 2) R.msk[(b * 11) % M] ^= 0x0101;
        lens[b] = b == 4 ? M + 1 : n;
        for (uint32_t i = 0; i < n; ++i) c_sm[b * stride + i] = R.chars[i];
        for (uint32_t r = 0; r < M; ++r) {
            for (uint32_t d = 0; d < D; ++d) {
                r_sm[(b * M + r) * D + d] = R.rec[(size_t)r * D + d];
                r_pm[((r / 4 * D + d) * B + b) * 4 + r % 4] = R.rec[(size_t)r * D + d];
            }
            m_sm[b * M + r] = R.msk[r];
            m_pm[(r / 8 * B + b) * 8 + r % 8] = R.msk[r];
        }
    }
    const auto lens_x = exact(lens);
    const auto c_x = exact(c_sm);
    const auto r_sm_x = exact(r_sm), r_pm_x = exact(r_pm);
    const auto m_sm_x = exact(m_sm), m_pm_x = exact(m_pm);
    for (int form = 0; form < 2; ++form) {
        std::unique_ptr<uint64_t[]> want(new uint64_t[B]);
        VerifyArgs a{};
        a.lens = lens_x.get(); a.stride = stride; a.B = (uint32_t)B; a.M = M; a.D = D; a.image = img.get(); a.verdict = want.get();
        a.rec_pitch = a.msk_pitch = M; a.chars = c_x.get();
        if (form == 0) { a.layout = 0; a.records = r_sm_x.get(); a.masked = m_sm_x.get(); }
        if (form == 1) { a.layout = 1; a.records = r_pm_x.get(); a.masked = m_pm_x.get(); }
        verify_rows_host(a, 1u);
        EXPECT(want[4] == ~0ull);
        for (uint32_t C : {32u, 64u, 96u, (M + 31) / 32 * 32}) {
            std::unique_ptr<uint64_t[]> out(new uint64_t[B]);
            for (size_t b = 0; b < B; ++b) out[b] = 0x5555555555555555ull;
            const size_t bytes = verify_chunked_workspace_bytes(B, M, C);
            EXPECT(bytes == 32 * (size_t)verify_chunk_count(M, C) * B);
            std::unique_ptr<uint32_t[]> ws(new uint32_t[bytes / 4]);
            a.verdict = out.get();
            verify_rows_chunked_host(a, C, ws.get(), C == 32 ? 1u : 5u);
            size_t bad = 0;
            for (size_t b = 0; b < B; ++b) bad += out[b] != want[b];
            if (bad) std::printf("host form: M %u B %zu D %u form %d chunk_rows %u: %zu words differ\n", M, B, D, form, C, bad);
            EXPECT(bad == 0);
        }
    }
}

int main() {
    const std::vector<Def> one = {kDef1}, two = {kDef1, kDef2}, three = {kDef1, kDef2, kDef3}, four = {kDef3, kDef1, kDef3, kDef2},
                           five = {kDef1, kDef3, kDef2, kDef3, kDef3};
    EXPECT(verify_chunked_workspace_bytes(3, 100, 0) == 0 && verify_chunked_workspace_bytes(3, 100, 48) == 0 && verify_chunked_workspace_bytes(3, 0, 32) == 0);
    EXPECT(verify_chunked_workspace_bytes(3, 100, 32) == 32u * 4 * 3 && verify_chunked_workspace_bytes(3, 100, 128) == 32u * 3 &&
           verify_chunked_workspace_bytes(3, 96, 32) == 32u * 3 * 3);
    events_at_borders(one);
    events_at_borders(two);
    for (const auto *defs : {&one, &two, &three, &four, &five}) lengths_and_no_events(*defs);
    overlap_elsewhere();
    for (const auto *defs : {&one, &two, &three, &four, &five}) one_cell_changes(*defs);
    for (uint32_t M : {33u, 139u}) {
        host_form(one, M, 11);
        host_form(three, M, 70);
        host_form(five, M, 7);
    }
    if (failures) {
        std::printf("verify chunk host: %d failures\n", failures);
        return 1;
    }
    std::printf("verify chunk host: ok (%zu folds)\n", checked);
    return 0;
}
