// test_permute_host.cpp — csrc/hrx_permute.hpp + csrc/hrx_permute_host.cpp as a program of their own (tests/test_permute_cpu.py builds it with the address and
// undefined-behaviour sanitizers): the host twin against a literal transcription of rules 1 to 7 on random and hand-made counts; counts, table and every
// output are heap blocks of their exact size, so a read or write one element outside is reported.  Prints "permute host: ok".
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_permute_host.cpp"

using namespace hrx;

static int failures = 0;
#define CHECK(cond, ...)                                                                                    \
    do {                                                                                                    \
        if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (++failures > 20) exit(1); } \
    } while (0)

// rules 1 to 7 as the header words them, nothing shared with the twin.  false: the lookup overflows
static bool literal_rule(const std::vector<uint32_t> &m, uint32_t n_rows, std::vector<uint32_t> &A, std::vector<uint32_t> &S) {
    const size_t T = m.size();
    unsigned __int128 sum = 0;                                       // 1
    for (uint32_t v : m) sum += v;
    if (sum > n_rows) return false;                                  // 2
    std::vector<uint64_t> mp(m.begin(), m.end());
    mp[0] += n_rows - (uint64_t)sum;                                 // 3
    A.clear();
    for (size_t t = 0; t < T; ++t)                                   // 4
        for (uint64_t k = 0; k < mp[t]; ++k) A.push_back((uint32_t)t);
    std::vector<uint32_t> fill;                                      // 7: the fill list
    for (size_t t = 0; t < T; ++t)
        if (mp[t] == 0) fill.push_back((uint32_t)t);
    for (size_t k = 0; k < n_rows - T; ++k) fill.push_back(0);
    S.assign(n_rows, 0);
    size_t j = 0;
    for (uint32_t i = 0; i < n_rows; ++i) {
        const bool first = i == 0 || A[i] != A[i - 1];               // 5
        if (first) S[i] = A[i];                                      // 6
        else S[i] = fill[j++];                                       // 7
    }
    return true;
}

struct Heap {          // a block of exactly n elements
    template <class X> static X *make(size_t n, X fill) { X *p = (X *)malloc(n ? n * sizeof(X) : 1); for (size_t i = 0; i < n; ++i) p[i] = fill; return p; }
};

// one call of the twin over b_count strings of a config of `cols` lookups (tables Ts), checked against the literal rule; returns the overflow words' OR
static uint32_t run_case(const std::vector<uint32_t> &Ts, const std::vector<std::vector<uint32_t>> &counts_of, uint32_t n_rows, uint32_t pitch, bool idx, bool cells,
                         bool per_string_table, unsigned threads) {
    const size_t b_count = counts_of.size();
    PermuteArgs a{};
    uint32_t w = 0;
    for (size_t c = 0; c < Ts.size(); ++c) { a.col[c] = PermuteCol{w, Ts[c]}; w += Ts[c]; }
    const uint32_t W = (w + 3u) & ~3u;
    a.ncols = (uint32_t)Ts.size(); a.W = W; a.b_count = (uint32_t)b_count; a.n_rows = n_rows; a.pitch = pitch;
    uint32_t *counts = Heap::make<uint32_t>(b_count * W, 0u);
    for (size_t b = 0; b < b_count; ++b)
        for (size_t k = 0; k < w; ++k) counts[b * W + k] = counts_of[b][k];
    const size_t runs = per_string_table ? b_count : 1, col = b_count * pitch, n = a.ncols * col;
    uint64_t *table = Heap::make<uint64_t>(runs * W * 4u, 0ull);
    for (size_t k = 0; k < runs * W * 4u; ++k) table[k] = 0x9e3779b97f4a7c15ull * (k + 1);
    const uint32_t POISON = 0xa5a5a5a5u;
    const uint64_t POISON64 = 0xa5a5a5a5a5a5a5a5ull;
    uint32_t *a_idx = idx ? Heap::make<uint32_t>(n, POISON) : nullptr, *s_idx = idx ? Heap::make<uint32_t>(n, POISON) : nullptr;
    uint64_t *a_cells = cells ? Heap::make<uint64_t>(n * 4u, POISON64) : nullptr, *s_cells = cells ? Heap::make<uint64_t>(n * 4u, POISON64) : nullptr;
    uint32_t *overflow = Heap::make<uint32_t>(b_count, POISON);
    a.counts = counts; a.a_idx = a_idx; a.s_idx = s_idx; a.table = cells ? table : nullptr; a.table_stride = per_string_table ? 4u * W : 0u;
    a.a_cells = a_cells; a.s_cells = s_cells; a.overflow = overflow;
    permute_host(a, threads);
    uint32_t any = 0;
    std::vector<uint32_t> A, S;
    for (size_t b = 0; b < b_count; ++b) {
        uint32_t want_over = 0;
        for (uint32_t c = 0; c < a.ncols; ++c) {
            const uint32_t off = a.col[c].off, T = Ts[c];
            std::vector<uint32_t> m(counts + b * W + off, counts + b * W + off + T);
            const bool ok = literal_rule(m, n_rows, A, S);
            if (!ok) want_over |= 1u << c;
            const size_t o = ((size_t)c * b_count + b) * pitch;
            const uint64_t *run = table + (per_string_table ? b : 0) * W * 4u;
            for (uint32_t i = 0; i < pitch; ++i) {
                const bool tail = i >= n_rows;
                const uint32_t wa = tail ? POISON : ok ? off + A[i] : kPmOverflow, ws = tail ? POISON : ok ? off + S[i] : kPmOverflow;
                if (idx) CHECK(a_idx[o + i] == wa && s_idx[o + i] == ws, "string %zu lookup %u position %u: (%u, %u), want (%u, %u)", b, c, i, a_idx[o + i], s_idx[o + i], wa, ws);
                if (cells)
                    for (uint32_t l = 0; l < 4; ++l) {
                        const uint64_t ca = tail ? POISON64 : ok ? run[(size_t)wa * 4u + l] : 0ull, cs = tail ? POISON64 : ok ? run[(size_t)ws * 4u + l] : 0ull;
                        CHECK(a_cells[(o + i) * 4u + l] == ca && s_cells[(o + i) * 4u + l] == cs, "string %zu lookup %u position %u limb %u", b, c, i, l);
                    }
            }
        }
        CHECK(overflow[b] == want_over, "string %zu: overflow %x, want %x", b, overflow[b], want_over);
        any |= overflow[b];
    }
    free(counts); free(table); free(a_idx); free(s_idx); free(a_cells); free(s_cells); free(overflow);
    return any;
}

int main() {
    std::mt19937 rng(12345);
    // random cases: T 1 .. 11, n_rows up to T + 11, sparse and clustered counts, sums up to and beyond n_rows
    for (int it = 0; it < 4000; ++it) {
        const uint32_t ncols = 1 + rng() % 3;
        std::vector<uint32_t> Ts(ncols);
        uint32_t T_max = 0, w = 0;
        for (uint32_t &T : Ts) { T = 1 + rng() % 11; T_max = std::max(T_max, T); w += T; }
        const uint32_t n_rows = T_max + rng() % 12, pitch = ((n_rows + 3u) & ~3u) + 4u * (rng() % 2);
        const size_t b_count = 1 + rng() % 3;
        std::vector<std::vector<uint32_t>> counts(b_count, std::vector<uint32_t>(w, 0u));
        for (auto &run : counts) {
            uint32_t off = 0;
            for (uint32_t T : Ts) {
                const uint32_t mode = rng() % 4, total = mode == 3 ? n_rows + rng() % 3 : rng() % (n_rows + 1);
                for (uint32_t k = 0; k < total; ++k) {
                    const uint32_t t = mode == 0 ? rng() % T : mode == 1 ? (rng() % 2 ? T - 1 : rng() % T) : 1 + rng() % T;      // mode 2, 3: row 0 mostly empty
                    ++run[off + (t < T ? t : T - 1)];
                }
                off += T;
            }
        }
        run_case(Ts, counts, n_rows, pitch, it % 3 != 1, it % 3 != 0, it % 2 == 0, 1 + it % 3);
    }
    // the hand-made cases, one lookup of T = 7 beside an untouched one of T = 3
    {
        const uint32_t T = 7, n_rows = 12;
        const std::vector<uint32_t> Ts = {T, 3};
        auto with = [&](std::vector<uint32_t> m) { m.resize(T + 3, 0u); m[T + 1] = 2; return std::vector<std::vector<uint32_t>>{m, m}; };
        CHECK(run_case(Ts, with({0, 0, 0, 0, 0, 0, 0}), n_rows, 12, true, true, true, 2) == 0, "all zero");
        CHECK(run_case(Ts, with({1, 1, 1, 1, 1, 1, 1}), T, 8, true, true, false, 1) == 0, "every row once, n_rows == T");
        CHECK(run_case(Ts, with({0, 0, 0, n_rows, 0, 0, 0}), n_rows, 16, true, true, true, 1) == 0, "one row holds n_rows");
        CHECK(run_case(Ts, with({0, 5, 0, 3, 0, 0, 4}), n_rows, 12, true, true, true, 1) == 0, "sum == n_rows with m[0] == 0");
        CHECK(run_case(Ts, with({0, 5, 0, 3, 0, 1, 4}), n_rows, 12, true, true, true, 1) == 1, "sum == n_rows + 1: overflow of lookup 0 only");
        CHECK(run_case(Ts, with({0, 0xffffffffu, 0, 0, 0xffffffffu, 2, 0}), n_rows, 12, true, true, false, 1) == 1, "two words of 0xffffffff: overflow, no wrapped sum");
        CHECK(run_case(Ts, with({0xffffffffu, 0, 0, 0, 0, 0, 1}), n_rows, 12, true, false, false, 1) == 1, "a sum of 2^32: overflow, not 0");
    }
    // a table longer than one of the kernel's chunks, uniform and clustered
    {
        const uint32_t T = kPmChunkRows + 77;
        std::vector<uint32_t> m(T, 0u);
        for (uint32_t t = 0; t < T; t += 3) m[t] = 1;
        run_case({T}, {m}, T + 5, (T + 5 + 3) & ~3u, true, true, false, 1);
        std::vector<uint32_t> m2(T, 0u);
        m2[T - 1] = T;
        run_case({T}, {m2}, T + 1, (T + 1 + 3) & ~3u, true, false, false, 1);
    }
    // the plan: whole tiles per workgroup, every position covered, a workspace only beyond one chunk
    for (size_t n_rows : {1u, 1023u, 1024u, 1025u, 4090u, 65537u})
        for (size_t b_count : {1u, 3u, 100u, 5000u}) {
            const PermutePlan p = plan_permute(2843, 2852, 3, b_count, n_rows, 256);
            CHECK(p.group_rows % kPmTileRows == 0 && (size_t)p.group_rows * p.groups >= n_rows && (size_t)p.group_rows * (p.groups - 1) < n_rows && p.workspace_bytes == 0,
                  "plan %zu x %zu", b_count, n_rows);
            const PermutePlan q = plan_permute(kPmChunkRows + 1, 4000, 3, b_count, 8000, 256);
            CHECK(q.groups == 1 && q.group_rows >= 8000 && q.workspace_bytes == b_count * 4000 * 4, "plan beyond a chunk");
        }
    if (failures) return 1;
    printf("permute host: ok\n");
    return 0;
}
