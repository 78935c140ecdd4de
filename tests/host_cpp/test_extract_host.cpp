// test_extract_host.cpp — csrc/hrx_extract.hpp and csrc/hrx_extract_host.cpp (the host form of EXTRACT, include/hrx.h) as a program of their own, built with
// -fsanitize=address,undefined by tests/test_extract_cpu.py.  Every output array is a heap block of exactly its cap, so one element too far is a
// sanitizer error: short caps (the stored runs are a prefix, totals and run_offsets complete), runs clipped to their slot / ragged string, decreasing
// offsets, the threaded copy.  The expectation is computed here, run by run, from the rule's text — not by the code under test.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_extract_host.cpp"

using namespace hrx;

static int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #c);               \
            ++failures;                                               \
        }                                                             \
    } while (0)

static uint64_t word(uint64_t start, uint64_t len, uint64_t id) { return start | len << 28 | id << 56; }

struct Case {
    int layout;
    std::vector<uint8_t> src;
    uint64_t stride;
    std::vector<uint64_t> offsets, status, spans;
    std::vector<uint32_t> counts;
    uint64_t max_spans;
    uint32_t require;
    uint64_t B() const { return status.size(); }
};

struct Want {
    std::vector<uint64_t> run_offsets, runs, byte_offsets;
    std::vector<uint8_t> values;
    uint64_t truncated = 0;
};

// the rule as include/hrx.h words it
static Want expect(const Case &c) {
    Want w;
    w.byte_offsets.push_back(0);
    for (uint64_t b = 0; b < c.B(); ++b) {
        w.run_offsets.push_back(w.runs.size());
        uint64_t limit = c.stride, base = b * c.stride;
        if (c.layout == kExtractLayoutRagged) {
            if (c.offsets[b + 1] < c.offsets[b]) continue;
            limit = c.offsets[b + 1] - c.offsets[b];
            base = c.offsets[b];
        }
        if ((c.status[b] & 0xff) || (((c.status[b] >> 8) & c.require) != c.require)) continue;
        uint64_t k = c.counts[b];
        if (k > c.max_spans) { k = c.max_spans; ++w.truncated; }
        for (uint64_t i = 0; i < k; ++i) {
            const uint64_t sw = c.spans[b * c.max_spans + i];
            uint64_t s = sw & 0xfffffff, n = (sw >> 28) & 0xfffffff;
            if (s > limit) s = limit;
            if (n > limit - s) n = limit - s;
            w.runs.push_back(sw);
            for (uint64_t x = 0; x < n; ++x) w.values.push_back(c.src[base + s + x]);
            w.byte_offsets.push_back(w.values.size());
        }
    }
    w.run_offsets.push_back(w.runs.size());
    return w;
}

static void run_case(const Case &c, uint64_t runs_cap, uint64_t values_cap, int threads) {
    const Want w = expect(c);
    const uint64_t B = c.B();
    // exactly sized heap blocks (new[]: no slack the sanitizer would not see)
    std::unique_ptr<uint64_t[]> ro(new uint64_t[B + 1]), runs(new uint64_t[runs_cap ? runs_cap : 1]), bo(new uint64_t[runs_cap + 1]), tot(new uint64_t[4]);
    std::unique_ptr<uint8_t[]> vals(new uint8_t[values_cap ? values_cap : 1]);
    for (uint64_t j = 0; j <= runs_cap; ++j) bo[j] = ~0ull;
    for (uint64_t j = 0; j < runs_cap; ++j) runs[j] = ~0ull;
    for (uint64_t j = 0; j < values_cap; ++j) vals[j] = 0xEE;
    ExtractIn in{};
    in.layout = c.layout; in.src = c.src.data(); in.stride = c.stride; in.offsets = c.offsets.data(); in.B = B;
    in.status = c.status.data(); in.span_counts = c.counts.data(); in.spans = c.spans.data(); in.max_spans = c.max_spans; in.require_accept = c.require;
    const hrx_extract_out out{ro.get(), runs_cap ? runs.get() : nullptr, bo.get(), values_cap ? vals.get() : nullptr, tot.get(), (size_t)runs_cap, (size_t)values_cap};
    extract_host(in, out, threads);
    EXPECT(tot[0] == w.runs.size() && tot[1] == w.values.size() && tot[2] == w.truncated && tot[3] == 0);
    for (uint64_t b = 0; b <= B; ++b) EXPECT(ro[b] == w.run_offsets[b]);
    uint64_t J = 0;
    while (J < w.runs.size() && J < runs_cap && w.byte_offsets[J + 1] <= values_cap) ++J;
    for (uint64_t j = 0; j < J; ++j) EXPECT(runs[j] == w.runs[j]);
    for (uint64_t j = 0; j <= J; ++j) EXPECT(bo[j] == w.byte_offsets[j]);
    for (uint64_t x = 0; x < w.byte_offsets[J]; ++x) EXPECT(vals[x] == w.values[x]);
    for (uint64_t j = J; j < runs_cap; ++j) EXPECT(runs[j] == ~0ull);
    for (uint64_t j = J + 1; j <= runs_cap; ++j) EXPECT(bo[j] == ~0ull);
    for (uint64_t x = w.byte_offsets[J]; x < values_cap; ++x) EXPECT(vals[x] == 0xEE);
}

static void sweep(const Case &c) {
    const Want w = expect(c);
    const uint64_t R = w.runs.size(), nb = w.values.size();
    for (int threads : {1, 3}) {
        run_case(c, R, nb, threads);
        run_case(c, R + 5, nb + 7, threads);
        for (uint64_t rc = 0; rc <= R; ++rc) run_case(c, rc, nb, threads);
        for (uint64_t vc = 0; vc <= nb; ++vc) run_case(c, R, vc, threads);      // every values_cap: those inside a run too
        run_case(c, R / 2, nb / 3, threads);
        run_case(c, 0, 0, threads);
    }
}

int main() {
    // string-major: 9 strings of 24 bytes; bad status, unaccepted, truncated, a run leaving the slot, one starting past it, an empty one, the whole slot
    Case sm;
    sm.layout = kExtractLayoutStringMajor; sm.stride = 24; sm.max_spans = 3; sm.require = 0;
    for (int i = 0; i < 9 * 24; ++i) sm.src.push_back((uint8_t)(i * 7 + 1));
    sm.status = {1u << 8, 3, 0, 3u << 8, 1u << 8, 2u << 8, 1u << 8, 1u << 8, 1u << 8};
    sm.counts = {2, 2, 1, 5, 0, 3, 1, 1, 1};
    sm.spans = {word(0, 4, 1), word(6, 2, 2), 0,
                word(1, 1, 1), word(3, 1, 1), 0,
                word(20, 9, 1), 0, 0,
                word(2, 2, 1), word(4, 1, 2), word(5, 19, 1),
                0, 0, 0,
                word(23, 1, 1), word(24, 4, 2), word(0, 0, 3),
                word(0, 24, 1), 0, 0,
                word(100, 100, 1), 0, 0,
                word(0, (1u << 28) - 1, 2), 0, 0};
    sweep(sm);
    sm.require = 1;
    sweep(sm);
    sm.require = 3;
    sweep(sm);
    // ragged: lengths 10, 0, decreasing, 7, 1 after a lead of 3
    Case rg;
    rg.layout = kExtractLayoutRagged; rg.stride = 0; rg.max_spans = 2; rg.require = 0;
    for (int i = 0; i < 40; ++i) rg.src.push_back((uint8_t)(200 - i));
    rg.offsets = {3, 13, 13, 9, 16, 17};
    rg.status = {1u << 8, 1u << 8, 1u << 8, 1u << 8, 1u << 8};
    rg.counts = {2, 1, 1, 4, 1};
    rg.spans = {word(8, 5, 1), word(2, 2, 3), word(0, 1, 1), 0, word(0, 4, 1), 0, word(5, 100, 1), word(6, 1, 2), word(0, 1, 9), 0};
    sweep(rg);
    // a batch large enough for the threaded copy to cut it
    Case big;
    big.layout = kExtractLayoutStringMajor; big.stride = 16; big.max_spans = 2; big.require = 0;
    for (uint64_t b = 0; b < 300; ++b) {
        for (int i = 0; i < 16; ++i) big.src.push_back((uint8_t)(b * 16 + i));
        big.status.push_back(b % 11 == 0 ? 2 : 1u << 8);
        big.counts.push_back((uint32_t)(b % 4));
        big.spans.push_back(word(b % 16, 1 + b % 5, 1));
        big.spans.push_back(word((b + 7) % 16, b % 3, 2));
    }
    const Want w = expect(big);
    for (int threads : {1, 2, 7, 64}) {
        run_case(big, w.runs.size(), w.values.size(), threads);
        run_case(big, w.runs.size() / 2, w.values.size(), threads);
        run_case(big, w.runs.size(), w.values.size() / 2 + 1, threads);
    }
    // an empty batch
    Case none;
    none.layout = kExtractLayoutRagged; none.stride = 0; none.max_spans = 1; none.require = 0;
    none.offsets = {0};
    run_case(none, 0, 0, 1);
    run_case(none, 4, 4, 2);
    if (failures) {
        std::printf("extract host: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("extract host: ok\n");
    return 0;
}
