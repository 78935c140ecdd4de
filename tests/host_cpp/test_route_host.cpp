// test_route_host.cpp — csrc/hrx_route.hpp and csrc/hrx_route_host.cpp (the host form of ROUTE, include/hrx.h) as a program of their own, built with
// -fsanitize=address,undefined by tests/test_route_cpu.py.  Every input and output array is a heap block of exactly its size, so one element too far is a
// sanitizer error: lens [B], offsets [B + 1], status [B], order [B], bucket_offsets [n_buckets + 2].  The expectation is computed here, bin by bin, from the
// rule's text — not by the code under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_route_host.cpp"

using namespace hrx;

static int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #c);               \
            ++failures;                                               \
        }                                                             \
    } while (0)

struct Case {
    bool screened;
    std::vector<uint64_t> status;
    uint32_t require;
    bool ragged;
    std::vector<uint32_t> lens;         // padded form
    std::vector<uint64_t> offsets;      // ragged form
    std::vector<uint32_t> bounds;
    uint64_t B() const { return ragged ? offsets.size() - 1 : lens.size(); }
};

// the rule as include/hrx.h words it: per range, the strings that belong to it in increasing b
static void expect(const Case &c, std::vector<uint32_t> &order, std::vector<uint64_t> &bo) {
    const size_t nb = c.bounds.size();
    for (size_t j = 0; j <= nb; ++j) {
        bo.push_back(order.size());
        for (uint64_t b = 0; b < c.B(); ++b) {
            bool kept = !c.screened || ((c.status[b] & 0xff) == 0 && ((c.status[b] >> 8) & c.require) == c.require);
            uint64_t n = 0;
            if (c.ragged) {
                if (c.offsets[b + 1] < c.offsets[b]) kept = false;
                else n = c.offsets[b + 1] - c.offsets[b];
            } else {
                n = c.lens[b];
            }
            if (n > c.bounds[nb - 1]) kept = false;
            size_t bucket = nb;
            if (kept)
                for (bucket = 0; n > c.bounds[bucket]; ++bucket) {}
            if (bucket == j) order.push_back((uint32_t)b);
        }
    }
    bo.push_back(order.size());
}

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T> &v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

static void run_case(const Case &c) {
    std::vector<uint32_t> want_order;
    std::vector<uint64_t> want_bo;
    expect(c, want_order, want_bo);
    const uint64_t B = c.B();
    const size_t nb = c.bounds.size();
    EXPECT(route_bounds_valid(c.bounds.data(), nb));
    // exactly sized heap blocks (new[]: no slack the sanitizer would not see)
    auto status = exact(c.status);
    auto lens = exact(c.lens);
    auto offsets = exact(c.offsets);
    std::unique_ptr<uint32_t[]> order(new uint32_t[B ? B : 1]);
    std::unique_ptr<uint64_t[]> bo(new uint64_t[nb + 2]);
    RouteIn in{};
    in.status = c.screened ? status.get() : nullptr;
    in.require_accept = c.require;
    in.lens = c.ragged ? nullptr : lens.get();
    in.offsets = c.ragged ? offsets.get() : nullptr;
    in.B = B;
    in.bounds.n = (uint32_t)nb;
    for (size_t j = 0; j < nb; ++j) in.bounds.v[j] = c.bounds[j];
    route_host(in, order.get(), bo.get());
    for (size_t j = 0; j < nb + 2; ++j) EXPECT(bo[j] == want_bo[j]);
    for (uint64_t k = 0; k < B; ++k) EXPECT(order[k] == want_order[k]);
    EXPECT(bo[0] == 0 && bo[nb + 1] == B);
}

int main() {
    // the predicates on their own
    EXPECT(passes_screen(0, 0) && passes_screen(3u << 8, 1) && passes_screen(3u << 8, 3) && !passes_screen(1u << 8, 3) && !passes_screen(2u << 8, 1));
    EXPECT(!passes_screen(1, 0) && !passes_screen(3 | 3u << 8, 0) && !passes_screen(0, 1));
    {
        const RouteBounds bd{3, {16, 64, 256}};
        EXPECT(bucket_of(bd, 0) == 0 && bucket_of(bd, 16) == 0 && bucket_of(bd, 17) == 1 && bucket_of(bd, 64) == 1 && bucket_of(bd, 65) == 2);
        EXPECT(bucket_of(bd, 256) == 2 && bucket_of(bd, 257) == 3 && bucket_of(bd, ~0ull) == 3);
        const RouteBounds one{1, {1u << 24}};
        EXPECT(bucket_of(one, 1u << 24) == 0 && bucket_of(one, (1u << 24) + 1) == 1);
    }
    {
        const uint32_t ok8[8] = {1, 2, 3, 4, 5, 6, 7, 1u << 24}, eq[2] = {16, 16}, down[2] = {64, 16}, big[1] = {(1u << 24) + 1}, nine[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
        EXPECT(route_bounds_valid(ok8, 8) && !route_bounds_valid(ok8, 0) && !route_bounds_valid(nine, 9) && !route_bounds_valid(eq, 2));
        EXPECT(!route_bounds_valid(down, 2) && !route_bounds_valid(big, 1) && !route_bounds_valid(nullptr, 1));
    }
    // padded lengths: every status kind, lengths on both sides of every bound
    Case pd;
    pd.screened = true; pd.ragged = false; pd.require = 0;
    const uint32_t edge[] = {0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 0xffffffffu};
    for (int rep = 0; rep < 5; ++rep)
        for (uint32_t n : edge) {
            pd.lens.push_back(n);
            const uint64_t kinds[] = {0, 1u << 8, 2u << 8, 3u << 8, 1, 2 | 1u << 8, 3};
            pd.status.push_back(kinds[(pd.lens.size() * 5 + rep) % 7]);
        }
    const std::vector<std::vector<uint32_t>> all_bounds = {{256}, {16, 64, 256}, {1, 15, 16, 17, 63, 64, 65, 256}, {16, 64}, {1}, {1u << 24}};
    for (uint32_t require : {0u, 1u, 2u, 3u})
        for (const auto &bd : all_bounds) {
            pd.require = require; pd.bounds = bd;
            pd.screened = true;
            run_case(pd);
            pd.screened = false;
            run_case(pd);
        }
    // ragged: a lead of 3, empty strings, decreasing pairs (the first and the last string among them)
    Case rg;
    rg.screened = true; rg.ragged = true; rg.require = 1;
    rg.offsets = {9, 3, 13, 13, 9, 16, 17, 81, 82, 338, 400, 399};
    for (size_t b = 0; b + 1 < rg.offsets.size(); ++b) rg.status.push_back(b % 4 == 3 ? 2 : 1u << 8);
    for (const auto &bd : all_bounds) {
        rg.bounds = bd;
        rg.screened = true;
        run_case(rg);
        rg.screened = false;
        run_case(rg);
    }
    // an empty batch and a batch of one
    Case none;
    none.screened = false; none.ragged = true; none.require = 0; none.offsets = {5}; none.bounds = {16, 64};
    run_case(none);
    Case single;
    single.screened = true; single.ragged = false; single.require = 0; single.lens = {16}; single.status = {0}; single.bounds = {16, 64};
    run_case(single);
    if (failures) {
        std::printf("route host: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("route host: ok\n");
    return 0;
}
