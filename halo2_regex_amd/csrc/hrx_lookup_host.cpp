// hrx_lookup_host.cpp — the host form of LOOKUP COUNTS (include/hrx.h hrx_lookup_counts_host): lookup_string of hrx_lookup.hpp over rows in host memory,
// string-major (tight or pitched) or position-major as copied from the device, over threads by ranges of strings.  No HIP, no allocation; the host twin of
// hrx_kernel_lookup.hip and the definition of the counts.  tests/host_cpp/test_lookup_host.cpp includes this file as it is.
#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

#include "hrx_lookup.hpp"

namespace hrx {

namespace {

// string b of a batch in host memory (the address rules of include/hrx.h, as hrx_verify_rows_host reads them)
struct LookupHostRows {
    const LookupArgs &a;
    size_t b, k, bl, nb, q4;
    bool pm, in_pm;
    LookupHostRows(const LookupArgs &args, size_t string) : a(args), b(string) {
        k = b / kVfyPmBlock; bl = b % kVfyPmBlock; nb = std::min<size_t>(kVfyPmBlock, a.B - k * kVfyPmBlock);
        q4 = ((size_t)a.M + 3) / 4;
        pm = (a.layout & 1u) != 0; in_pm = (a.layout & 2u) != 0;
    }
    uint32_t chr(size_t i) const { return in_pm ? a.chars[k * kVfyPmBlock * a.stride + ((i / 16) * nb + bl) * 16 + i % 16] : a.chars[b * a.stride + i]; }
    uint32_t rec(size_t r, size_t d) const {
        return pm ? a.records[k * kVfyPmBlock * q4 * a.D * 4 + ((r / 4 * a.D + d) * nb + bl) * 4 + r % 4] : a.records[(b * a.rec_pitch + r) * a.D + d];
    }
};

// strings [i0, i1) of the window
void lookup_range(const LookupArgs &a, size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
        const size_t b = (size_t)a.b_begin + i;
        const uint32_t m = lookup_string(a.image, a.D, a.lens[b], a.M, LookupHostRows(a, b), a.counts + i * a.W);
        if (a.misses) a.misses[i] = m;
    }
}

}  // namespace

// arguments checked by the caller (a.image: build_lookup_image of the config, in host memory; a.W its lookup_words).  threads: 0 = as many as the machine
// has, at most 16; never more than one per 64 strings
void lookup_counts_host(const LookupArgs &a, unsigned threads) {
    if (a.b_count == 0 || a.M == 0) return;
    if (threads == 0) threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    threads = (unsigned)std::min<size_t>(threads, ((size_t)a.b_count + 63) / 64);
    if (threads <= 1) return lookup_range(a, 0, a.b_count);
    const size_t per = ((size_t)a.b_count + threads - 1) / threads;
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < threads; ++t) {
        const size_t i0 = std::min<size_t>(a.b_count, t * per), i1 = std::min<size_t>(a.b_count, i0 + per);
        if (i0 < i1) pool.emplace_back(lookup_range, std::cref(a), i0, i1);
    }
    lookup_range(a, 0, std::min<size_t>(a.b_count, per));
    for (std::thread &t : pool) t.join();
}

}  // namespace hrx
