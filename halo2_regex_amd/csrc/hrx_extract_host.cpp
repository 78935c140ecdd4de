// hrx_extract_host.cpp — the host form of EXTRACT (include/hrx.h hrx_extract_spans_host): run_offsets / runs / byte_offsets / values / totals out of a
// match call's status, counts and spans and the input bytes, all in host memory.  No context, no HIP, re-entrant; the rules are those of
// hrx_extract.hpp.  tests/host_cpp/test_extract_host.cpp includes this file as it is.
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/hrx.h"
#include "hrx_extract.hpp"

namespace hrx {

// arguments checked by the caller.  One sequential pass lays out the runs (a few words per run); the byte copies then go over `threads` ranges of
// strings, each into its own part of values (the ranges are disjoint: nothing is shared but read-only arrays)
void extract_host(const ExtractIn &in, const hrx_extract_out &out, int threads) {
    uint64_t j = 0, bytes = 0, truncated = 0, stored = 0;
    out.byte_offsets[0] = 0;
    for (uint64_t b = 0; b < in.B; ++b) {
        out.run_offsets[b] = j;
        uint64_t limit;
        bool trunc;
        const uint64_t k = contributed_runs(in, b, limit, trunc);
        truncated += trunc;
        for (uint64_t i = 0; i < k; ++i, ++j) {
            const uint64_t w = in.spans[b * in.max_spans + i];
            bytes += clip_run(w, limit).len;
            if (!run_is_stored(j, bytes, out.runs_cap, out.values_cap)) continue;
            out.runs[j] = w;
            out.byte_offsets[j + 1] = bytes;
            stored = j + 1;
        }
    }
    out.run_offsets[in.B] = j;
    out.totals[0] = j;
    out.totals[1] = bytes;
    out.totals[2] = truncated;
    out.totals[3] = 0;
    if (stored == 0) return;
    auto copy_strings = [&](uint64_t b0, uint64_t b1) {
        for (uint64_t b = b0; b < b1; ++b) {
            uint64_t limit;
            if (!string_limit(in, b, limit)) continue;
            const uint64_t r1 = out.run_offsets[b + 1] < stored ? out.run_offsets[b + 1] : stored;
            for (uint64_t r = out.run_offsets[b]; r < r1; ++r) {
                const ClippedRun c = clip_run(out.runs[r], limit);
                uint8_t *dst = out.values + out.byte_offsets[r];
                if (in.layout != kExtractLayoutPositionMajor) {
                    if (c.len) std::memcpy(dst, string_byte(in, b, c.start), c.len);
                } else {
                    for (uint64_t x = 0; x < c.len; ++x) dst[x] = *string_byte(in, b, c.start + x);
                }
            }
        }
    };
    const uint64_t nt = threads > 1 ? (uint64_t)threads : 1;
    if (nt == 1 || in.B < 2 * nt) {
        copy_strings(0, in.B);
        return;
    }
    std::vector<std::thread> pool;
    for (uint64_t t = 0; t < nt; ++t) pool.emplace_back(copy_strings, in.B * t / nt, in.B * (t + 1) / nt);
    for (auto &t : pool) t.join();
}

}  // namespace hrx
