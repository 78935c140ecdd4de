// hrx_extract.hpp — the rules of EXTRACT (include/hrx.h: hrx_extract_spans_device / hrx_extract_spans_host) that must exist once: how a span word of
// a match call is decoded, how a run is clipped to its string, and how many runs a string contributes.  No HIP dependency: the kernels
// (hrx_kernel_extract.hip), the host gather (hrx_extract_host.cpp) and tests/host_cpp/test_extract_host.cpp all include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hrx_route.hpp"      // HRX_XHD, passes_screen: the screen ROUTE shares

namespace hrx {

constexpr uint32_t kExtractPmBlock = 65536u;      // = kPmBlock (hrx_lane.h): position-major input is blocked by this many strings
constexpr int kExtractLayoutStringMajor = 0, kExtractLayoutPositionMajor = 2, kExtractLayoutRagged = 8;      // the HRX_LAYOUT_* values the entry points take

// a span word as hrx_match_batch_* packs it: bits 0..27 start row, 28..55 length, 56..63 masked_substr_id
HRX_XHD uint64_t span_start(uint64_t w) { return w & 0xfffffffull; }
HRX_XHD uint64_t span_length(uint64_t w) { return (w >> 28) & 0xfffffffull; }
HRX_XHD uint64_t span_id(uint64_t w) { return w >> 56; }

// the part of a run that lies inside its string of `limit` bytes: rows [start, start + len)
struct ClippedRun {
    uint64_t start, len;
};
HRX_XHD ClippedRun clip_run(uint64_t w, uint64_t limit) {
    const uint64_t s = span_start(w) < limit ? span_start(w) : limit;
    const uint64_t room = limit - s;
    return ClippedRun{s, span_length(w) < room ? span_length(w) : room};
}

// the input of an extract call as both the host gather and the kernels see it
struct ExtractIn {
    int layout;                 // kExtractLayout*
    const uint8_t *src;         // chars [B][stride] / position-major blocks / values
    uint64_t stride;
    const uint64_t *offsets;    // ragged: [B + 1]
    uint64_t B;
    const uint64_t *status;
    const uint32_t *span_counts;
    const uint64_t *spans;      // [B][max_spans]
    uint64_t max_spans;
    uint32_t require_accept;
};

// the bytes of string b a run may name: [0, stride) of a padded slot, [0, n_b) of a ragged string; false: decreasing offsets (it contributes nothing)
HRX_XHD bool string_limit(const ExtractIn &in, uint64_t b, uint64_t &limit) {
    if (in.layout != kExtractLayoutRagged) {
        limit = in.stride;
        return true;
    }
    const uint64_t o0 = in.offsets[b], o1 = in.offsets[b + 1];
    limit = o1 >= o0 ? o1 - o0 : 0;
    return o1 >= o0;
}

// k_b: the runs string b contributes — min(span_counts[b], max_spans) where its status code is 0 and its accept bits cover require_accept, else 0;
// `truncated`: it contributes and the match call cut its runs at max_spans
HRX_XHD uint64_t contributed_runs(const ExtractIn &in, uint64_t b, uint64_t &limit, bool &truncated) {
    truncated = false;
    if (!string_limit(in, b, limit)) return 0;
    if (!passes_screen(in.status[b], in.require_accept)) return 0;
    const uint64_t c = in.span_counts[b];
    truncated = c > in.max_spans;
    return truncated ? in.max_spans : c;
}

// the address of byte r of string b (r below the string's limit)
HRX_XHD const uint8_t *string_byte(const ExtractIn &in, uint64_t b, uint64_t r) {
    if (in.layout == kExtractLayoutRagged) return in.src + in.offsets[b] + r;
    if (in.layout == kExtractLayoutStringMajor) return in.src + b * in.stride + r;
    // position-major: per block of kExtractPmBlock strings [stride / 16][nb][16]
    const uint64_t blk0 = b / kExtractPmBlock * kExtractPmBlock;
    const uint64_t nb = in.B - blk0 < kExtractPmBlock ? in.B - blk0 : kExtractPmBlock;
    return in.src + blk0 * in.stride + ((r >> 4) * nb + (b - blk0)) * 16 + (r & 15);
}

// the capacity rule: run j, whose bytes end at `end`, is stored iff j < runs_cap and end <= values_cap (both monotone in j: the stored runs are a prefix)
HRX_XHD bool run_is_stored(uint64_t j, uint64_t end, uint64_t runs_cap, uint64_t values_cap) { return j < runs_cap && end <= values_cap; }

}  // namespace hrx
