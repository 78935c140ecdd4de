// hrx_host_walk.hpp — native small-batch host path (hrx_host_walk.cpp): the lane algorithm of hrx_lane.h run on a host core.
#pragma once
#include <cstddef>
#include <cstdint>

#include "hrx_defs.hpp"

namespace hrx {

// one string -> compact rows (records [M][D], masked [M]); returns the status word of include/hrx.h
uint64_t host_witness_one(const DefsSet &s, const uint8_t *chars, size_t n, size_t M, uint32_t *records, uint16_t *masked);
// string-major batch, `threads` host threads (contiguous slices of the batch)
void host_witness_batch(const DefsSet &s, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B, size_t M,
                        uint32_t *records, uint16_t *masked, uint64_t *status, int threads);
// one string -> status, its revealed runs (the first max_spans of them into spans) and their number (0 unless the status code is 0); no rows written
uint64_t host_match_one(const DefsSet &s, const uint8_t *chars, size_t n, size_t M, uint64_t *spans, size_t max_spans, uint32_t *count);
// string-major batch: status [B], span_counts [B] (may be NULL), spans [B][max_spans] (NULL when max_spans = 0)
void host_match_batch(const DefsSet &s, const uint8_t *chars, size_t stride, const uint32_t *lens, size_t B, size_t M,
                      uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, int threads);
// ragged batch (include/hrx.h RAGGED): string b is values[offsets[b] .. offsets[b + 1])
void host_match_batch_ragged(const DefsSet &s, const uint8_t *values, const uint64_t *offsets, size_t B, size_t M,
                             uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, int threads);
// a selection of either batch form (include/hrx.h hrx_match_selected_host): offsets non-NULL: ragged; results at index sel[k]
void host_match_selected(const DefsSet &s, const uint8_t *src, size_t stride, const uint32_t *lens, const uint64_t *offsets, size_t B, const uint32_t *sel,
                         size_t n_sel, size_t M, uint64_t *status, uint32_t *span_counts, uint64_t *spans, size_t max_spans, int threads);
bool host_derive_states(const DefsSet &s, const uint8_t *chars, size_t n, uint64_t *states, uint32_t &bad_state, uint32_t &bad_char);
void host_pair_tags(const DefsSet &s, const uint64_t *states, size_t n, uint16_t *tags);
void host_endpoint_flags(const DefsSet &s, const uint64_t *states, const uint64_t *substr_ids, size_t n, uint8_t *flags);

}  // namespace hrx
