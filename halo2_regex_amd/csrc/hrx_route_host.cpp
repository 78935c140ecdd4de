// hrx_route_host.cpp — the host form of ROUTE (include/hrx.h hrx_route_host): order / bucket_offsets out of status, lengths and the bucket bounds, all in
// host memory.  No context, no HIP, no allocation, re-entrant; the rules are those of hrx_route.hpp.  tests/host_cpp/test_route_host.cpp includes this
// file as it is.
#include "hrx_route.hpp"

namespace hrx {

// arguments checked by the caller.  Sequential: the strings are counted per bin, the counts become each bin's start (= bucket_offsets), then every
// string goes to its bin's next free place in increasing b — the partition is stable
void route_host(const RouteIn &in, uint32_t *order, uint64_t *bucket_offsets) {
    uint64_t at[kRouteBins] = {};
    for (uint64_t b = 0; b < in.B; ++b) ++at[route_bin(in, b)];
    uint64_t sum = 0;
    for (uint32_t n = 0; n <= in.bounds.n; ++n) {
        const uint64_t c = at[n];
        bucket_offsets[n] = at[n] = sum;
        sum += c;
    }
    bucket_offsets[in.bounds.n + 1] = sum;
    for (uint64_t b = 0; b < in.B; ++b) order[at[route_bin(in, b)]++] = (uint32_t)b;
}

}  // namespace hrx
