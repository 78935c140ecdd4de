// hrx_route.hpp — the rules of ROUTE (include/hrx.h: hrx_route_device / hrx_route_host) that must exist once: which strings pass the screen, which
// length a string has, and which circuit-size bucket takes it.  No HIP dependency: the kernels (hrx_kernel_route.hip), the host form
// (hrx_route_host.cpp) and tests/host_cpp/test_route_host.cpp all include it; EXTRACT (hrx_extract.hpp) takes its screen from here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__)  // clang in HIP mode (hipcc), host and device passes alike
#define HRX_XHD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define HRX_XHD inline
#endif

namespace hrx {

constexpr uint32_t kRouteMaxBuckets = 8;            // = HRX_MAX_BUCKETS
constexpr uint32_t kRouteBins = kRouteMaxBuckets + 1;      // the buckets and the range of the strings that are not kept
constexpr uint32_t kRouteMaxBound = 1u << 24;       // the largest M a witness entry point takes

// the screen of EXTRACT and ROUTE: status code 0 and the accept bits cover require_accept
HRX_XHD bool passes_screen(uint64_t status, uint32_t require_accept) {
    return (status & 0xffu) == 0 && ((uint32_t)(status >> 8) & require_accept) == require_accept;
}

// the bucket bounds, passed by value (the kernels take them as arguments: the caller's array is host memory)
struct RouteBounds {
    uint32_t n;                         // 1..kRouteMaxBuckets
    uint32_t v[kRouteMaxBuckets];       // strictly increasing, v[n - 1] <= kRouteMaxBound
};

// n in 1..kRouteMaxBuckets, strictly increasing, the last one <= kRouteMaxBound
inline bool route_bounds_valid(const uint32_t *bounds, size_t n) {
    if (!bounds || n < 1 || n > kRouteMaxBuckets) return false;
    for (size_t j = 1; j < n; ++j)
        if (bounds[j] <= bounds[j - 1]) return false;
    return bounds[n - 1] <= kRouteMaxBound;
}

// the input of a route call as both the host form and the kernels see it
struct RouteIn {
    const uint64_t *status;         // [B], or NULL: no screening
    uint32_t require_accept;
    const uint32_t *lens;           // [B], or NULL ...
    const uint64_t *offsets;        // ... then [B + 1]
    uint64_t B;
    RouteBounds bounds;
};

// n_b; false: a ragged string whose offsets decrease (it has no valid length)
HRX_XHD bool route_length(const RouteIn &in, uint64_t b, uint64_t &n) {
    if (in.lens) {
        n = in.lens[b];
        return true;
    }
    const uint64_t o0 = in.offsets[b], o1 = in.offsets[b + 1];
    n = o1 >= o0 ? o1 - o0 : 0;
    return o1 >= o0;
}

// the least j with n <= v[j] (n == v[j] belongs to bucket j: the witness accepts n == M); bounds.n where n passes the last bound
// (the bounds increase, so that j is the number of bounds below n; counted over all kRouteMaxBuckets with constant indices: no indexed array in a kernel)
HRX_XHD uint32_t bucket_of(const RouteBounds &bounds, uint64_t n) {
    uint32_t j = 0;
    for (uint32_t i = 0; i < kRouteMaxBuckets; ++i) j += (i < bounds.n && n > bounds.v[i]) ? 1u : 0u;
    return j;
}

// the range string b goes into: its bucket where it is kept (passes the screen, valid length, n_b <= the last bound), else bounds.n
HRX_XHD uint32_t route_bin(const RouteIn &in, uint64_t b) {
    uint64_t n;
    if (!route_length(in, b, n)) return in.bounds.n;
    if (in.status && !passes_screen(in.status[b], in.require_accept)) return in.bounds.n;
    return bucket_of(in.bounds, n);
}

}  // namespace hrx
