// hrx_kernel_route.hip — ROUTE (include/hrx.h hrx_route_device): a screened batch as a stable partition by circuit-size bucket, on the device.
//
// Three launches on the caller's stream, each one complete before the next starts; no workgroup waits for another (no look-back, flag, counter or atomic),
// so the result is deterministic and the sequence can be captured — the model of hrx_kernel_extract.hip, with its workgroup scan (hrx_block_scan.h):
//   route_count_kernel   one lane per string: its bin (hrx_route.hpp route_bin: the bucket of a kept string, bounds.n for every other one), the workgroup's
//                        strings per bin into the workspace
//   route_scan_kernel    one workgroup: exclusive prefix over the workgroups' partials (in place) for all kRouteBins bins at once (unused bins are zero: no
//                        variant per bucket count), then the prefix over the bins' totals = bucket_offsets, kept in the workspace as each bin's start
//   route_apply_kernel   one lane per string again: its rank among the workgroup's strings of its bin + the workgroup's base + the bin's start -> order
// Workspace (u64 words): [0, kRouteBins) the start of each bin's range in order, then kRouteBins words per count workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hrx_block_scan.h"
#include "hrx_kernel.hpp"

namespace hrx {

constexpr uint32_t kRT = kScanThreads;        // lanes (strings) per workgroup of count / apply, partials per round of scan
constexpr int kNB = (int)kRouteBins;

// v[n] = 1 for the bin of string b (none past the batch's end); returns the bin
__device__ __forceinline__ uint32_t string_bin(const RouteIn &in, uint64_t b, uint64_t (&v)[kNB]) {
    const uint32_t bin = b < in.B ? route_bin(in, b) : kRouteBins;
#pragma unroll
    for (int n = 0; n < kNB; ++n) v[n] = bin == (uint32_t)n ? 1u : 0u;
    return bin;
}

__global__ __launch_bounds__(kRT) void route_count_kernel(const RouteArgs a) {
    __shared__ uint64_t sh[kNB][kRT];
    uint64_t v[kNB], total[kNB];
    string_bin(a.in, (uint64_t)blockIdx.x * kRT + threadIdx.x, v);
    block_scan<kNB>(v, total, sh);
#pragma unroll
    for (int n = 0; n < kNB; ++n)
        if (threadIdx.x == (uint32_t)n) a.ws[kNB + kNB * (uint64_t)blockIdx.x + n] = total[n];
}

__global__ __launch_bounds__(kRT) void route_scan_kernel(uint64_t *ws, uint64_t n_parts, uint64_t *bucket_offsets, uint32_t n_buckets) {
    __shared__ uint64_t sh[kNB][kRT];
    uint64_t carry[kNB];
#pragma unroll
    for (int n = 0; n < kNB; ++n) carry[n] = 0;
    for (uint64_t g0 = 0; g0 < n_parts; g0 += kRT) {
        const uint64_t g = g0 + threadIdx.x;
        uint64_t v[kNB], total[kNB];
#pragma unroll
        for (int n = 0; n < kNB; ++n) v[n] = g < n_parts ? ws[kNB + kNB * g + n] : 0;
        block_scan<kNB>(v, total, sh);
        if (g < n_parts) {
#pragma unroll
            for (int n = 0; n < kNB; ++n) ws[kNB + kNB * g + n] = carry[n] + v[n];
        }
#pragma unroll
        for (int n = 0; n < kNB; ++n) carry[n] += total[n];
    }
    if (threadIdx.x == 0) {      // the bins in order: buckets 0 .. n_buckets - 1, then the strings that are not kept; bucket_offsets[n_buckets + 1] = B
        uint64_t at = 0;
#pragma unroll
        for (int n = 0; n < kNB; ++n) {
            ws[n] = at;
            if ((uint32_t)n <= n_buckets) bucket_offsets[n] = at;
            at += carry[n];
        }
        bucket_offsets[n_buckets + 1] = at;
    }
}

__global__ __launch_bounds__(kRT) void route_apply_kernel(const RouteArgs a) {
    __shared__ uint64_t sh[kNB][kRT];
    const uint64_t b = (uint64_t)blockIdx.x * kRT + threadIdx.x;
    uint64_t v[kNB], total[kNB];
    const uint32_t bin = string_bin(a.in, b, v);
    block_scan<kNB>(v, total, sh);
    if (b >= a.in.B) return;
    uint64_t rank = 0;      // (selected with constant indices: no indexed register array)
#pragma unroll
    for (int n = 0; n < kNB; ++n) rank += bin == (uint32_t)n ? v[n] : 0;
    const uint64_t at = a.ws[bin] + a.ws[kNB + kNB * (uint64_t)blockIdx.x + bin] + rank;
    if (at < a.in.B) a.order[at] = (uint32_t)b;      // (always, unless the input changed between the launches)
}

size_t route_workspace_bytes(size_t B) { return (kRouteBins + kRouteBins * ((B + kRT - 1) / kRT)) * sizeof(uint64_t); }

hipError_t launch_route(const RouteArgs &a, hipStream_t stream) {
    const uint64_t n_parts = (a.in.B + kRT - 1) / kRT;
    if (n_parts) hipLaunchKernelGGL(route_count_kernel, dim3((unsigned)n_parts), dim3(kRT), 0, stream, a);
    hipLaunchKernelGGL(route_scan_kernel, dim3(1), dim3(kRT), 0, stream, a.ws, n_parts, a.bucket_offsets, a.in.bounds.n);
    if (n_parts) hipLaunchKernelGGL(route_apply_kernel, dim3((unsigned)n_parts), dim3(kRT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hrx
