// hrx_block_scan.h — the one workgroup scan of the count / scan / apply launches of EXTRACT (hrx_kernel_extract.hip) and ROUTE (hrx_kernel_route.hip):
// N sums at once over the kScanThreads lanes of a workgroup, in LDS, no atomics.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "hrx_kernel.hpp"

namespace hrx {

constexpr uint32_t kScanThreads = kExtractThreads;      // lanes per workgroup of every kernel that calls block_scan

// v[n] -> the exclusive prefix over the workgroup's lanes, total[n] the workgroup's sum (sh: N x kScanThreads words of LDS)
template <int N>
__device__ __forceinline__ void block_scan(uint64_t (&v)[N], uint64_t (&total)[N], uint64_t (*sh)[kScanThreads]) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int n = 0; n < N; ++n) sh[n][tid] = v[n];
    __syncthreads();
    for (uint32_t off = 1; off < kScanThreads; off <<= 1) {
        uint64_t t[N];
#pragma unroll
        for (int n = 0; n < N; ++n) t[n] = tid >= off ? sh[n][tid - off] : 0;
        __syncthreads();
#pragma unroll
        for (int n = 0; n < N; ++n) sh[n][tid] += t[n];
        __syncthreads();
    }
#pragma unroll
    for (int n = 0; n < N; ++n) {
        total[n] = sh[n][kScanThreads - 1];
        v[n] = sh[n][tid] - v[n];
    }
    __syncthreads();
}

}  // namespace hrx
