// hrx_kernel_extract.hip — EXTRACT (include/hrx.h hrx_extract_spans_device): the revealed bytes of a matched batch as an Arrow list column, on the device.
//
// Four launches on the caller's stream, each one complete before the next starts; no workgroup waits for another (no look-back, flag, counter or atomic),
// so the result is deterministic and the sequence can be captured:
//   extract_count_kernel    one lane per string: its k_b runs and their clipped bytes (hrx_extract.hpp), reduced per workgroup into the workspace
//   extract_scan_kernel     one workgroup: exclusive prefix over the workgroups' partials (in place), the totals
//   extract_apply_kernel    one lane per string again: scan inside the workgroup + the workgroup's base -> run_offsets[b], and runs[j] / byte_offsets[j + 1]
//                           of its runs under the capacity rule; the one lane that meets the first run that is not stored (or, where all are, the lane
//                           that owns the end) leaves J, the number of stored runs, in the workspace
//   extract_gather_kernel   a workgroup per 64 consecutive strings, which own one contiguous window of runs and of output bytes: 256 runs at a time go
//                           into LDS (byte offset, source address of the run's first byte), then every lane takes one output byte of the window — it finds
//                           the byte's run by binary search in LDS and copies the byte; the lanes of a wave write consecutive bytes, however long or
//                           short the runs are
// Workspace (u64 words): [0] R, [1] bytes, [2] truncated strings, [3] J, then 3 words per count workgroup (runs, bytes, truncated strings).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hrx_block_scan.h"
#include "hrx_kernel.hpp"

namespace hrx {

constexpr uint32_t kXT = kScanThreads;           // lanes (strings) per workgroup of count / apply, partials per round of scan (block_scan: hrx_block_scan.h)
constexpr uint32_t kGatherStrings = 64;          // strings per gather workgroup
constexpr uint32_t kGatherRuns = 256;            // runs in LDS at a time

// string b's runs, clipped bytes and whether it was truncated
__device__ __forceinline__ void string_sums(const ExtractIn &in, uint64_t b, uint64_t &k, uint64_t &bytes, uint64_t &trunc, uint64_t &limit) {
    k = bytes = trunc = limit = 0;
    if (b >= in.B) return;
    bool t;
    k = contributed_runs(in, b, limit, t);
    trunc = t;
    const uint64_t *sp = in.spans + b * in.max_spans;
    for (uint64_t i = 0; i < k; ++i) bytes += clip_run(sp[i], limit).len;
}

__global__ __launch_bounds__(kXT) void extract_count_kernel(const ExtractArgs a) {
    __shared__ uint64_t sh[3][kXT];
    uint64_t v[3], total[3], limit;
    string_sums(a.in, (uint64_t)blockIdx.x * kXT + threadIdx.x, v[0], v[1], v[2], limit);
    block_scan<3>(v, total, sh);
    if (threadIdx.x < 3) a.ws[4 + 3 * (uint64_t)blockIdx.x + threadIdx.x] = total[threadIdx.x];
}

__global__ __launch_bounds__(kXT) void extract_scan_kernel(uint64_t *ws, uint64_t n_parts) {
    __shared__ uint64_t sh[3][kXT];
    uint64_t carry[3] = {0, 0, 0};
    for (uint64_t g0 = 0; g0 < n_parts; g0 += kXT) {
        const uint64_t g = g0 + threadIdx.x;
        uint64_t v[3] = {0, 0, 0}, total[3];
        if (g < n_parts) {
#pragma unroll
            for (int n = 0; n < 3; ++n) v[n] = ws[4 + 3 * g + n];
        }
        block_scan<3>(v, total, sh);
        if (g < n_parts) {
#pragma unroll
            for (int n = 0; n < 3; ++n) ws[4 + 3 * g + n] = carry[n] + v[n];
        }
#pragma unroll
        for (int n = 0; n < 3; ++n) carry[n] += total[n];
    }
    if (threadIdx.x < 3) ws[threadIdx.x] = carry[threadIdx.x];
}

__global__ __launch_bounds__(kXT) void extract_apply_kernel(const ExtractArgs a) {
    __shared__ uint64_t sh[2][kXT];
    const ExtractIn &in = a.in;
    const uint64_t b = (uint64_t)blockIdx.x * kXT + threadIdx.x;
    uint64_t k, bytes, trunc, limit;
    string_sums(in, b, k, bytes, trunc, limit);
    uint64_t v[2] = {k, bytes}, total[2];
    block_scan<2>(v, total, sh);
    if (b < in.B) {
        uint64_t j = a.ws[4 + 3 * (uint64_t)blockIdx.x] + v[0], at = a.ws[4 + 3 * (uint64_t)blockIdx.x + 1] + v[1];
        a.run_offsets[b] = j;
        const uint64_t *sp = in.spans + b * in.max_spans;
        for (uint64_t i = 0; i < k; ++i, ++j) {
            const uint64_t w = sp[i], end = at + clip_run(w, limit).len;
            if (!run_is_stored(j, end, a.runs_cap, a.values_cap)) {
                // no later run is stored either; this one is the first such run iff the run before it is stored (its bytes end at `at`)
                if (j == 0 || run_is_stored(j - 1, at, a.runs_cap, a.values_cap)) a.ws[3] = j;
                break;
            }
            a.runs[j] = w;
            a.byte_offsets[j + 1] = end;
            at = end;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {      // the end: the totals, and J where every run is stored
        const uint64_t R = a.ws[0], total_bytes = a.ws[1];
        a.run_offsets[in.B] = R;
        a.byte_offsets[0] = 0;
        a.totals[0] = R;
        a.totals[1] = total_bytes;
        a.totals[2] = a.ws[2];
        a.totals[3] = 0;
        if (R == 0 || run_is_stored(R - 1, total_bytes, a.runs_cap, a.values_cap)) a.ws[3] = R;
    }
}

__global__ __launch_bounds__(256) void extract_gather_kernel(const ExtractArgs a) {
    __shared__ uint64_t s_ro[kGatherStrings + 1];      // run_offsets of the workgroup's strings
    __shared__ uint64_t s_bo[kGatherRuns + 1];         // byte_offsets of the runs in hand
    __shared__ uint64_t s_src[kGatherRuns];            // linear input: the address of the run's first byte; position-major: of byte 0 of its string's first chunk
    __shared__ uint32_t s_row[kGatherRuns], s_nb[kGatherRuns];     // position-major: the run's first row, the strings of its block
    const ExtractIn &in = a.in;
    const uint32_t tid = threadIdx.x;
    const uint64_t b0 = (uint64_t)blockIdx.x * kGatherStrings;
    const bool pm = in.layout == kExtractLayoutPositionMajor;
    if (tid <= kGatherStrings) s_ro[tid] = a.run_offsets[b0 + tid < in.B ? b0 + tid : in.B];
    __syncthreads();
    const uint64_t J = a.ws[3];
    const uint64_t r_end = s_ro[kGatherStrings] < J ? s_ro[kGatherStrings] : J;
    for (uint64_t r0 = s_ro[0]; r0 < r_end; r0 += kGatherRuns) {
        const uint32_t n = (uint32_t)(r_end - r0 < kGatherRuns ? r_end - r0 : kGatherRuns);
        if (tid < n) {
            const uint64_t j = r0 + tid;
            uint32_t lo = 0, hi = kGatherStrings;      // the run's string: s_ro[lo] <= j < s_ro[hi]
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_ro[mid] <= j) lo = mid; else hi = mid;
            }
            const uint64_t b = b0 + lo;
            uint64_t limit;
            (void)string_limit(in, b, limit);
            const ClippedRun c = clip_run(a.runs[j], limit);
            s_bo[tid] = a.byte_offsets[j];
            if (pm) {
                const uint64_t blk0 = b / kExtractPmBlock * kExtractPmBlock;
                s_src[tid] = (uint64_t)(uintptr_t)string_byte(in, b, 0);
                s_row[tid] = (uint32_t)c.start;
                s_nb[tid] = (uint32_t)(in.B - blk0 < kExtractPmBlock ? in.B - blk0 : kExtractPmBlock);
            } else {
                s_src[tid] = (uint64_t)(uintptr_t)string_byte(in, b, c.start);
            }
        }
        if (tid == 0) s_bo[n] = a.byte_offsets[r0 + n];
        __syncthreads();
        const uint64_t o_end = s_bo[n];
        // four bytes per lane and round, 256 apart: the four loads are in flight together
        for (uint64_t o0 = s_bo[0] + tid; o0 < o_end; o0 += 4 * 256) {
            uint8_t val[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t o = o0 + 256u * u;
                val[u] = 0;
                if (o < o_end) {
                    uint32_t lo = 0, hi = n;      // the byte's run: s_bo[lo] <= o < s_bo[hi] (the last of several that start at o: the one with bytes)
                    while (hi - lo > 1) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (s_bo[mid] <= o) lo = mid; else hi = mid;
                    }
                    const uint64_t x = o - s_bo[lo];
                    const uint8_t *p = reinterpret_cast<const uint8_t *>((uintptr_t)s_src[lo]);
                    if (pm) {
                        const uint64_t r = s_row[lo] + x;
                        val[u] = p[(r >> 4) * s_nb[lo] * 16 + (r & 15)];
                    } else {
                        val[u] = p[x];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t o = o0 + 256u * u;
                if (o < o_end) a.values[o] = val[u];
            }
        }
        __syncthreads();
    }
}

size_t extract_workspace_bytes(size_t B) { return (4 + 3 * ((B + kXT - 1) / kXT)) * sizeof(uint64_t); }

hipError_t launch_extract(const ExtractArgs &a, hipStream_t stream) {
    const uint64_t B = a.in.B, n_parts = (B + kXT - 1) / kXT;
    if (n_parts) hipLaunchKernelGGL(extract_count_kernel, dim3((unsigned)n_parts), dim3(kXT), 0, stream, a);
    hipLaunchKernelGGL(extract_scan_kernel, dim3(1), dim3(kXT), 0, stream, a.ws, n_parts);
    hipLaunchKernelGGL(extract_apply_kernel, dim3((unsigned)std::max<uint64_t>(n_parts, 1)), dim3(kXT), 0, stream, a);
    if (B) hipLaunchKernelGGL(extract_gather_kernel, dim3((unsigned)((B + kGatherStrings - 1) / kGatherStrings)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hrx
