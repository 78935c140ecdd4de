// hrx_kernel_lookup.hip — LOOKUP COUNTS on the device (include/hrx.h hrx_lookup_counts_device*): the rule of hrx_lookup.hpp over the witness rows where they lie.
//
// A histogram with the bins in LDS.  A workgroup of 512 lanes owns G consecutive strings of the window (G a power of two, plan_lookup of hrx_lookup.hpp) and
// keeps their whole runs — every def's trans / start / end bins, G x W u32 — in LDS.  All its waves stride over (string, record quad) items def by def: a lane
// takes the four records of one quad of one string, the state behind the quad from the next quad's first record, the quad's four input bytes, looks the
// three tuples of each row up in the image (device memory; it stays cache resident) and adds to the bins with LDS atomics that return nothing (ds_add_u32),
// one add per run of equal bins among the quad's four rows (a row without a flag and a disabled row hit the tables' first rows: no image read).  In the
// position-major layouts consecutive lanes hold consecutive strings, so a wave's load reads runs of G x 16 bytes; string-major rows go through the same
// loop with consecutive lanes on consecutive quads of one string.  At the end the workgroup writes its G runs — one contiguous piece of the output — in
// 16-byte stores, every word once, pad words included, and the strings' misses beside them.
// A run that does not fit the LDS of a CU at G = 1 is served in passes: the workgroup walks the rows once per range of pass_words bins and adds only what
// falls into the range; a def's misses are counted in the pass that holds its first bin.
// No global atomics, no scratch, nothing allocated; the result does not depend on the order of the adds.
#include <hip/hip_runtime.h>

#include "../../include/hrx.h"
#include "hrx_device.h"
#include "hrx_lookup.hpp"

namespace hrx {

namespace {

template <int REC>
__global__ __launch_bounds__(kLkThreads) void lookup_counts_kernel(const LookupArgs a) {
    uint32_t *bins = reinterpret_cast<uint32_t *>(smem);
    const uint32_t G = a.G, PW = a.pass_words, W = a.W, M = a.M, tid = threadIdx.x;
    uint32_t *miss = bins + (size_t)G * PW;
    const uint32_t i0 = blockIdx.x * G;                      // the group's first string in the window
    const uint32_t gv = min(G, a.b_count - i0);              // its strings
    const uint32_t Q = (M + 3u) / 4u, lgG = 31u - (uint32_t)__clz((int)G);
    const LookupDef *defs = reinterpret_cast<const LookupDef *>(a.image);
    if (tid < G) miss[tid] = 0u;
    for (uint32_t p = 0; p < a.passes; ++p) {
        const uint32_t lo = p * PW, hi = min(W, lo + PW);    // the pass's range of a run: multiples of 4
        for (uint32_t v = tid; v < G * (PW / 4u); v += kLkThreads) reinterpret_cast<uint4 *>(bins)[v] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        for (uint32_t d = 0; d < a.D; ++d) {
            const LookupDef T = defs[d];
            const uint32_t dlo = T.off, dhi = T.off + T.n_tr + 2u * T.n_ep;
            if (dhi <= lo || dlo >= hi) continue;
            const bool count_miss = dlo >= lo;               // the pass that holds the def's first bin
            uint32_t g_cur = 0xffffffffu, n = 0;
            RowsPlace s{};
            for (uint32_t item = tid; item < G * Q; item += kLkThreads) {
                uint32_t g, q;
                if constexpr (REC == kRecSm) { g = item / Q; q = item - g * Q; }
                else { g = item & (G - 1u); q = item >> lgG; }
                if (g >= gv) continue;
                if (g != g_cur) {
                    const uint32_t b = a.b_begin + i0 + g;
                    g_cur = g; n = a.lens[b]; s = rows_place<false>(a, b);
                }
                if (n > M) continue;                         // the string has no rows: its bins stay 0
                const uint32_t r0 = 4u * q;
                uint32_t c4 = 0;
                if (r0 < n) c4 = *reinterpret_cast<const uint32_t *>(chr_chunk(s, r0) + (r0 & 15u));
                uint32_t x[4];                               // def d's records of rows 4 q .. 4 q + 3 (rows >= M: never judged)
                if constexpr (REC == kRecSm) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) x[j] = r0 + j < M ? rec_cell<kRecSm>(a, s, r0 + j, d) : 0u;
                } else {
                    const uint4 v = *reinterpret_cast<const uint4 *>(rec_quad<REC>(a, s, q, d));
                    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
                }
                const uint32_t behind = r0 + 4u < M ? rec_cell<REC>(a, s, r0 + 4u, d) & 0xffffu : T.dummy;
                uint32_t *mine = bins + (size_t)g * PW;
                // one add per run of equal bins among the quad's rows (the flagless rows' and the padding rows' tuples all hit the tables' first rows)
                uint32_t run_at[3] = {kLkNone, kLkNone, kLkNone}, run_n[3] = {0u, 0u, 0u};
                auto flush = [&](const uint32_t at, const uint32_t cnt) {
                    if (at == kLkMiss) {
                        if (count_miss) atomicAdd(&miss[g], cnt);
                    } else if (at != kLkNone && at >= lo && at < hi) {
                        atomicAdd(&mine[at - lo], cnt);
                    }
                };
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t r = r0 + j;
                    if (r >= M) break;
                    const uint32_t next_state = j == 3 ? behind : (r + 1u < M ? x[j < 3 ? j + 1 : 3] & 0xffffu : T.dummy);
                    const uint32_t c = r < n ? (c4 >> (8 * j)) & 0xffu : 0u;
                    const LookupHit h = lookup_def_row(a.image, T, r, n, M, c, x[j], next_state);
                    const uint32_t w[3] = {h.trans, h.start, h.end};
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (w[k] == run_at[k]) {
                            ++run_n[k];
                        } else {
                            flush(run_at[k], run_n[k]);
                            run_at[k] = w[k]; run_n[k] = 1u;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) flush(run_at[k], run_n[k]);
            }
        }
        __syncthreads();
        const uint32_t nw4 = (hi - lo) / 4u;
        for (uint32_t v = tid; v < gv * nw4; v += kLkThreads) {
            const uint32_t g = v / nw4, k = v - g * nw4;
            const uint4 val = reinterpret_cast<const uint4 *>(bins + (size_t)g * PW)[k];
            *reinterpret_cast<uint4 *>(a.counts + (size_t)(i0 + g) * W + lo + 4u * k) = val;
        }
        __syncthreads();
    }
    if (a.misses && tid < gv) a.misses[i0 + tid] = a.lens[a.b_begin + i0 + tid] > M ? kLkTooLong : miss[tid];
}

template <int REC>
hipError_t launch_lookup_form(const LookupArgs &a, size_t lds_bytes, hipStream_t stream) {
    static std::atomic<size_t> granted{64u * 1024u};
    if (const hipError_t e = ensure_lds(lookup_counts_kernel<REC>, granted, lds_bytes); e != hipSuccess) return e;
    const dim3 grid((a.b_count + a.G - 1u) / a.G), block(kLkThreads);
    hipLaunchKernelGGL((lookup_counts_kernel<REC>), grid, block, lds_bytes, stream, a);
    return hipGetLastError();
}

}  // namespace

// the caller has checked the arguments, planned G / pass_words / passes and that ceil(b_count / G) workgroups fit a grid
hipError_t launch_lookup_counts(const LookupArgs &a, size_t lds_bytes, hipStream_t stream) {
    if (a.b_count == 0 || a.M == 0) return hipSuccess;
    switch (rows_form(a)) {
        case kRecSm: return launch_lookup_form<kRecSm>(a, lds_bytes, stream);
        case kRecPm: return launch_lookup_form<kRecPm>(a, lds_bytes, stream);
        default: return launch_lookup_form<kRecPlanes>(a, lds_bytes, stream);
    }
}

}  // namespace hrx
