// hrx_kernel.hip — dispatch of the witness kernels (hrx_kernel_sm.hip, hrx_kernel_pm.hip; their launches are planned in hrx_plan.cpp) and the
// small auxiliary kernels: the states-in entry points of lib.rs:825-888 and the field-cell expansion.
#include <hip/hip_runtime.h>

#include "hrx_fr_device.h"
#include "hrx_kernel.hpp"
#include "hrx_lane.h"

namespace hrx {

__global__ void zero_u32_kernel(uint32_t *p) { *p = 0u; }
hipError_t launch_zero_u32(uint32_t *p, hipStream_t stream) {
    hipLaunchKernelGGL(zero_u32_kernel, dim3(1), dim3(1), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_witness(const WitnessArgs &a, const LaunchInfo &li, hipStream_t stream) {
    if (li.kernel == Kernel::Pp) return launch_witness_pp(a, li, stream);
    if (li.kernel == Kernel::Pmd) return launch_witness_pmd(a, li, stream);
    return li.kernel == Kernel::Pm ? launch_witness_pm(a, li, stream) : launch_witness_sm(a, li, stream);
}

// ---------------------------------------------------------------------------------------------
// states-in entry points (lib.rs:825-888): one thread per (def, row) looks the pair (s[i], s[i+1]) up.
// ---------------------------------------------------------------------------------------------
struct PairArgs {     // one def per launch
    const uint64_t *states;   // this def's n + 1 states
    uint64_t n;
    const uint16_t *pt;
    uint32_t ns;
    uint16_t *tags;           // this def's n tags
};

__global__ void pair_tags_kernel(const PairArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    const uint64_t cur = a.states[r], next = a.states[r + 1];
    uint16_t t = 0;
    if (cur < a.ns && next < a.ns) t = a.pt[cur * a.ns + next];
    a.tags[r] = t;
}

hipError_t launch_pair_tags(const uint64_t *states, size_t n, uint32_t D, const uint16_t *const *pair_tags,
                            const uint32_t *n_states, uint16_t *tags, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    for (uint32_t d = 0; d < D; ++d) {
        PairArgs a{states + (size_t)d * (n + 1), n, pair_tags[d], n_states[d], tags + (size_t)d * n};
        hipLaunchKernelGGL(pair_tags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
    }
    return hipGetLastError();
}

struct EndpointDefArgs {     // one def per launch
    const uint64_t *states, *substr_ids;
    uint64_t n;
    const uint8_t *member;
    uint32_t n_states, n_substrs, id_offset;
    uint8_t *flags;
};

__global__ void endpoint_flags_kernel(const EndpointDefArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    const uint64_t sid = a.substr_ids[r];
    uint8_t f = 0;
    if (sid != 0) {  // lib.rs:861-866, 874-879
        const uint64_t j = sid - a.id_offset;
        const uint64_t cur = a.states[r], next = a.states[r + 1];
        if (j < a.n_substrs) {
            if (cur < a.n_states) f |= a.member[j * a.n_states + cur] & 1;
            if (next < a.n_states) f |= a.member[j * a.n_states + next] & 2;
        }
    }
    a.flags[r] = f;
}

hipError_t launch_endpoint_flags(const EndpointArgs &a, const uint8_t *const *member, const uint32_t *dims, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    for (uint32_t d = 0; d < a.D; ++d) {
        EndpointDefArgs e{a.states + (size_t)d * (a.n + 1), a.substr_ids + (size_t)d * a.n, a.n, member[d], dims[3 * d], dims[3 * d + 1], dims[3 * d + 2],
                          a.flags + (size_t)d * a.n};
        hipLaunchKernelGGL(endpoint_flags_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, e);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// compact witness -> field cells.  A pair of threads per (string, row) expands the row's integers into what
// `Value::known(F::from(v))` holds for every advice cell the reference assigns (lib.rs:339-418, 473-519) and for its two
// result columns (lib.rs:752-771), F = bn256::Fr in Montgomery form (hrx_fr.h), column-major [col][string][row][4 limbs].
// Write-bound: 32 B per cell x (4 + 4 D) cells per row.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kFrJ = 4u;                                  // store instructions (32 rows each) per wave and column
constexpr uint32_t kFrRowsPerBlock = 4u * 32u * kFrJ;
__global__ __launch_bounds__(256) void fr_columns_kernel(const FrArgs a) {
    // thread = (row, half of the 32-byte cell): both lanes of a pair compute the cell, each stores its 16 bytes, so that a
    // store instruction writes 1 KiB of full lines (one lane per row stored half of every 32 bytes per instruction)
    // Every value a row holds is small — bytes, states, ids, flags — and F::from(v) costs ~200 VALU operations: the cells of v < 256 come out of an LDS table the block's 256 threads
    // build first (one entry each; 8 KiB), anything larger (states of DFAs beyond 256 states) is computed in place.  Computed per cell by both lanes of a pair the launch was VALU-bound
    // at 0.68 of the HBM peak.
    __shared__ uint4 frtab[512];
    fr_store16(&frtab[2u * threadIdx.x], fr_from_u32(threadIdx.x, a.canonical != 0));
    __syncthreads();
    const uint32_t half = threadIdx.x & 1u;
    const uint32_t bi = blockIdx.y;              // index inside the requested range
    const uint32_t b = a.b_begin + bi;
    const uint32_t n = min(a.lens[b], a.M);
    const RowsPlace s = rows_place<true>(a, b);           // where the string's cells lie (hrx_rows.hpp)
    const int form = rows_form(a);
    // a wave owns 32 kFrJ consecutive rows and writes them column by column: kFrJ store instructions in a row put 4 KiB
    // of ONE column down before the next column's turn (interleaving the columns instruction by instruction left every stream in
    // 1-KiB pieces)
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t rbase = blockIdx.x * kFrRowsPerBlock + wave * (32u * kFrJ) + (lane >> 1);
    const size_t col_cells = (size_t)a.col_cells;   // cells per column
    uint64_t *out0 = a.cells + ((size_t)bi * a.M + rbase) * 4u + half * 2u;
    auto put_rows = [&](const uint32_t col, const uint32_t (&v)[kFrJ]) {
#pragma unroll
        for (uint32_t j = 0; j < kFrJ; ++j) {
            if (rbase + j * 32u < a.M) {
                uint4 cell;
                if (v[j] < 256u) {
                    cell = frtab[2u * v[j] + half];
                } else {
                    const Fr w = fr_from_u32(v[j], a.canonical != 0);
                    cell = half ? fr_hi16(w) : fr_lo16(w);
                }
                unsigned char *p = reinterpret_cast<unsigned char *>(out0 + (size_t)col * col_cells * 4u + (size_t)j * 32u * 4u);
                store16_nt(p, cell);    // streaming: nothing reads the cells back here
            }
        }
    };
    uint32_t live[kFrJ], c[kFrJ];
#pragma unroll
    for (uint32_t j = 0; j < kFrJ; ++j) {
        const uint32_t r = min(rbase + j * 32u, a.M - 1u);
        live[j] = (rbase + j * 32u) < n ? 1u : 0u;
        c[j] = 0;
        if (live[j]) c[j] = chr_cell(s, r);
    }
    put_rows(0, live);   // char_enable                        lib.rs:342,346
    put_rows(1, c);      // characters                         lib.rs:343,347
    for (uint32_t d = 0; d < a.D; ++d) {
        uint32_t rec[kFrJ], f[kFrJ];
#pragma unroll
        for (uint32_t j = 0; j < kFrJ; ++j) {
            const uint32_t r = min(rbase + j * 32u, a.M - 1u);
            rec[j] = form == kRecPlanes ? rec_cell<kRecPlanes>(a, s, r, d) : form == kRecPm ? rec_cell<kRecPm>(a, s, r, d) : rec_cell<kRecSm>(a, s, r, d);
        }
#pragma unroll
        for (uint32_t j = 0; j < kFrJ; ++j) f[j] = rec[j] & 0xffffu;
        put_rows(2 + 4 * d, f);            // states[d]         lib.rs:390,415
#pragma unroll
        for (uint32_t j = 0; j < kFrJ; ++j) f[j] = (rec[j] >> 16) & 0xffu;
        put_rows(3 + 4 * d, f);            // substr_ids[d]     lib.rs:394,405
#pragma unroll
        for (uint32_t j = 0; j < kFrJ; ++j) f[j] = (rec[j] >> 24) & 1u;
        put_rows(4 + 4 * d, f);            // start_enable[d]   lib.rs:483-491
#pragma unroll
        for (uint32_t j = 0; j < kFrJ; ++j) f[j] = (rec[j] >> 25) & 1u;
        put_rows(5 + 4 * d, f);            // end_enable[d]     lib.rs:502-511
    }
    uint32_t mk[kFrJ], f[kFrJ];
#pragma unroll
    for (uint32_t j = 0; j < kFrJ; ++j) {
        const uint32_t r = min(rbase + j * 32u, a.M - 1u);
        mk[j] = form == kRecSm ? msk_cell<false>(s, r) : msk_cell<true>(s, r);
    }
#pragma unroll
    for (uint32_t j = 0; j < kFrJ; ++j) f[j] = mk[j] & 0xffu;
    put_rows(2 + 4 * a.D, f);              // masked_characters  lib.rs:752-757
#pragma unroll
    for (uint32_t j = 0; j < kFrJ; ++j) f[j] = mk[j] >> 8;
    put_rows(3 + 4 * a.D, f);              // all_substr_ids     lib.rs:758-761
}

hipError_t launch_fr_columns(const FrArgs &a, hipStream_t stream) {
    if (a.b_count == 0 || a.M == 0) return hipSuccess;
    hipLaunchKernelGGL(fr_columns_kernel, dim3((a.M + kFrRowsPerBlock - 1u) / kFrRowsPerBlock, a.b_count), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hrx
