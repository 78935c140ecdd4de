// hrx_fr_scan.h — the workgroup PRODUCT scan over bn256::Fr elements that LOOKUP PRODUCT's two kernels share (hrx_kernel_product.hip): what hrx_block_scan.h
// is for sums of u64, for Montgomery products of eight u32 limbs.  Device code only.
//
// The caller's lane multiplies its own consecutive elements serially and hands their product in; the 64 lanes of a wave scan with shuffles — eight limbs
// per element, one fr_mul per step, six steps; the waves meet through LDS (one element per wave); the lane gets the product of everything before it in
// the workgroup and the workgroup's total, and applies the first to its own elements.  With k elements per lane that is 2 + 10 / k fr_mul per element:
// k - 1 for the lane's own products, 6 + 3 + 1 here, k - 1 to apply the prefix (the first element IS the prefix), and the caller's two for a carry.
// No atomics; two barriers.
#pragma once
#include <hip/hip_runtime.h>

#include "hrx_fr.h"

namespace hrx {

// v: the product of the lane's elements (Montgomery form).  before: the product of the elements of all lanes below this one (R, the Montgomery one, for
// lane 0); total: the workgroup's product.  wtot: WAVES x 8 words of LDS, free again after the call's first barrier.  Every lane of the workgroup calls.
template <uint32_t WAVES>
__device__ __forceinline__ void fr_block_scan_excl(const uint32_t (&v)[8], uint32_t (&before)[8], uint32_t (&total)[8], uint32_t (*wtot)[8]) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) inc[i] = v[i];
#pragma nounroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        uint32_t n[8], p[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) n[i] = (uint32_t)__shfl_up((int)inc[i], off, 64);
        fr_mul(n, inc, p);
#pragma unroll
        for (int i = 0; i < 8; ++i) inc[i] = lane >= off ? p[i] : inc[i];
    }
    __syncthreads();                                 // (wtot is free again)
    if (lane == 63u) {
#pragma unroll
        for (int i = 0; i < 8; ++i) wtot[wave][i] = inc[i];
    }
    __syncthreads();
    uint32_t ex[8];                                  // the lanes below in this wave
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc[i], 1u, 64);
        ex[i] = lane == 0u ? kFrR32[i] : up;
    }
    uint32_t wb[8];                                  // the waves below: R for wave 0, else what `total` was before this wave's turn
#pragma unroll
    for (int i = 0; i < 8; ++i) { wb[i] = kFrR32[i]; total[i] = wtot[0][i]; }
#pragma unroll
    for (uint32_t w = 1; w < WAVES; ++w) {
        uint32_t x[8], p[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { x[i] = wtot[w][i]; wb[i] = wave == w ? total[i] : wb[i]; }
        fr_mul(total, x, p);
#pragma unroll
        for (int i = 0; i < 8; ++i) total[i] = p[i];
    }
    fr_mul(wb, ex, before);
}

}  // namespace hrx
