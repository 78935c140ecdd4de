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

#include "hrx_fr_device.h"

namespace hrx {

struct FrScan {
    Fr before;      // the product of the elements of all lanes below this one (R, the Montgomery one, for lane 0)
    Fr total;       // the workgroup's product
};

// v: the product of the lane's elements (Montgomery form).  wtot: WAVES elements of LDS, free again after the call's first barrier.  Every lane of the
// workgroup calls.
template <uint32_t WAVES>
__device__ __forceinline__ FrScan fr_block_scan_excl(const Fr &v, Fr *wtot) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Fr inc = v;
#pragma nounroll
    for (uint32_t off = 1; off < 64u; off <<= 1) inc = fr_select(lane >= off, fr_mul(fr_shfl_up(inc, off), inc), inc);
    __syncthreads();                                 // (wtot is free again)
    if (lane == 63u) wtot[wave] = inc;
    __syncthreads();
    const Fr ex = fr_select(lane == 0u, fr_R(), fr_shfl_up(inc, 1u));      // the lanes below in this wave
    Fr wb = fr_R();                                  // the waves below: R for wave 0, else what `total` was before this wave's turn
    FrScan out;
    out.total = wtot[0];
#pragma unroll
    for (uint32_t w = 1; w < WAVES; ++w) {
        wb = fr_select(wave == w, out.total, wb);
        out.total = fr_mul(out.total, wtot[w]);
    }
    out.before = fr_mul(wb, ex);
    return out;
}

}  // namespace hrx
