// hrx_fr_device.h — an element of hrx_fr.h as the device moves it: two 16-byte halves to and from global memory or LDS, across the lanes of a wave, into
// scalar registers.  Device code only.  Where the halves lie — a cell's address, an LDS slot, which lane holds which half — is the kernel's own business;
// this is the eight words <-> two uint4 part.  No reduction anywhere: a cell read is below r by contract (include/hrx.h).
#pragma once
#include <hip/hip_runtime.h>

#include "hrx_device.h"
#include "hrx_fr.h"

namespace hrx {

__device__ __forceinline__ uint4 fr_lo16(const Fr &x) { return make_uint4(x.w[0], x.w[1], x.w[2], x.w[3]); }
__device__ __forceinline__ uint4 fr_hi16(const Fr &x) { return make_uint4(x.w[4], x.w[5], x.w[6], x.w[7]); }
__device__ __forceinline__ Fr fr_of16(const uint4 &lo, const uint4 &hi) { return Fr{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}}; }

// p: the low half, 16-byte aligned, in global memory or LDS; the high half lies `apart` 16-byte slots on (1: a cell as it lies in memory)
__device__ __forceinline__ Fr fr_load16(const void *p, const uint32_t apart = 1u) {
    const uint4 *h = static_cast<const uint4 *>(p);
    return fr_of16(h[0], h[apart]);
}
// plain stores: for cells that are read back (inside the workgroup, or by the next launch) and for LDS
__device__ __forceinline__ void fr_store16(void *p, const Fr &x, const uint32_t apart = 1u) {
    uint4 *h = static_cast<uint4 *>(p);
    h[0] = fr_lo16(x);
    h[apart] = fr_hi16(x);
}
// streaming stores (global memory): for cells nothing reads back here
__device__ __forceinline__ void fr_store16_nt(void *p, const Fr &x) {
    store16_nt(p, fr_lo16(x));
    store16_nt(static_cast<uint4 *>(p) + 1, fr_hi16(x));
}

// the element of the lane `off` below in the wave (the lane's own where there is none)
__device__ __forceinline__ Fr fr_shfl_up(const Fr &x, const uint32_t off) {
    Fr out;
#pragma unroll
    for (int i = 0; i < 8; ++i) out.w[i] = (uint32_t)__shfl_up((int)x.w[i], off, 64);
    return out;
}
// a value every lane of the wave holds alike, into scalar registers
__device__ __forceinline__ Fr fr_readfirstlane(const Fr &x) {
    Fr out;
#pragma unroll
    for (int i = 0; i < 8; ++i) out.w[i] = __builtin_amdgcn_readfirstlane(x.w[i]);
    return out;
}

}  // namespace hrx
