// hrx_ragged_src.h — where the strings of the persistent-lane match kernels and of the staging kernels lie (hrx_kernel_ragged.hip, hrx_kernel_match_wide.hip):
//   realign        the bytes that start at byte sh of a window of aligned dwords
//   ragged_string  string b of a ragged batch: first byte and length
//   RaggedSrc / PaddedSrc   the two sources of the selected and the fused-wide kernels: string(b, limit, p, n)
// Included after hrx_device.h.
#pragma once

namespace hrx {

// o[k] = dword k of the bytes that start at byte sh (0..15) of the window w (N + 4 dwords): a dword shift by sh / 4 in two select
// stages (the shift is the lane's own: no indexed register array), then v_alignbyte_b32 by sh % 4
template <int N>
__device__ __forceinline__ void realign(const uint32_t (&w)[N + 4], uint32_t sh, uint32_t (&o)[N]) {
    // (bit masks, not ?: on array elements, which the compiler turns into a dynamically indexed load: scratch memory)
    uint32_t y[N + 2], z[N + 1];
    const uint32_t m2 = 0u - ((sh >> 3) & 1u), m1 = 0u - ((sh >> 2) & 1u);
#pragma unroll
    for (int i = 0; i < N + 2; ++i) y[i] = (w[i + 2] & m2) | (w[i] & ~m2);
#pragma unroll
    for (int i = 0; i < N + 1; ++i) z[i] = (y[i + 1] & m1) | (y[i] & ~m1);
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = __builtin_amdgcn_alignbyte(z[k + 1], z[k], sh & 3u);
}

// string b of a ragged batch: its first byte and length; false where the offsets decrease or the length passes `limit`
__device__ __forceinline__ bool ragged_string(const uint8_t *values, const uint64_t *offsets, uint64_t base, size_t b, uint64_t limit,
                                              const uint8_t *&p, uint32_t &n) {
    const uint64_t o0 = offsets[b], o1 = offsets[b + 1];
    if (o1 < o0 || o1 - o0 > limit) return false;
    p = values + (o0 - base);
    n = (uint32_t)(o1 - o0);
    return true;
}

// where a string of the staging kernels and of the selected match lies: string(b, limit, p, n) -> its first byte and length; false where it has no
// valid length or the length passes `limit` (none of its bytes is read then)
struct RaggedSrc {          // values + offsets
    const uint8_t *values;
    const uint64_t *offsets;
    uint64_t base;
    __device__ __forceinline__ bool string(size_t b, uint64_t limit, const uint8_t *&p, uint32_t &n) const {
        return ragged_string(values, offsets, base, b, limit, p, n);
    }
};
struct PaddedSrc {          // chars + b * src_stride with lens[b]: 16-byte aligned slots, the sh = 0 case of ragged_chunk (bytes past n are never kept)
    const uint8_t *chars;
    const uint32_t *lens;
    uint64_t src_stride;
    __device__ __forceinline__ bool string(size_t b, uint64_t limit, const uint8_t *&p, uint32_t &n) const {
        const uint32_t len = lens[b];
        if (len > limit || len > src_stride) return false;
        p = chars + b * src_stride;
        n = len;
        return true;
    }
};

}  // namespace hrx
