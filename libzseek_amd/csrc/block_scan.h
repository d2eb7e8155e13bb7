// block_scan.h — the one-workgroup prefix sum over n 64-bit values that the
// segment copy's scan (range_gather.hip, range_scan_kernel) and the image
// builder's plan (image_build.hip, image_plan_kernel) share: each of the T
// threads takes a contiguous share of the n elements, sums it, and the shares'
// sums are scanned in LDS.  Device code, internal.
#ifndef ZSK_BLOCK_SCAN_H
#define ZSK_BLOCK_SCAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zsk {

// thread t's share [a, b) of n elements
template <uint32_t T>
__device__ __forceinline__ void block_share(uint32_t n, uint32_t t, uint32_t *a, uint32_t *b)
{
    const uint64_t per = (n + T - 1) / T;
    const uint64_t lo = per * t, hi = per * (t + 1);
    *a = (uint32_t)(lo < n ? lo : n);
    *b = (uint32_t)(hi < n ? hi : n);
}

// The inclusive scan of the threads' `sum` (every thread of the workgroup
// calls it; s_sum: T words of LDS): the sum of the shares up to and including
// thread t's.  s_sum[T - 1] is the total afterwards.
template <uint32_t T>
__device__ __forceinline__ uint64_t block_scan_inclusive(uint64_t *s_sum, uint32_t t, uint64_t sum)
{
    s_sum[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < T; d <<= 1) {
        const uint64_t y = t >= d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += y;
        __syncthreads();
    }
    return s_sum[t];
}

}   // namespace zsk

#endif
