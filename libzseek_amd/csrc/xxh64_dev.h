// xxh64_dev.h — XXH64's primes, round, merge and avalanche on the device, for
// frame_check.hip and zstd_check_kernel (zstd_decode.hip).  Each keeps its own
// stripe loop and tail: they load differently on purpose.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zsk {
namespace xxh64d {

constexpr uint64_t P64_1 = 0x9E3779B185EBCA87ull, P64_2 = 0xC2B2AE3D27D4EB4Full,
                   P64_3 = 0x165667B19E3779F9ull, P64_4 = 0x85EBCA77C2B2AE63ull,
                   P64_5 = 0x27D4EB2F165667C5ull;

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r)
{
    return (x << r) | (x >> (64 - r));
}

__device__ __forceinline__ uint64_t xround(uint64_t acc, uint64_t v)
{
    acc += v * P64_2;
    acc = rotl64(acc, 31);
    return acc * P64_1;
}

__device__ __forceinline__ uint64_t xmerge(uint64_t acc, uint64_t v)
{
    acc ^= xround(0, v);
    return acc * P64_1 + P64_4;
}

__device__ __forceinline__ uint64_t xavalanche(uint64_t h)
{
    h ^= h >> 33;
    h *= P64_2;
    h ^= h >> 29;
    h *= P64_3;
    h ^= h >> 32;
    return h;
}

}   // namespace xxh64d
}   // namespace zsk
