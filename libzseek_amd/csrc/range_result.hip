// range_result.hip — the per-range results of zsk_preadv_device_async, on the
// device (gfx950): range_result.h's walk, one wave64 per range.
//
// A wave takes ranges in a grid-stride loop.  Its lanes test the range's
// touched frames 64 at a time, in order (range_lane_failed); a ballot plus its
// lowest set bit gives the first failed frame and the walk stops at the first
// chunk that has one.  Lane 0 writes d_result[r].  The ranges delivered in full
// are counted per wave, summed per workgroup through LDS, and added to
// d_result[n] (zeroed on the stream first) with one vector atomic per
// workgroup.  The row and the chunk loop are wave-uniform (the wave's index is
// read through readfirstlane), so the row comes through scalar loads and the
// only vector memory traffic is one status dword per lane and chunk.
// Plain vector loads, stores and atomics only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "range_result.h"
#include "zsk_internal.h"

namespace zsk {

namespace {

// (sixteen waves per workgroup and at most two workgroups per CU: every
// workgroup ends in one atomic on the same word, and those serialize)
constexpr uint32_t kResultT = 1024;                         // threads per workgroup
constexpr uint32_t kResultWaves = kResultT / kResultLanes;  // ranges in flight per workgroup
constexpr uint32_t kResultGrid = 512;                       // most workgroups (2 per CU of 256)

__global__ __launch_bounds__(kResultT) void range_result_kernel(const RangeRow *__restrict__ rows,
                                                                const uint64_t *__restrict__ t_doff,
                                                                const int32_t *__restrict__ status, uint64_t n,
                                                                int64_t *__restrict__ result)
{
    __shared__ uint32_t s_full[kResultWaves];
    const uint32_t lane = threadIdx.x & (kResultLanes - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kResultLanes);
    uint32_t nfull = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kResultWaves + wave; r < n; r += (uint64_t)gridDim.x * kResultWaves) {
        const RangeRow row = rows[r];
        uint64_t bad = kNoBad;
        for (uint64_t k0 = 0; k0 < row.rtn; k0 += kResultLanes) {
            const uint64_t failed = __ballot(range_lane_failed(row, status, k0, lane));
            if (failed) {
                bad = k0 + (uint64_t)__builtin_ctzll(failed);
                break;
            }
        }
        bool full;
        const int64_t res = range_result_of(row, t_doff, bad, &full);
        if (lane == 0)
            result[r] = res;
        nfull += full;
    }
    if (lane == 0)
        s_full[wave] = nfull;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kResultWaves; w++)
            sum += s_full[w];
        if (sum)
            atomicAdd(reinterpret_cast<unsigned long long *>(result + n), (unsigned long long)sum);
    }
}

}   // namespace

int launch_range_result(const RangeRow *d_rows, const uint64_t *d_tdoff, const int32_t *d_status, uint64_t n,
                        int64_t *d_result, hipStream_t stream)
{
    if (!d_result)
        return -1;
    if (hipMemsetAsync(d_result + n, 0, sizeof(int64_t), stream) != hipSuccess)
        return -1;
    if (n == 0)
        return 0;
    if (!d_rows)
        return -1;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kResultWaves - 1) / kResultWaves, kResultGrid);
    hipLaunchKernelGGL(range_result_kernel, dim3(grid), dim3(kResultT), 0, stream, d_rows, d_tdoff, d_status, n,
                       d_result);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}   // namespace zsk
