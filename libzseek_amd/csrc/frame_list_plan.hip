// frame_list_plan.hip — the device plan of zsk_read_frames_indirect (gfx950):
// frame_list_plan.h's four steps as kernels.  The index list is read from
// device memory on the caller's stream, the seek table is the reader's resident
// copy, and everything the plan produces -- offsets, descriptors, checksum
// words, the span's flag -- stays on the device: the host sizes the grids by
// nidx and learns no size.
//
//   frame_list_size_kernel     thread per slot
//   frame_list_scan_kernel     one workgroup of kCompactT threads (block_scan.h)
//   frame_list_emit_kernel     thread per slot
//   frame_list_result_kernel   thread per slot, behind the decode
//
// Plain vector loads, stores and atomics only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stddef.h>

#include "block_scan.h"
#include "frame_list_plan.h"
#include "zsk_internal.h"

namespace zsk {

static_assert(sizeof(DevFrame) == sizeof(FrameDesc) && offsetof(DevFrame, c_size) == offsetof(FrameDesc, c_size) &&
                  offsetof(DevFrame, d_off) == offsetof(FrameDesc, d_off),
              "descriptor ABI");
static_assert(kPlanSpan == ZSK_PLAN_SPAN, "the flag is part of the C ABI");

namespace {

constexpr uint32_t kListT = 256;   // threads per workgroup of the per-slot kernels

__global__ __launch_bounds__(kListT) void frame_list_size_kernel(const int64_t *__restrict__ idx, uint64_t n,
                                                                 const uint64_t *__restrict__ d_off, uint64_t nframes,
                                                                 int64_t *__restrict__ want)
{
    const uint64_t i = (uint64_t)blockIdx.x * kListT + threadIdx.x;
    if (i < n)
        want[i] = fl_size(idx[i], d_off, nframes);
}

__global__ __launch_bounds__(kCompactT) void frame_list_scan_kernel(const int64_t *__restrict__ idx,
                                                                    const int64_t *__restrict__ want, uint64_t n,
                                                                    const uint64_t *__restrict__ c_off,
                                                                    FrameListHead *__restrict__ head,
                                                                    uint64_t *__restrict__ off,
                                                                    int64_t *__restrict__ result)
{
    __shared__ uint64_t s_sum[kCompactT];
    __shared__ unsigned long long s_lo, s_hi;
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        s_lo = ~0ull;
        s_hi = 0;
    }
    uint64_t a, b, bytes, lo, hi;
    pd_share(n, kCompactT, t, &a, &b);
    fl_share_sum(idx, want, a, b, c_off, &bytes, &lo, &hi);
    // (the scan's first barrier orders s_lo / s_hi's initial values before these)
    const uint64_t packed_end = block_scan_inclusive<kCompactT>(s_sum, t, bytes);
    if (lo <= hi) {
        atomicMin(&s_lo, (unsigned long long)lo);
        atomicMax(&s_hi, (unsigned long long)hi);
    }
    uint64_t packed = packed_end - bytes;
    fl_share_emit(want, a, b, &packed, off);
    __syncthreads();
    if (t == 0) {
        const FrameListHead h = fl_head(s_sum[kCompactT - 1], s_lo, s_hi);
        *head = h;
        off[n] = h.total;
        // the count the result kernel adds to, or the flag it leaves alone
        result[n] = h.flag;
    }
}

__global__ __launch_bounds__(kListT) void frame_list_emit_kernel(const int64_t *__restrict__ idx, uint64_t n,
                                                                 uint64_t stride, uint64_t buf_size, PlanTables T,
                                                                 const FrameListHead *__restrict__ head,
                                                                 const uint64_t *__restrict__ off,
                                                                 int64_t *__restrict__ want,
                                                                 DevFrame *__restrict__ desc,
                                                                 uint32_t *__restrict__ ck,
                                                                 uint64_t *__restrict__ offsets)
{
    const uint64_t i = (uint64_t)blockIdx.x * kListT + threadIdx.x;
    if (i >= n)
        return;
    const FrameListHead h = *head;
    const uint64_t dst = fl_dst(i, stride, off);
    const int64_t w = fl_want(want[i], dst, stride, buf_size, h.flag);
    // (w > 0: fl_size found idx[i] inside the table)
    const uint64_t f = w > 0 ? (uint64_t)idx[i] : 0;
    desc[i] = fl_desc(w, f, dst, T, h);
    if (ck)
        ck[i] = w > 0 ? T.ck[f] : 0;
    want[i] = w;
    if (offsets) {
        offsets[i] = dst;
        if (i == 0)
            offsets[n] = stride ? n * stride : h.total;
    }
}

__global__ __launch_bounds__(kListT) void frame_list_result_kernel(const int64_t *__restrict__ want, uint64_t n,
                                                                   const FrameListHead *__restrict__ head,
                                                                   const int32_t *__restrict__ status,
                                                                   int64_t *__restrict__ result)
{
    const uint64_t i = (uint64_t)blockIdx.x * kListT + threadIdx.x;
    int64_t res = -1;
    if (i < n) {
        res = fl_result(want[i], status[i]);
        result[i] = res;
    }
    // (a flagged call: every want is -1, and result[n] keeps the flag)
    const int delivered = __syncthreads_count(res >= 0);
    if (threadIdx.x == 0 && delivered && !head->flag)
        atomicAdd(reinterpret_cast<unsigned long long *>(result + n), (unsigned long long)delivered);
}

}   // namespace

int launch_frame_list_plan(uint8_t *d_plan, const FrameListLayout &L, const PlanTables &T, const int64_t *d_idx,
                           uint64_t n, uint64_t stride, uint64_t buf_size, uint64_t *d_offsets, int64_t *d_result,
                           hipStream_t stream)
{
    if (!d_plan || !d_idx || !d_result || n == 0 || (!stride && !d_offsets))
        return -1;
    FrameListHead *const head = reinterpret_cast<FrameListHead *>(d_plan + L.head);
    uint64_t *const off = reinterpret_cast<uint64_t *>(d_plan + L.off);
    int64_t *const want = reinterpret_cast<int64_t *>(d_plan + L.want);
    DevFrame *const desc = reinterpret_cast<DevFrame *>(d_plan + L.desc);
    uint32_t *const ck = T.ck ? reinterpret_cast<uint32_t *>(d_plan + L.ck) : nullptr;
    const uint32_t grid = (uint32_t)((n + kListT - 1) / kListT);
    hipLaunchKernelGGL(frame_list_size_kernel, dim3(grid), dim3(kListT), 0, stream, d_idx, n, T.d_off, T.nframes, want);
    hipLaunchKernelGGL(frame_list_scan_kernel, dim3(1), dim3(kCompactT), 0, stream, d_idx, want, n, T.c_off, head, off,
                       d_result);
    hipLaunchKernelGGL(frame_list_emit_kernel, dim3(grid), dim3(kListT), 0, stream, d_idx, n, stride, buf_size, T, head,
                       off, want, desc, ck, d_offsets);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_frame_list_result(const uint8_t *d_plan, const FrameListLayout &L, uint64_t n, const int32_t *d_status,
                             int64_t *d_result, hipStream_t stream)
{
    if (!d_plan || !d_status || !d_result || n == 0)
        return -1;
    const uint32_t grid = (uint32_t)((n + kListT - 1) / kListT);
    hipLaunchKernelGGL(frame_list_result_kernel, dim3(grid), dim3(kListT), 0, stream,
                       reinterpret_cast<const int64_t *>(d_plan + L.want), n,
                       reinterpret_cast<const FrameListHead *>(d_plan + L.head), d_status, d_result);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}   // namespace zsk
