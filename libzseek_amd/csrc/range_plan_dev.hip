// range_plan_dev.hip — the device plan of zsk_preadv_device_indirect (gfx950):
// range_plan_dev.h's four steps as kernels.  The range list is read from device
// memory on the caller's stream, the seek table is the reader's resident copy,
// and everything the plan produces -- descriptors, rows, segments, the checks'
// flag -- stays on the device: the host sizes the grids by its bounds
// (nranges, max_frames) and learns no count.
//
//   plan_touch_kernel     thread per range
//   plan_compact_kernel   one workgroup of kCompactT threads (block_scan.h)
//   plan_segments_kernel  thread per range
//   plan_fix_kernel       thread per range, behind range_result_kernel
//
// Plain vector loads, stores and atomics only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stddef.h>

#include "block_scan.h"
#include "range_plan_dev.h"
#include "zsk_internal.h"

namespace zsk {

static_assert(sizeof(DevRange) == sizeof(zsk_range_t) && offsetof(DevRange, dst_off) == offsetof(zsk_range_t, dst_off),
              "range ABI");
static_assert(sizeof(DevFrame) == sizeof(FrameDesc) && offsetof(DevFrame, c_size) == offsetof(FrameDesc, c_size),
              "descriptor ABI");
static_assert(sizeof(DevSeg) == sizeof(GatherSeg) && offsetof(DevSeg, len) == offsetof(GatherSeg, len), "segment ABI");

namespace {

constexpr uint32_t kPlanT = 256;   // threads per workgroup of the per-range kernels

__global__ __launch_bounds__(kPlanT) void plan_touch_kernel(const DevRange *__restrict__ rg, uint64_t n,
                                                            const uint64_t *__restrict__ d_off, uint64_t nframes,
                                                            uint64_t buf_size, RangeRow *__restrict__ rows,
                                                            uint64_t *__restrict__ dst, uint32_t *bitmap)
{
    const uint64_t r = (uint64_t)blockIdx.x * kPlanT + threadIdx.x;
    if (r >= n)
        return;
    const DevRange q = rg[r];
    const RangeRow row = pd_touch(q, d_off, nframes, buf_size);
    rows[r] = row;
    dst[r] = q.dst_off;
    if (row.rtn)
        pd_mark(row.rt0, row.rt0 + row.rtn - 1, [&](uint64_t w, uint32_t m) { atomicOr(&bitmap[w], m); });
}

__global__ __launch_bounds__(kCompactT) void plan_compact_kernel(PlanTables T, const uint32_t *__restrict__ bitmap,
                                                                 uint64_t words, uint64_t max_frames,
                                                                 PlanHead *__restrict__ head,
                                                                 uint32_t *__restrict__ wrank,
                                                                 DevFrame *__restrict__ desc,
                                                                 uint64_t *__restrict__ t_doff,
                                                                 uint32_t *__restrict__ ck)
{
    __shared__ uint64_t s_sum[kCompactT];
    __shared__ uint64_t s_first, s_last, s_pad;
    __shared__ int64_t s_flag;
    const uint32_t t = threadIdx.x;
    uint64_t wa, wb;
    pd_share(words, kCompactT, t, &wa, &wb);
    // this thread's share of the bitmap: its set frames, their decoded bytes,
    // the first and the last of them
    uint64_t count = 0, bytes = 0, first = 0, last = 0;
    for (uint64_t w = wa; w < wb; w++) {
        const uint32_t word = bitmap[w];
        if (!word)
            continue;
        if (!count)
            first = 32 * w + (uint32_t)__builtin_ctz(word);
        last = 32 * w + 31 - (uint32_t)__builtin_clz(word);
        pd_word_sum(word, w, T.d_off, &count, &bytes);
    }
    const uint64_t rank_end = block_scan_inclusive<kCompactT>(s_sum, t, count);
    const uint64_t touched = s_sum[kCompactT - 1];
    __syncthreads();
    const uint64_t packed_end = block_scan_inclusive<kCompactT>(s_sum, t, bytes);
    const uint64_t total_bytes = s_sum[kCompactT - 1];
    // (exactly one thread holds the first touched frame, one the last)
    if (count && rank_end == count)
        s_first = first;
    if (count && rank_end == touched)
        s_last = last;
    __syncthreads();
    if (t == 0) {
        const uint64_t span = touched ? T.c_off[s_last + 1] - T.c_off[s_first] : 0;
        const int64_t flag = pd_flag(touched, max_frames, span);
        s_flag = flag;
        s_pad = touched && !flag ? T.c_off[s_first] : 0;
        *head = PlanHead{touched, total_bytes, span, flag};
    }
    __syncthreads();
    const int64_t flag = s_flag;
    if (!flag) {
        uint64_t rank = rank_end - count, packed = packed_end - bytes;
        for (uint64_t w = wa; w < wb; w++) {
            wrank[w] = (uint32_t)rank;
            pd_word_emit(bitmap[w], w, &rank, &packed, T, desc, t_doff, ck);
        }
    }
    // a flagged call decodes nothing: every descriptor is padding
    for (uint64_t i = (flag ? 0 : touched) + t; i < max_frames; i += kCompactT) {
        desc[i] = pd_padding(T, s_pad);
        t_doff[i] = 0;
        if (ck)
            ck[i] = 0;
    }
}

__global__ __launch_bounds__(kPlanT) void plan_segments_kernel(RangeRow *__restrict__ rows, uint64_t n,
                                                               const uint64_t *__restrict__ dst,
                                                               const PlanHead *__restrict__ head,
                                                               const uint32_t *__restrict__ bitmap,
                                                               const uint32_t *__restrict__ wrank,
                                                               const uint64_t *__restrict__ d_off,
                                                               const DevFrame *__restrict__ desc,
                                                               DevSeg *__restrict__ segs)
{
    const uint64_t r = (uint64_t)blockIdx.x * kPlanT + threadIdx.x;
    if (r >= n)
        return;
    RangeRow row = rows[r];
    const uint64_t fa = row.rt0;
    row.rt0 = 0;
    if (head->flag)
        row.rtn = 0;   // (a segment of no bytes, and no status for range_result_kernel to look at)
    else if (row.rtn)
        row.rt0 = pd_rank(bitmap, wrank, fa);
    rows[r] = row;
    segs[r] = pd_segment(row, fa, dst[r], d_off, desc);
}

__global__ __launch_bounds__(kPlanT) void plan_fix_kernel(const RangeRow *__restrict__ rows, uint64_t n,
                                                          const PlanHead *__restrict__ head, int64_t *result)
{
    const uint64_t r = (uint64_t)blockIdx.x * kPlanT + threadIdx.x;
    if (r >= n)
        return;
    const int64_t flag = head->flag;
    bool uncount;
    const int64_t res = pd_fix(rows[r], flag, 0, &uncount);
    if (res < 0)
        result[r] = -1;
    if (uncount)
        atomicAdd(reinterpret_cast<unsigned long long *>(result + n), ~0ull);   // - 1
    // (a flagged call: no range is uncounted, this is the only write)
    if (flag && r == 0)
        result[n] = flag;
}

}   // namespace

int launch_indirect_plan(uint8_t *d_plan, const PlanLayout &L, const PlanTables &T, const void *d_ranges, uint64_t n,
                         uint64_t buf_size, uint64_t max_frames, hipStream_t stream)
{
    if (!d_plan || !d_ranges || n == 0 || max_frames == 0)
        return -1;
    if (hipMemsetAsync(d_plan, 0, L.zero_end, stream) != hipSuccess)
        return -1;
    PlanHead *const head = reinterpret_cast<PlanHead *>(d_plan + L.head);
    uint32_t *const bitmap = reinterpret_cast<uint32_t *>(d_plan + L.bitmap);
    uint32_t *const wrank = reinterpret_cast<uint32_t *>(d_plan + L.wrank);
    RangeRow *const rows = reinterpret_cast<RangeRow *>(d_plan + L.rows);
    uint64_t *const dst = reinterpret_cast<uint64_t *>(d_plan + L.dst);
    DevFrame *const desc = reinterpret_cast<DevFrame *>(d_plan + L.desc);
    uint64_t *const t_doff = reinterpret_cast<uint64_t *>(d_plan + L.t_doff);
    uint32_t *const ck = T.ck ? reinterpret_cast<uint32_t *>(d_plan + L.ck) : nullptr;
    const uint32_t grid = (uint32_t)((n + kPlanT - 1) / kPlanT);
    hipLaunchKernelGGL(plan_touch_kernel, dim3(grid), dim3(kPlanT), 0, stream, static_cast<const DevRange *>(d_ranges),
                       n, T.d_off, T.nframes, buf_size, rows, dst, bitmap);
    hipLaunchKernelGGL(plan_compact_kernel, dim3(1), dim3(kCompactT), 0, stream, T, bitmap, L.words, max_frames, head,
                       wrank, desc, t_doff, ck);
    hipLaunchKernelGGL(plan_segments_kernel, dim3(grid), dim3(kPlanT), 0, stream, rows, n, dst, head, bitmap, wrank,
                       T.d_off, desc, reinterpret_cast<DevSeg *>(d_plan + L.segs));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_indirect_fix(const uint8_t *d_plan, const PlanLayout &L, uint64_t n, int64_t *d_result, hipStream_t stream)
{
    if (!d_plan || !d_result || n == 0)
        return -1;
    const uint32_t grid = (uint32_t)((n + kPlanT - 1) / kPlanT);
    hipLaunchKernelGGL(plan_fix_kernel, dim3(grid), dim3(kPlanT), 0, stream,
                       reinterpret_cast<const RangeRow *>(d_plan + L.rows), n,
                       reinterpret_cast<const PlanHead *>(d_plan + L.head), d_result);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}   // namespace zsk
