// Test-only C shim over libzseek_amd/csrc/range_result.h (pure functions, no
// HIP): tests/test_range_result.py builds it with g++ and calls it via ctypes.
// rr_lanes drives the shared result functions the way range_result_kernel
// does (64 lanes per range, chunk by chunk, early exit); rr_host is
// range_plan.h's range_results, the yardstick.
#include "../../libzseek_amd/csrc/range_result.h"

using namespace zsk;

extern "C" {

// ranges: n x (offset, count, dst_off); frames by their decoded offsets
// d_off[0..nframes]
void *rr_plan(const uint64_t *ranges, size_t n, const uint64_t *d_off, size_t nframes, uint64_t batch_bytes)
{
    static_assert(sizeof(RangeReq) == 24, "three u64");
    return new RangePlan(plan_ranges(reinterpret_cast<const RangeReq *>(ranges), n, d_off, nframes, batch_bytes));
}

void rr_free(void *p) { delete static_cast<RangePlan *>(p); }

size_t rr_touched(void *p) { return static_cast<RangePlan *>(p)->frames.size(); }

size_t rr_batches(void *p) { return static_cast<RangePlan *>(p)->batches.size(); }

// the flat table: per range offset, full, rt0, rtn (rows: 4 n u64); per
// touched frame its decoded offset (t_doff)
void rr_table(void *p, const uint64_t *ranges, size_t n, const uint64_t *d_off, size_t nframes, uint64_t *rows,
              uint64_t *t_doff)
{
    const RangeTable T = build_range_table(*static_cast<RangePlan *>(p), reinterpret_cast<const RangeReq *>(ranges), n,
                                           d_off, nframes);
    for (size_t r = 0; r < n; r++) {
        const uint64_t v[4] = {T.rows[r].offset, T.rows[r].full, T.rows[r].rt0, T.rows[r].rtn};
        std::copy(v, v + 4, rows + 4 * r);
    }
    std::copy(T.t_doff.begin(), T.t_doff.end(), t_doff);
}

// status: one per touched frame; results: one per range; returns the ranges
// delivered in full -- the kernel's walk
size_t rr_lanes(void *p, const uint64_t *ranges, size_t n, const uint64_t *d_off, size_t nframes,
                const int32_t *status, int64_t *results)
{
    const RangeTable T = build_range_table(*static_cast<RangePlan *>(p), reinterpret_cast<const RangeReq *>(ranges), n,
                                           d_off, nframes);
    return range_results_lanes(T, status, results);
}

// ... and the host's loop
size_t rr_host(void *p, const uint64_t *ranges, size_t n, const uint64_t *d_off, size_t nframes, const int32_t *status,
               int64_t *results)
{
    return range_results(*static_cast<RangePlan *>(p), reinterpret_cast<const RangeReq *>(ranges), n, d_off, nframes,
                         status, results);
}
}
