// Test-only C shim over libzseek_amd/csrc/range_plan.h (pure functions, no
// HIP): tests/test_range_plan.py builds it with g++ and calls it via ctypes.
#include "../../libzseek_amd/csrc/range_plan.h"

using namespace zsk;

extern "C" {

// ranges: n x (offset, count, dst_off); frames by their decoded offsets
// d_off[0..nframes]
void *rp_plan(const uint64_t *ranges, size_t n, const uint64_t *d_off, size_t nframes, uint64_t batch_bytes)
{
    static_assert(sizeof(RangeReq) == 24, "three u64");
    return new RangePlan(plan_ranges(reinterpret_cast<const RangeReq *>(ranges), n, d_off, nframes, batch_bytes));
}

void rp_free(void *p) { delete static_cast<RangePlan *>(p); }

// what: 0 frames, 1 runs, 2 batches, 3 segments
size_t rp_count(void *p, int what)
{
    const RangePlan &P = *static_cast<RangePlan *>(p);
    return what == 0 ? P.frames.size() : what == 1 ? P.runs.size() : what == 2 ? P.batches.size() : P.segs.size();
}

void rp_frames(void *p, uint64_t *out)
{
    const RangePlan &P = *static_cast<RangePlan *>(p);
    for (size_t i = 0; i < P.frames.size(); i++)
        out[i] = P.frames[i];
}

// per run: f0, f1
void rp_runs(void *p, uint64_t *out)
{
    const RangePlan &P = *static_cast<RangePlan *>(p);
    for (size_t i = 0; i < P.runs.size(); i++) {
        out[2 * i] = P.runs[i].f0;
        out[2 * i + 1] = P.runs[i].f1;
    }
}

// per batch: t0, t1, r0, r1, s0, s1, d_bytes, out_bytes
void rp_batches(void *p, uint64_t *out)
{
    const RangePlan &P = *static_cast<RangePlan *>(p);
    for (size_t i = 0; i < P.batches.size(); i++) {
        const PlanBatch &b = P.batches[i];
        const uint64_t v[8] = {b.t0, b.t1, b.r0, b.r1, b.s0, b.s1, b.d_bytes, b.out_bytes};
        std::copy(v, v + 8, out + 8 * i);
    }
}

// per segment: src_off, dst_off, len, frame (within its batch), range, and its
// entry of the batch's length prefix sum (the bytes of the batch's segments
// before it)
void rp_segs(void *p, uint64_t *out)
{
    const RangePlan &P = *static_cast<RangePlan *>(p);
    for (size_t bi = 0; bi < P.batches.size(); bi++)
        for (size_t s = P.batches[bi].s0; s < P.batches[bi].s1; s++) {
            const PlanSeg &g = P.segs[s];
            const uint64_t v[6] = {g.src_off, g.dst_off, g.len, g.frame, g.range, P.cum[s + bi]};
            std::copy(v, v + 6, out + 6 * s);
        }
}

// status: one per touched frame; results: one per range; returns the ranges
// delivered in full
size_t rp_results(void *p, const uint64_t *ranges, size_t n, const uint64_t *d_off, size_t nframes,
                  const int32_t *status, int64_t *results)
{
    return range_results(*static_cast<RangePlan *>(p), reinterpret_cast<const RangeReq *>(ranges), n, d_off, nframes,
                         status, results);
}
}
