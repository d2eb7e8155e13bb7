// Test-only C shim over libzseek_amd/csrc/range_plan_dev.h (pure functions, no
// HIP): tests/test_range_plan_dev.py builds it with g++ and calls it via
// ctypes.  pd_run drives the shared plan functions the way the kernels of
// range_plan_dev.hip do (plan_dev_lanes: a thread per range, the compact
// workgroup's 1,024 shares and scans); ref_* is range_plan.h's plan_ranges,
// range_result.h's build_range_table and range_results -- the yardstick.
#include "../../libzseek_amd/csrc/range_plan_dev.h"

#include <algorithm>

using namespace zsk;

namespace {
struct Ref {
    RangePlan P;
    RangeTable T;
};
}   // namespace

extern "C" {

// ranges: n x (offset, count, dst_off, result); ck may be NULL
void *pd_run(const uint64_t *ranges, size_t n, const uint64_t *c_off, const uint64_t *d_off, const uint32_t *ck,
             size_t nframes, uint64_t bias, uint64_t buf_size, uint64_t max_frames)
{
    static_assert(sizeof(DevRange) == 32, "four 8-byte fields");
    const PlanTables T{c_off, d_off, ck, nframes, bias};
    return new DevPlan(plan_dev_lanes(reinterpret_cast<const DevRange *>(ranges), n, T, buf_size, max_frames));
}

void pd_free(void *p) { delete static_cast<DevPlan *>(p); }

// touched, bytes, span, flag
void pd_head(void *p, int64_t *out)
{
    const PlanHead &h = static_cast<DevPlan *>(p)->head;
    out[0] = (int64_t)h.touched;
    out[1] = (int64_t)h.bytes;
    out[2] = (int64_t)h.span;
    out[3] = h.flag;
}

size_t pd_seg_cap(void *p) { return static_cast<DevPlan *>(p)->segs.size(); }

// rows: 4 n u64 (offset, full, rt0, rtn)
void pd_rows(void *p, uint64_t *rows)
{
    const DevPlan &P = *static_cast<DevPlan *>(p);
    for (size_t r = 0; r < P.rows.size(); r++) {
        const uint64_t v[4] = {P.rows[r].offset, P.rows[r].full, P.rows[r].rt0, P.rows[r].rtn};
        std::copy(v, v + 4, rows + 4 * r);
    }
}

// per descriptor (max_frames of them): c_off, d_off, c_size, d_size, t_doff, ck
void pd_frames(void *p, uint64_t *out)
{
    const DevPlan &P = *static_cast<DevPlan *>(p);
    for (size_t t = 0; t < P.desc.size(); t++) {
        const uint64_t v[6] = {P.desc[t].c_off, P.desc[t].d_off, P.desc[t].c_size, P.desc[t].d_size, P.t_doff[t],
                               P.ck.empty() ? 0 : P.ck[t]};
        std::copy(v, v + 6, out + 6 * t);
    }
}

// per segment (one per range): src_off, dst_off, len, frame
void pd_segs(void *p, uint64_t *out)
{
    const DevPlan &P = *static_cast<DevPlan *>(p);
    for (size_t i = 0; i < P.segs.size(); i++) {
        const uint64_t v[4] = {P.segs[i].src_off, P.segs[i].dst_off, P.segs[i].len, P.segs[i].frame};
        std::copy(v, v + 4, out + 4 * i);
    }
}

// status: max_frames words; results: n + 1
void pd_results(void *p, const int32_t *status, int64_t *results)
{
    plan_dev_results(*static_cast<DevPlan *>(p), status, results);
}

// ---- the yardstick: ranges as n x (offset, count, dst_off), one batch ----
void *ref_plan(const uint64_t *ranges, size_t n, const uint64_t *d_off, size_t nframes)
{
    Ref *R = new Ref();
    const RangeReq *rq = reinterpret_cast<const RangeReq *>(ranges);
    R->P = plan_ranges(rq, n, d_off, nframes, ~0ull);
    R->T = build_range_table(R->P, rq, n, d_off, nframes);
    return R;
}

void ref_free(void *p) { delete static_cast<Ref *>(p); }

size_t ref_touched(void *p) { return static_cast<Ref *>(p)->P.frames.size(); }
size_t ref_nsegs(void *p) { return static_cast<Ref *>(p)->P.segs.size(); }
size_t ref_batches(void *p) { return static_cast<Ref *>(p)->P.batches.size(); }

void ref_get(void *p, uint64_t *frames, uint64_t *rows, uint64_t *t_doff, uint64_t *segs)
{
    const Ref &R = *static_cast<Ref *>(p);
    for (size_t t = 0; t < R.P.frames.size(); t++) {
        frames[t] = R.P.frames[t];
        t_doff[t] = R.T.t_doff[t];
    }
    for (size_t r = 0; r < R.T.rows.size(); r++) {
        const uint64_t v[4] = {R.T.rows[r].offset, R.T.rows[r].full, R.T.rows[r].rt0, R.T.rows[r].rtn};
        std::copy(v, v + 4, rows + 4 * r);
    }
    for (size_t i = 0; i < R.P.segs.size(); i++) {   // src_off, dst_off, len, frame, range
        const PlanSeg &s = R.P.segs[i];
        const uint64_t v[5] = {s.src_off, s.dst_off, s.len, s.frame, s.range};
        std::copy(v, v + 5, segs + 5 * i);
    }
}

size_t ref_results(void *p, const uint64_t *ranges, size_t n, const uint64_t *d_off, size_t nframes,
                   const int32_t *status, int64_t *results)
{
    return range_results(static_cast<Ref *>(p)->P, reinterpret_cast<const RangeReq *>(ranges), n, d_off, nframes,
                         status, results);
}
}
