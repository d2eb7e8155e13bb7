// Test-only C shim over libzseek_amd/csrc/frame_list_plan.h (pure functions, no
// HIP): tests/test_frame_list_plan.py builds it with g++ and calls it via
// ctypes.  fl_run drives the shared plan functions the way the kernels of
// frame_list_plan.hip do (frame_list_lanes: a thread per slot, the scan
// workgroup's 1,024 shares); the yardstick is the test's own numpy arithmetic.
#include "../../libzseek_amd/csrc/frame_list_plan.h"

#include <algorithm>

using namespace zsk;

extern "C" {

// ck may be NULL
void *fl_run(const int64_t *idx, size_t n, uint64_t stride, uint64_t buf_size, const uint64_t *c_off,
             const uint64_t *d_off, const uint32_t *ck, size_t nframes, uint64_t bias)
{
    const PlanTables T{c_off, d_off, ck, nframes, bias};
    return new FrameListPlan(frame_list_lanes(idx, n, stride, buf_size, T));
}

void fl_free(void *p) { delete static_cast<FrameListPlan *>(p); }

// head: total, c_lo, span, flag; off / offsets: n + 1; want: n; desc: n x
// (c_off, d_off, c_size, d_size); ck: n (NULL when the run had none)
void fl_get(void *p, int64_t *head, uint64_t *off, uint64_t *offsets, int64_t *want, uint64_t *desc, uint32_t *ck)
{
    const FrameListPlan &P = *static_cast<FrameListPlan *>(p);
    head[0] = (int64_t)P.head.total;
    head[1] = (int64_t)P.head.c_lo;
    head[2] = (int64_t)P.head.span;
    head[3] = P.head.flag;
    std::copy(P.off.begin(), P.off.end(), off);
    std::copy(P.offsets.begin(), P.offsets.end(), offsets);
    std::copy(P.want.begin(), P.want.end(), want);
    for (size_t i = 0; i < P.desc.size(); i++) {
        const uint64_t v[4] = {P.desc[i].c_off, P.desc[i].d_off, P.desc[i].c_size, P.desc[i].d_size};
        std::copy(v, v + 4, desc + 4 * i);
    }
    if (ck)
        std::copy(P.ck.begin(), P.ck.end(), ck);
}

// result: n + 1
void fl_results(void *p, const int32_t *status, int64_t *result)
{
    frame_list_results(*static_cast<FrameListPlan *>(p), status, result);
}

// the layout of the call's device buffer: head, off, want, desc, ck, total
void fl_layout(uint64_t n, int ck, uint64_t *out)
{
    const FrameListLayout L = frame_list_layout(n, ck != 0);
    const uint64_t v[6] = {L.head, L.off, L.want, L.desc, L.ck, L.total};
    std::copy(v, v + 6, out);
}

uint64_t fl_span_limit() { return kPlanSpanLimit; }

}   // extern "C"
