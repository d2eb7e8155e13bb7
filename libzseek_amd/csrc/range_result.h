// Per-range results of a vectored read, computed where the frames' statuses
// are: on the device, behind the decode (zsk_preadv_device_async), with no
// host wait.  range_plan.h's range_results is the host form and the yardstick:
// everything here gives exactly its answers.  No HIP runtime calls and no
// reader state, so tests/native/range_result_shim.cpp drives it on the CPU;
// range_result.hip's kernel and reader_vec.cpp use exactly these.
//
// The device gets a flat table of the call: one RangeRow per range and, per
// touched frame t, t_doff[t] = d_off[P.frames[t]] -- all a result needs beside
// status[t].  A range's result is decided by its FIRST failed touched frame,
// so one wave64 walks the range's touched frames 64 at a time, in order:
// lane l of the chunk at k0 tests frame k0 + l (range_lane_failed), a ballot
// gathers the 64 answers, its lowest set bit is the first failure, and the
// walk stops at the first chunk that has one (range_result_of).  A range over
// a whole file of 60,000 frames is under a thousand wave steps.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "range_plan.h"

#ifdef __HIP__
#define ZSK_RR_HD __host__ __device__
#else
#define ZSK_RR_HD
#endif

namespace zsk {

struct RangeRow {
    uint64_t offset;   // the range's decoded offset
    uint64_t full;     // bytes a clean read delivers: range_end - offset (0 when rtn == 0)
    uint64_t rt0;      // its touched frames: [rt0, rt0 + rtn) of the call's list
    uint64_t rtn;
};
static_assert(sizeof(RangeRow) == 32, "RangeRow is uploaded as is");

struct RangeTable {
    std::vector<RangeRow> rows;     // per range
    std::vector<uint64_t> t_doff;   // per touched frame: its decoded offset in the file
};

constexpr uint32_t kResultLanes = 64;   // lanes of a walk's chunk: one wave
constexpr uint64_t kNoBad = ~0ull;      // no failed frame in the range

inline RangeTable build_range_table(const RangePlan &P, const RangeReq *rg, size_t n, const uint64_t *d_off,
                                    size_t nframes)
{
    RangeTable T;
    const uint64_t size = nframes ? d_off[nframes] : 0;
    T.rows.resize(n);
    for (size_t r = 0; r < n; r++)
        T.rows[r] = {rg[r].offset, P.rtn[r] ? range_end(rg[r], size) - rg[r].offset : 0, P.rt0[r], P.rtn[r]};
    T.t_doff.resize(P.frames.size());
    for (size_t t = 0; t < P.frames.size(); t++)
        T.t_doff[t] = d_off[P.frames[t]];
    return T;
}

// Lane `lane` of the chunk that starts at the range's k0-th touched frame: is
// its frame inside the range and failed?  (k0 advances by the lane count.)
ZSK_RR_HD inline bool range_lane_failed(const RangeRow &row, const int32_t *status, uint64_t k0, uint32_t lane)
{
    const uint64_t k = k0 + lane;
    return k < row.rtn && status[row.rt0 + k] != 0;
}

// The range's result from bad_k, the index within the range of its first
// failed touched frame (kNoBad: none); *full: delivered in full.
ZSK_RR_HD inline int64_t range_result_of(const RangeRow &row, const uint64_t *t_doff, uint64_t bad_k, bool *full)
{
    *full = bad_k == kNoBad;
    if (!row.rtn)
        return 0;
    if (bad_k == kNoBad)
        return (int64_t)row.full;
    if (bad_k == 0)
        return -1;
    return (int64_t)(t_doff[row.rt0 + bad_k] - row.offset);
}

// The kernel's walk with the wave spelled out as a loop over its lanes (the
// ballot is the inner loop): every range's result and the count of ranges
// delivered in full, as range_result_kernel leaves them in d_result.
inline size_t range_results_lanes(const RangeTable &T, const int32_t *status, int64_t *result)
{
    size_t ok = 0;
    for (size_t r = 0; r < T.rows.size(); r++) {
        const RangeRow &row = T.rows[r];
        uint64_t bad = kNoBad;
        for (uint64_t k0 = 0; k0 < row.rtn && bad == kNoBad; k0 += kResultLanes) {
            uint64_t ballot = 0;
            for (uint32_t lane = 0; lane < kResultLanes; lane++)
                ballot |= (uint64_t)range_lane_failed(row, status, k0, lane) << lane;
            if (ballot)
                bad = k0 + (uint64_t)__builtin_ctzll(ballot);
        }
        bool full;
        result[r] = range_result_of(row, T.t_doff.data(), bad, &full);
        ok += full;
    }
    return ok;
}

}   // namespace zsk
