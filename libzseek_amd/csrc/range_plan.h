// Pure planning of a vectored read (zsk_preadv): which frames the ranges
// touch, how those frames are read (runs of adjacent frames, one pread
// callback each) and decoded (batches of at most batch_bytes decoded bytes, in
// frame order, their compressed and decoded bytes packed back to back), and
// the (range, frame) overlaps -- the segments the gather kernel moves
// (range_gather.hip).  No HIP and no reader state, so
// tests/native/range_plan_shim.cpp unit-tests it on the CPU; reader_vec.cpp
// uses exactly these.
//
// Replaces a caller's loop of zseek_pread calls over scattered ranges (the
// reference has no vectored read: decompress.c:806-824 takes one range).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace zsk {

struct RangeReq {
    uint64_t offset, count, dst_off;   // zsk_range_t's input fields
};

// One (range, frame) overlap.
struct PlanSeg {
    uint64_t src_off;   // in the batch's packed decoded staging
    uint64_t dst_off;   // in the caller's buffer
    uint32_t len;
    uint32_t frame;     // the frame's index within its batch
    uint32_t range;
};

struct PlanRun {
    size_t f0, f1;   // file frames [f0, f1): adjacent, one pread
};

// Everything below indexes RangePlan's vectors: t* its touched frames,
// r* its runs, s* its segments.
struct PlanBatch {
    size_t t0, t1, r0, r1, s0, s1;
    uint64_t d_bytes;     // decoded bytes of its frames
    uint64_t out_bytes;   // bytes its segments move
};

struct RangePlan {
    std::vector<size_t> frames;       // touched file frames, sorted, each once
    std::vector<PlanRun> runs;        // in frame order; a run never crosses a batch
    std::vector<PlanBatch> batches;
    std::vector<PlanSeg> segs;        // grouped by batch
    // batch b's segment length prefix sum: cum[s0 + b .. s1 + b] (s1 - s0 + 1
    // entries, the first 0, the last out_bytes)
    std::vector<uint64_t> cum;
    // a range's frames are consecutive file frames, so consecutive touched
    // ones: [rt0[r], rt0[r] + rtn[r]) (rtn 0: zero-length or at / past EOF)
    std::vector<size_t> rt0, rtn;
};

// The frame holding decoded byte x (x < d_off[nframes]): the last frame that
// starts at or before x (zero-size frames are skipped, as SeekTable::frame_of).
inline size_t plan_frame_of(const uint64_t *d_off, size_t nframes, uint64_t x)
{
    return (size_t)(std::upper_bound(d_off, d_off + nframes + 1, x) - d_off) - 1;
}

inline uint64_t range_end(const RangeReq &q, uint64_t size)
{
    return q.count < size - q.offset ? q.offset + q.count : size;   // (offset < size)
}

// c_off / span_limit (optional; a reader over a device image, whose frames are
// decoded where they lie instead of packed): a batch also ends where the
// compressed distance from its first frame's start to a frame's end would
// exceed span_limit (a frame longer than that is a batch of its own).
inline RangePlan plan_ranges(const RangeReq *rg, size_t n, const uint64_t *d_off, size_t nframes,
                             uint64_t batch_bytes, const uint64_t *c_off = nullptr, uint64_t span_limit = 0)
{
    RangePlan P;
    P.rt0.assign(n, 0);
    P.rtn.assign(n, 0);
    const uint64_t size = nframes ? d_off[nframes] : 0;
    std::vector<std::pair<size_t, size_t>> span(n), iv;   // per range [first, last] frame
    for (size_t r = 0; r < n; r++) {
        if (rg[r].count == 0 || rg[r].offset >= size)
            continue;
        const size_t fa = plan_frame_of(d_off, nframes, rg[r].offset);
        const size_t fb = plan_frame_of(d_off, nframes, range_end(rg[r], size) - 1);
        span[r] = {fa, fb};
        P.rtn[r] = fb - fa + 1;
        iv.push_back({fa, fb});
    }
    if (iv.empty())
        return P;
    // touched frames: the union of the ranges' frame intervals
    std::sort(iv.begin(), iv.end());
    size_t m = 0;
    for (size_t i = 1; i < iv.size(); i++) {
        if (iv[i].first <= iv[m].second + 1)
            iv[m].second = std::max(iv[m].second, iv[i].second);
        else
            iv[++m] = iv[i];
    }
    iv.resize(m + 1);
    for (const auto &v : iv)
        for (size_t f = v.first; f <= v.second; f++)
            P.frames.push_back(f);
    const size_t T = P.frames.size();
    for (size_t r = 0; r < n; r++)
        if (P.rtn[r])
            P.rt0[r] = (size_t)(std::lower_bound(P.frames.begin(), P.frames.end(), span[r].first) - P.frames.begin());
    // batches in frame order (a frame bigger than batch_bytes is a batch of its
    // own); runs break where frames are not adjacent and at batch ends
    std::vector<size_t> batch_of(T);
    std::vector<uint64_t> packed(T);   // the frame's decoded offset within its batch
    for (size_t t = 0; t < T;) {
        PlanBatch b{};
        b.t0 = t;
        b.r0 = P.runs.size();
        while (t < T) {
            const uint64_t d = d_off[P.frames[t] + 1] - d_off[P.frames[t]];
            if (t > b.t0 && b.d_bytes + d > batch_bytes)
                break;
            if (t > b.t0 && c_off && c_off[P.frames[t] + 1] - c_off[P.frames[b.t0]] > span_limit)
                break;
            if (t == b.t0 || P.frames[t] != P.frames[t - 1] + 1)
                P.runs.push_back({P.frames[t], P.frames[t] + 1});
            else
                P.runs.back().f1++;
            batch_of[t] = P.batches.size();
            packed[t] = b.d_bytes;
            b.d_bytes += d;
            t++;
        }
        b.t1 = t;
        b.r1 = P.runs.size();
        P.batches.push_back(b);
    }
    // segments, grouped by batch (counting sort), in range order within one
    std::vector<size_t> fill(P.batches.size() + 1, 0);
    for (size_t r = 0; r < n; r++) {
        const uint64_t end = P.rtn[r] ? range_end(rg[r], size) : 0;
        for (size_t k = 0; k < P.rtn[r]; k++) {
            const size_t f = span[r].first + k;
            if (std::min(end, d_off[f + 1]) > std::max(rg[r].offset, d_off[f]))
                fill[batch_of[P.rt0[r] + k] + 1]++;
        }
    }
    for (size_t b = 0; b < P.batches.size(); b++) {
        P.batches[b].s0 = fill[b];
        fill[b + 1] += fill[b];
        P.batches[b].s1 = fill[b + 1];
    }
    P.segs.resize(fill.back());
    for (size_t r = 0; r < n; r++) {
        const uint64_t end = P.rtn[r] ? range_end(rg[r], size) : 0;
        for (size_t k = 0; k < P.rtn[r]; k++) {
            const size_t f = span[r].first + k, t = P.rt0[r] + k;
            const uint64_t lo = std::max(rg[r].offset, d_off[f]), hi = std::min(end, d_off[f + 1]);
            if (hi <= lo)
                continue;   // (a zero-size frame inside the range)
            const PlanBatch &b = P.batches[batch_of[t]];
            PlanSeg &s = P.segs[fill[batch_of[t]]++];
            s.src_off = packed[t] + (lo - d_off[f]);
            s.dst_off = rg[r].dst_off + (lo - rg[r].offset);
            s.len = (uint32_t)(hi - lo);
            s.frame = (uint32_t)(t - b.t0);
            s.range = (uint32_t)r;
        }
    }
    P.cum.resize(P.segs.size() + P.batches.size());
    for (size_t bi = 0; bi < P.batches.size(); bi++) {
        PlanBatch &b = P.batches[bi];
        uint64_t run = 0;
        P.cum[b.s0 + bi] = 0;
        for (size_t s = b.s0; s < b.s1; s++) {
            run += P.segs[s].len;
            P.cum[s + bi + 1] = run;
        }
        b.out_bytes = run;
    }
    return P;
}

// Per-range results from the touched frames' statuses (status[t] for
// P.frames[t], 0 = decoded): the bytes before the range's first failed frame,
// -1 when that frame is its first, 0 for an empty range.  bad_t (optional):
// the touched index of each range's first failed frame, SIZE_MAX when none.
// Returns the number of ranges delivered in full (result == min(count, size -
// offset), empty ranges included).
inline size_t range_results(const RangePlan &P, const RangeReq *rg, size_t n, const uint64_t *d_off, size_t nframes,
                            const int32_t *status, int64_t *result, size_t *bad_t = nullptr)
{
    const uint64_t size = nframes ? d_off[nframes] : 0;
    size_t ok = 0;
    for (size_t r = 0; r < n; r++) {
        size_t bad = SIZE_MAX;
        for (size_t t = P.rt0[r]; t < P.rt0[r] + P.rtn[r]; t++)
            if (status[t] != 0) {
                bad = t;
                break;
            }
        if (bad_t)
            bad_t[r] = bad;
        if (!P.rtn[r])
            result[r] = 0;
        else if (bad == SIZE_MAX)
            result[r] = (int64_t)(range_end(rg[r], size) - rg[r].offset);
        else if (bad == P.rt0[r])
            result[r] = -1;
        else
            result[r] = (int64_t)(d_off[P.frames[bad]] - rg[r].offset);
        ok += bad == SIZE_MAX;
    }
    return ok;
}

}   // namespace zsk
