// The plan of a vectored read whose range list is in DEVICE memory
// (zsk_preadv_device_indirect): range_plan.h's plan_ranges and range_result.h's
// build_range_table, computed where the ranges are, from the seek table a
// device-image reader keeps resident (DeviceImage::d_coff / d_doff / d_ck).
// range_plan.h is the host form and the yardstick: for ranges the call accepts,
// everything here gives exactly its touched list, rows and segments (one
// batch).  No HIP runtime calls and no reader state, so
// tests/native/range_plan_dev_shim.cpp drives it on the CPU, lane by lane
// (plan_dev_lanes below spells the kernels out as loops over their threads);
// range_plan_dev.hip's kernels use exactly these functions.
//
// Four steps, every grid sized by host bounds (nranges, max_frames), every
// true count left on the device:
//
//   touch     thread per range: the range's first and last file frame by
//             bisection of d_doff (plan_frame_of's rule), its row with rt0 =
//             the first FILE frame for now, and bits fa..fb set in a bitmap of
//             one bit per file frame (whole words for long runs);
//   compact   one workgroup: a scan of the bitmap's popcounts and of the set
//             frames' decoded sizes gives every touched frame its rank t (file
//             order) and its packed staging offset -> FrameDesc[t], t_doff[t],
//             the checksum word of t, a per-word rank table; the checks
//             (more touched frames than max_frames, a compressed span of
//             2 GiB) end in one flag; descriptors [T, max_frames) become
//             padding (c_size 0, d_size 0);
//   segments  thread per range: rt0 from the rank table, and the range's ONE
//             segment;
//   fix       after range_result_kernel: a flagged call's results are all -1
//             and the count the flag; a range whose destination is outside the
//             caller's buffer gets -1 and leaves the count.
//
// One segment per range, nranges slots, whatever the ranges share: a range
// touches every frame from its first to its last, so those frames have
// consecutive ranks and lie back to back in the packed staging -- the range's
// bytes are one contiguous piece there.  plan_ranges cuts that piece at frame
// boundaries (one segment per (range, frame) overlap) so that the gather can
// skip the part of a failed frame; a list in device memory cannot be sized
// that way (overlapping ranges need a slot per range AND frame: the 257-range
// mix of the tests needs 595 on a file of 74 frames).  Here the segment is
// gated by the range's FIRST frame alone.  That delivers the same contract:
// when the first frame failed the result is -1 and nothing is moved; otherwise
// every byte before the first failed frame is delivered, and what the segment
// moves behind it lands inside the range's own destination, past `result`,
// where the bytes are unspecified.  A segment's length is a u32: the host
// refuses a call whose staging reaches 4 GiB.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "range_result.h"

#ifdef __HIP__
#define ZSK_PD_HD __host__ __device__
#else
#define ZSK_PD_HD
#endif

namespace zsk {

constexpr int64_t kPlanOverflow = -2;   // ZSK_PLAN_OVERFLOW
constexpr int64_t kPlanSpan = -3;       // ZSK_PLAN_SPAN
// the touched frames' compressed span the parse kernels can address (reader_vec.cpp
// refuses a host-planned batch at the same bound): 2 GiB less the read slack
constexpr uint64_t kPlanSpanLimit = 0x7FFFFF00ull;
constexpr uint64_t kBadDst = ~0ull;     // RangeRow::full of a range with rtn == 0: destination outside the buffer
constexpr uint32_t kCompactT = 1024;    // threads of the compact workgroup

// zsk_range_t, zsk_frame_desc_t (FrameDesc) and zsk_segment_t (GatherSeg) as
// this header sees them (range_plan_dev.hip asserts the layouts)
struct DevRange {
    uint64_t offset, count, dst_off;
    int64_t result;
};
struct DevFrame {
    uint64_t c_off, d_off;
    uint32_t c_size, d_size;
};
struct DevSeg {
    uint64_t src_off, dst_off;
    uint32_t len, frame;
};

// the resident seek table (nframes + 1 prefix sums each; ck NULL: no checksums
// wanted) and the image's offset from the base the decode kernels get
struct PlanTables {
    const uint64_t *c_off, *d_off;
    const uint32_t *ck;
    uint64_t nframes, bias;
};

// What the compact step leaves for the call (zeroed on the stream first).
struct PlanHead {
    uint64_t touched;   // T, whatever max_frames is
    uint64_t bytes;     // decoded bytes of the touched frames
    uint64_t span;      // compressed bytes from the first touched frame's start to the last one's end
    int64_t flag;       // 0, kPlanOverflow, kPlanSpan
};

// Byte offsets of a call's arrays in one device buffer.  [0, zero_end) is
// zeroed on the stream before the touch kernel: the head and the bitmap.
struct PlanLayout {
    size_t head, bitmap, zero_end, segs, rows, dst, wrank, desc, t_doff, ck, total;
    uint64_t words, seg_cap;
};

inline PlanLayout plan_layout(uint64_t nranges, uint64_t max_frames, uint64_t nframes, bool ck)
{
    PlanLayout L{};
    auto take = [&](size_t bytes) {
        const size_t at = L.total;
        L.total = (L.total + bytes + 15) & ~(size_t)15;
        return at;
    };
    L.words = (nframes + 31) / 32;
    L.seg_cap = nranges;
    L.head = take(sizeof(PlanHead));
    L.bitmap = take(L.words * 4);
    L.zero_end = L.total;
    L.segs = take(L.seg_cap * sizeof(DevSeg));
    L.rows = take(nranges * sizeof(RangeRow));
    L.dst = take(nranges * 8);
    L.wrank = take(L.words * 4);
    L.desc = take(max_frames * sizeof(DevFrame));
    L.t_doff = take(max_frames * 8);
    L.ck = take(ck ? max_frames * 4 : 0);
    return L;
}

// thread t's contiguous share [a, b) of n elements among T threads
// (block_scan.h's block_share, for 64-bit counts and for the host)
ZSK_PD_HD inline void pd_share(uint64_t n, uint32_t T, uint32_t t, uint64_t *a, uint64_t *b)
{
    const uint64_t per = (n + T - 1) / T;
    const uint64_t lo = per * t, hi = per * (t + 1);
    *a = lo < n ? lo : n;
    *b = hi < n ? hi : n;
}

// plan_frame_of: the last frame that starts at or before x (x < d_off[nframes];
// zero-size frames are skipped the same way)
ZSK_PD_HD inline uint64_t pd_frame_of(const uint64_t *d_off, uint64_t nframes, uint64_t x)
{
    uint64_t lo = 0, hi = nframes + 1;   // the first entry above x
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (d_off[mid] > x)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo - 1;
}

// touch: the range's row, rt0 holding its first FILE frame (pd_rank makes it
// the touched index later).  An empty range, one at / past EOF: rtn 0, full 0.
// A destination [dst_off, dst_off + count) that is not inside [0, buf_size):
// rtn 0, full kBadDst -- the range touches nothing and moves nothing.
// offset + count may wrap (range_plan.h's range_end).
ZSK_PD_HD inline RangeRow pd_touch(const DevRange &q, const uint64_t *d_off, uint64_t nframes, uint64_t buf_size)
{
    RangeRow row{q.offset, 0, 0, 0};
    if (q.count == 0)
        return row;
    if (q.dst_off > buf_size || q.count > buf_size - q.dst_off) {
        row.full = kBadDst;
        return row;
    }
    const uint64_t size = nframes ? d_off[nframes] : 0;
    if (q.offset >= size)
        return row;
    const uint64_t end = q.count < size - q.offset ? q.offset + q.count : size;
    const uint64_t fa = pd_frame_of(d_off, nframes, q.offset), fb = pd_frame_of(d_off, nframes, end - 1);
    row.full = end - q.offset;
    row.rt0 = fa;
    row.rtn = fb - fa + 1;
    return row;
}

ZSK_PD_HD inline bool pd_bad_dst(const RangeRow &row)
{
    return row.rtn == 0 && row.full == kBadDst;
}

// bits fa..fb of the bitmap through orw(word index, mask): one call per word,
// whole words in the middle of a long run
template <class Or>
ZSK_PD_HD inline void pd_mark(uint64_t fa, uint64_t fb, Or orw)
{
    const uint64_t wa = fa >> 5, wb = fb >> 5;
    const uint32_t ma = 0xFFFFFFFFu << (fa & 31), mb = 0xFFFFFFFFu >> (31 - (fb & 31));
    if (wa == wb) {
        orw(wa, ma & mb);
        return;
    }
    orw(wa, ma);
    for (uint64_t w = wa + 1; w < wb; w++)
        orw(w, 0xFFFFFFFFu);
    orw(wb, mb);
}

// compact, first pass over bitmap word w: its set frames and their decoded bytes
ZSK_PD_HD inline void pd_word_sum(uint32_t word, uint64_t w, const uint64_t *d_off, uint64_t *count, uint64_t *bytes)
{
    for (uint32_t m = word; m; m &= m - 1) {
        const uint64_t f = 32 * w + (uint32_t)__builtin_ctz(m);
        *count += 1;
        *bytes += d_off[f + 1] - d_off[f];
    }
}

// ... second pass: the word's set frames get ranks *rank.. and packed offsets
// *packed.. (both advanced)
ZSK_PD_HD inline void pd_word_emit(uint32_t word, uint64_t w, uint64_t *rank, uint64_t *packed, const PlanTables &T,
                                   DevFrame *desc, uint64_t *t_doff, uint32_t *ck)
{
    for (uint32_t m = word; m; m &= m - 1) {
        const uint64_t f = 32 * w + (uint32_t)__builtin_ctz(m);
        const uint64_t dsz = T.d_off[f + 1] - T.d_off[f];
        desc[*rank] = DevFrame{T.c_off[f] + T.bias, *packed, (uint32_t)(T.c_off[f + 1] - T.c_off[f]), (uint32_t)dsz};
        t_doff[*rank] = T.d_off[f];
        if (ck)
            ck[*rank] = T.ck[f];
        *rank += 1;
        *packed += dsz;
    }
}

// a descriptor no kernel decodes anything for: every parse rejects a frame of
// under 7 compressed bytes before it loads one.  Its c_off is the first
// touched frame's (c_first; 0 when nothing is touched or the call is flagged):
// the lane-per-frame parses address a wave's frames through one buffer
// resource from the lowest c_off to the highest end among them, so a padding
// frame must not lie outside the span the call checked
ZSK_PD_HD inline DevFrame pd_padding(const PlanTables &T, uint64_t c_first)
{
    return DevFrame{c_first + T.bias, 0, 0, 0};
}

// span: compressed bytes from the first touched frame's start to the last
// one's end
ZSK_PD_HD inline int64_t pd_flag(uint64_t touched, uint64_t max_frames, uint64_t span)
{
    if (touched > max_frames)
        return kPlanOverflow;
    return span >= kPlanSpanLimit ? kPlanSpan : 0;
}

// the touched index of file frame f (its bit is set)
ZSK_PD_HD inline uint64_t pd_rank(const uint32_t *bitmap, const uint32_t *wrank, uint64_t f)
{
    return (uint64_t)wrank[f >> 5] + (uint32_t)__builtin_popcount(bitmap[f >> 5] & ((1u << (f & 31)) - 1u));
}

// segments: the range's one segment (fa its first file frame, row.rt0 already
// the touched index, which gates it); len 0 for a range without bytes
ZSK_PD_HD inline DevSeg pd_segment(const RangeRow &row, uint64_t fa, uint64_t dst_off, const uint64_t *d_off,
                                   const DevFrame *desc)
{
    if (!row.rtn)
        return DevSeg{0, 0, 0, 0};
    return DevSeg{desc[row.rt0].d_off + (row.offset - d_off[fa]), dst_off, (uint32_t)row.full, (uint32_t)row.rt0};
}

// fix: what a range's result becomes after range_result_kernel wrote `res`
// (*uncount: the range was counted as delivered in full and must not be)
ZSK_PD_HD inline int64_t pd_fix(const RangeRow &row, int64_t flag, int64_t res, bool *uncount)
{
    *uncount = !flag && pd_bad_dst(row);
    return flag || pd_bad_dst(row) ? -1 : res;
}

#ifndef __HIP_DEVICE_COMPILE__
// The four kernels with their grids spelled out as loops over threads: what
// the device leaves in the call's buffer (plan_dev_lanes) and in d_result
// (plan_dev_results).
struct DevPlan {
    PlanHead head{};
    std::vector<uint32_t> bitmap, wrank;
    std::vector<RangeRow> rows;
    std::vector<uint64_t> dst, t_doff;
    std::vector<DevFrame> desc;
    std::vector<uint32_t> ck;
    std::vector<DevSeg> segs;
};

inline DevPlan plan_dev_lanes(const DevRange *rg, uint64_t n, const PlanTables &T, uint64_t buf_size,
                              uint64_t max_frames)
{
    const PlanLayout L = plan_layout(n, max_frames, T.nframes, T.ck != nullptr);
    DevPlan P;
    P.bitmap.assign(L.words, 0);
    P.wrank.assign(L.words, 0);
    P.rows.resize(n);
    P.dst.resize(n);
    P.t_doff.assign(max_frames, 0);
    P.desc.resize(max_frames);
    P.ck.assign(T.ck ? max_frames : 0, 0);
    P.segs.assign(L.seg_cap, DevSeg{0, 0, 0, 0});
    // touch
    for (uint64_t r = 0; r < n; r++) {
        const RangeRow row = pd_touch(rg[r], T.d_off, T.nframes, buf_size);
        P.rows[r] = row;
        P.dst[r] = rg[r].dst_off;
        if (row.rtn)
            pd_mark(row.rt0, row.rt0 + row.rtn - 1, [&](uint64_t w, uint32_t m) { P.bitmap[w] |= m; });
    }
    // compact: per thread the sums of its share, then the scans
    std::vector<uint64_t> cnt(kCompactT, 0), byt(kCompactT, 0);
    uint64_t first = 0, last = 0;
    bool any = false;
    for (uint32_t t = 0; t < kCompactT; t++) {
        uint64_t a, b;
        pd_share(L.words, kCompactT, t, &a, &b);
        for (uint64_t w = a; w < b; w++) {
            const uint32_t word = P.bitmap[w];
            if (!word)
                continue;
            if (!any)
                first = 32 * w + (uint32_t)__builtin_ctz(word);
            any = true;
            last = 32 * w + 31 - (uint32_t)__builtin_clz(word);
            pd_word_sum(word, w, T.d_off, &cnt[t], &byt[t]);
        }
    }
    uint64_t rank = 0, packed = 0;
    std::vector<uint64_t> rank0(kCompactT), packed0(kCompactT);
    for (uint32_t t = 0; t < kCompactT; t++) {
        rank0[t] = rank;
        packed0[t] = packed;
        rank += cnt[t];
        packed += byt[t];
    }
    const uint64_t span = any ? T.c_off[last + 1] - T.c_off[first] : 0;
    P.head = PlanHead{rank, packed, span, pd_flag(rank, max_frames, span)};
    const uint64_t live = P.head.flag ? 0 : P.head.touched;
    for (uint32_t t = 0; t < kCompactT && !P.head.flag; t++) {
        uint64_t a, b, k = rank0[t], p = packed0[t];
        pd_share(L.words, kCompactT, t, &a, &b);
        for (uint64_t w = a; w < b; w++) {
            P.wrank[w] = (uint32_t)k;
            pd_word_emit(P.bitmap[w], w, &k, &p, T, P.desc.data(), P.t_doff.data(), T.ck ? P.ck.data() : nullptr);
        }
    }
    for (uint64_t i = live; i < max_frames; i++)
        P.desc[i] = pd_padding(T, live ? T.c_off[first] : 0);
    // segments
    for (uint64_t r = 0; r < n; r++) {
        RangeRow row = P.rows[r];
        const uint64_t fa = row.rt0;
        row.rt0 = 0;
        if (P.head.flag)
            row.rtn = 0;
        else if (row.rtn)
            row.rt0 = pd_rank(P.bitmap.data(), P.wrank.data(), fa);
        P.rows[r] = row;
        P.segs[r] = pd_segment(row, fa, P.dst[r], T.d_off, P.desc.data());
    }
    return P;
}

// d_result[0 .. n] from the touched frames' statuses (max_frames entries)
inline void plan_dev_results(const DevPlan &P, const int32_t *status, int64_t *result)
{
    RangeTable tab;
    tab.rows = P.rows;
    tab.t_doff = P.t_doff;
    const size_t n = P.rows.size();
    result[n] = (int64_t)range_results_lanes(tab, status, result);
    for (size_t r = 0; r < n; r++) {
        bool uncount;
        result[r] = pd_fix(P.rows[r], P.head.flag, result[r], &uncount);
        result[n] -= uncount;
    }
    if (P.head.flag)
        result[n] = P.head.flag;
}
#endif

}   // namespace zsk
