// The plan of a whole-frame read whose INDEX list is in device memory
// (zsk_read_frames_indirect): slot i of the list asks for seek-table frame
// idx[i], whole, and the frame is decoded straight into the caller's buffer --
// at the scan of the sizes before it (packed) or at i * stride (rows).  No
// staging, no gather, no bitmap of touched frames: a repeated index is simply
// two slots with two destinations.  Everything comes from the seek table a
// device-image reader keeps resident (range_plan_dev.h's PlanTables).  No HIP
// runtime calls and no reader state, so tests/native/frame_list_plan_shim.cpp
// drives it on the CPU, lane by lane (frame_list_lanes below spells the
// kernels out as loops over their threads); frame_list_plan.hip's kernels use
// exactly these functions.
//
// Four steps, every grid sized by nidx:
//
//   size     thread per slot: want[i] = the frame's decoded size, or -1 for an
//            index that is no frame of the file;
//   scan     one workgroup: every thread sums its share of the sizes and
//            reduces the compressed bounds [c_off[f], c_off[f + 1]) of its
//            valid non-empty slots; a scan of the sums gives every slot its
//            packed offset (off[0 .. nidx]) and the head the total, the lowest
//            touched compressed byte and the span's flag;
//   emit     thread per slot: d_offsets[i], the slot's descriptor {c_off[f] +
//            bias, destination offset, c_size, d_size}, its checksum word, and
//            want[i] made final -- -1 for a slot whose region is not inside
//            the buffer or wider than its row, and for every slot of a flagged
//            call.  A slot that decodes nothing (want <= 0) gets pd_padding's
//            descriptor at the lowest touched frame;
//   result   thread per slot, behind the decode: d_result[i] from want[i] and
//            the frame's status, and their count.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "range_plan_dev.h"

namespace zsk {

// What the scan step leaves for the call.
struct FrameListHead {
    uint64_t total;   // decoded bytes of the valid slots (the packed layout's size)
    uint64_t c_lo;    // the lowest touched frame's c_off (0: nothing touched)
    uint64_t span;    // compressed bytes from there to the highest touched frame's end
    int64_t flag;     // 0 or kPlanSpan
};

// Byte offsets of a call's arrays in one device buffer (nothing to zero).
struct FrameListLayout {
    size_t head, off, want, desc, ck, total;
};

inline FrameListLayout frame_list_layout(uint64_t nidx, bool ck)
{
    FrameListLayout L{};
    auto take = [&](size_t bytes) {
        const size_t at = L.total;
        L.total = (L.total + bytes + 15) & ~(size_t)15;
        return at;
    };
    L.head = take(sizeof(FrameListHead));
    L.off = take((nidx + 1) * 8);
    L.want = take(nidx * 8);
    L.desc = take(nidx * sizeof(DevFrame));
    L.ck = take(ck ? nidx * 4 : 0);
    return L;
}

// size: the decoded size of frame idx, -1 when idx is no frame of the file
ZSK_PD_HD inline int64_t fl_size(int64_t idx, const uint64_t *d_off, uint64_t nframes)
{
    if (idx < 0 || (uint64_t)idx >= nframes)
        return -1;
    return (int64_t)(d_off[idx + 1] - d_off[idx]);
}

// scan, a thread's share [a, b): the decoded bytes of its valid slots and the
// compressed bounds of its valid non-empty ones (*lo > *hi: none)
ZSK_PD_HD inline void fl_share_sum(const int64_t *idx, const int64_t *want, uint64_t a, uint64_t b,
                                   const uint64_t *c_off, uint64_t *bytes, uint64_t *lo, uint64_t *hi)
{
    *bytes = 0;
    *lo = ~0ull;
    *hi = 0;
    for (uint64_t i = a; i < b; i++) {
        const int64_t w = want[i];
        if (w <= 0)
            continue;
        const uint64_t f = (uint64_t)idx[i];
        *bytes += (uint64_t)w;
        *lo = c_off[f] < *lo ? c_off[f] : *lo;
        *hi = c_off[f + 1] > *hi ? c_off[f + 1] : *hi;
    }
}

// ... second pass: the share's slots get the packed offsets *packed.. (advanced)
ZSK_PD_HD inline void fl_share_emit(const int64_t *want, uint64_t a, uint64_t b, uint64_t *packed, uint64_t *off)
{
    for (uint64_t i = a; i < b; i++) {
        off[i] = *packed;
        *packed += want[i] > 0 ? (uint64_t)want[i] : 0;
    }
}

ZSK_PD_HD inline FrameListHead fl_head(uint64_t total, uint64_t lo, uint64_t hi)
{
    const bool any = lo <= hi;
    const uint64_t span = any ? hi - lo : 0;
    return FrameListHead{total, any ? lo : 0, span, span >= kPlanSpanLimit ? kPlanSpan : 0};
}

// where slot i goes: its scanned offset, or its row
ZSK_PD_HD inline uint64_t fl_dst(uint64_t i, uint64_t stride, const uint64_t *off)
{
    return stride ? i * stride : off[i];
}

// emit: what slot i delivers when its frame decodes -- the size, 0 (an empty
// frame: delivered, nothing decoded, wherever its offset lies) or -1 (no such
// frame, a flagged call, a region [dst, dst + size) that is not inside [0,
// buf_size), a frame wider than its row)
ZSK_PD_HD inline int64_t fl_want(int64_t size, uint64_t dst, uint64_t stride, uint64_t buf_size, int64_t flag)
{
    if (size < 0 || flag)
        return -1;
    if (size == 0)
        return 0;
    if (dst > buf_size || (uint64_t)size > buf_size - dst)
        return -1;
    return stride && (uint64_t)size > stride ? -1 : size;
}

// ... and its descriptor (want > 0: frame f decoded at dst; else padding inside
// the span the call checked)
ZSK_PD_HD inline DevFrame fl_desc(int64_t want, uint64_t f, uint64_t dst, const PlanTables &T,
                                  const FrameListHead &h)
{
    if (want <= 0)
        return pd_padding(T, h.flag ? 0 : h.c_lo);
    return DevFrame{T.c_off[f] + T.bias, dst, (uint32_t)(T.c_off[f + 1] - T.c_off[f]), (uint32_t)want};
}

// result: d_result[i] (status: the slot's frame status, 0 = ZSK_OK)
ZSK_PD_HD inline int64_t fl_result(int64_t want, int32_t status)
{
    return want <= 0 ? want : status == 0 ? want : -1;
}

#ifndef __HIP_DEVICE_COMPILE__
// The kernels with their grids spelled out as loops over threads: what the
// device leaves in the call's buffer and d_offsets (frame_list_lanes) and in
// d_result (frame_list_results).
struct FrameListPlan {
    FrameListHead head{};
    std::vector<uint64_t> off;       // nidx + 1: the packed scan
    std::vector<uint64_t> offsets;   // nidx + 1: what d_offsets receives
    std::vector<int64_t> want;
    std::vector<DevFrame> desc;
    std::vector<uint32_t> ck;
};

inline FrameListPlan frame_list_lanes(const int64_t *idx, uint64_t n, uint64_t stride, uint64_t buf_size,
                                      const PlanTables &T)
{
    FrameListPlan P;
    P.off.assign(n + 1, 0);
    P.offsets.assign(n + 1, 0);
    P.want.assign(n, -1);
    P.desc.resize(n);
    P.ck.assign(T.ck ? n : 0, 0);
    // size
    for (uint64_t i = 0; i < n; i++)
        P.want[i] = fl_size(idx[i], T.d_off, T.nframes);
    // scan: per thread the sums of its share, then the scan of the shares
    std::vector<uint64_t> byt(kCompactT);
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t t = 0; t < kCompactT; t++) {
        uint64_t a, b, l, h;
        pd_share(n, kCompactT, t, &a, &b);
        fl_share_sum(idx, P.want.data(), a, b, T.c_off, &byt[t], &l, &h);
        lo = l < lo ? l : lo;
        hi = h > hi ? h : hi;
    }
    uint64_t packed = 0;
    for (uint32_t t = 0; t < kCompactT; t++) {
        uint64_t a, b, p = packed;
        pd_share(n, kCompactT, t, &a, &b);
        fl_share_emit(P.want.data(), a, b, &p, P.off.data());
        packed += byt[t];
    }
    P.off[n] = packed;
    P.head = fl_head(packed, lo, hi);
    // emit
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t dst = fl_dst(i, stride, P.off.data());
        const int64_t w = fl_want(P.want[i], dst, stride, buf_size, P.head.flag);
        P.offsets[i] = dst;
        P.desc[i] = fl_desc(w, (uint64_t)idx[i], dst, T, P.head);
        if (T.ck)
            P.ck[i] = w > 0 ? T.ck[idx[i]] : 0;
        P.want[i] = w;
    }
    P.offsets[n] = stride ? n * stride : P.head.total;
    return P;
}

// d_result[0 .. n] from the slots' statuses
inline void frame_list_results(const FrameListPlan &P, const int32_t *status, int64_t *result)
{
    const size_t n = P.want.size();
    int64_t count = 0;
    for (size_t i = 0; i < n; i++) {
        result[i] = fl_result(P.want[i], status[i]);
        count += result[i] >= 0;
    }
    result[n] = P.head.flag ? P.head.flag : count;
}
#endif

}   // namespace zsk
