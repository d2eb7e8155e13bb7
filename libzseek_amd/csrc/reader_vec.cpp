// reader_vec.cpp -- the vectored reads (zsk_preadv, zsk_preadv_device,
// zsk_preadv_device_async, zsk_preadv_device_indirect): range_plan.h's batches
// through the first lane's slots.  A batch holds only the frames its ranges
// touch, read run by run and packed back to back; the decode is the
// contiguous read's (decode_batch), every frame whole (stop_last off); the
// bytes leave through the gather kernel (range_gather.hip), segment by segment.
// zsk_read_frames_indirect reads whole frames by index and needs neither
// staging nor gather: decode_batch writes into the caller's buffer.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "frame_list_plan.h"
#include "range_plan.h"
#include "range_plan_dev.h"
#include "range_result.h"
#include "reader_internal.h"
#include "zstd_caps.h"

using namespace zsk;

namespace {

struct VecJob {
    LaneJob J;   // r, g, call_data, err, io_failed: read_span's context
    const RangePlan *P;
    uint8_t *buf;
    bool device_dst;
    std::vector<int32_t> status;     // per touched frame (P->frames)
    std::vector<uint32_t> fail_at;
    // zsk_preadv_device_async: the batch's commands go on the caller's stream
    // `q` (NULL: the null stream) and nobody waits for them; its statuses are
    // appended on that stream to d_call_status (per touched frame, the call's
    // CallTable) instead of downloaded, and there is no finish_gather
    bool async = false;
    hipStream_t q = nullptr;
    int32_t *d_call_status = nullptr;

    VecJob(zseek_reader *r, void *call_data, const RangePlan &plan, void *dst, bool device)
        : P(&plan), buf(static_cast<uint8_t *>(dst)), device_dst(device)
    {
        J.r = r;
        J.call_data = call_data;
    }
};

// Batch b's descriptors -- its touched frames packed back to back, or where
// they lie in a device image -- into desc[0, n).  Returns the compressed
// bytes they cover; *max_dsize: the largest decoded size.
uint64_t fill_desc(const zseek_reader *r, const RangePlan &P, const PlanBatch &b, FrameDesc *desc, uint32_t *max_dsize)
{
    const SeekTable &st = r->st;
    uint64_t c = 0, d = 0;
    *max_dsize = 0;
    for (size_t t = b.t0; t < b.t1; t++) {
        const size_t f = P.frames[t];
        FrameDesc &fd = desc[t - b.t0];
        fd.c_off = r->img ? st.c_off[f] + r->img->bias : c;
        fd.d_off = d;
        fd.c_size = (uint32_t)st.csize(f);
        fd.d_size = (uint32_t)st.dsize(f);
        c += fd.c_size;
        d += fd.d_size;
        *max_dsize = std::max(*max_dsize, fd.d_size);
    }
    return c;
}

// The bounds an asynchronous zstd batch is decoded by (zsk_reader_set_zstd_async),
// from the seek table alone: its decoded span (the descriptors pack the frames
// back to back from 0), a sequence per seq_bytes of it, and per frame two
// blocks and one per 16 KiB.
ZstdBounds zstd_async_bounds(const zseek_reader *r, const FrameDesc *desc, size_t n)
{
    ZstdBounds B{0, 0, 0};
    for (size_t i = 0; i < n; i++) {
        B.out_bytes += desc[i].d_size;
        B.max_blocks += 2 + desc[i].d_size / 16384;
    }
    B.max_sequences = B.out_bytes / (r->zstd_async ? r->zstd_async : 3);
    return B;
}

// Read, upload, decode and gather batch bi on slot s.  Asynchronous mode
// (V.async): everything is queued on the caller's stream, directly -- the
// slot's own stream is not used, so "stream-ordered" needs no event bridge --
// and the slot is left `pending` behind its `done` event for its next user
// to drain.
bool submit_gather(VecJob &V, Slot &s, size_t bi)
{
    zseek_reader *r = V.J.r;
    DeviceCtx &g = *V.J.g;
    const SeekTable &st = r->st;
    const RangePlan &P = *V.P;
    const PlanBatch &b = P.batches[bi];
    const size_t n = b.t1 - b.t0, nseg = b.s1 - b.s0;
    uint64_t csz = 0;
    for (size_t t = b.t0; t < b.t1; t++)
        csz += st.csize(P.frames[t]);
    const uint64_t dsz = b.d_bytes;
    const bool ck = r->verify && st.checksum_flag;
    // a host destination: the segments compacted (in segment order, P.cum)
    // into the slot's pinned bounce -- by the gather itself through the
    // bounce's device mapping when the batch is small (download_small's
    // bound), else compacted behind the decoded bytes in d_out and brought
    // down by one DMA
    const uint64_t h_len = V.device_dst ? 0 : b.out_bytes;
    const uint64_t pack_at = gather_pack_at(dsz);
    (void)hipSetDevice(g.device);
    // the slot's previous asynchronous batch must have finished before the
    // host rewrites its pinned staging below (a host wait, the one a fourth
    // batch in flight costs)
    s.drain();
    hipStream_t const q = V.async ? V.q : s.stream;
    if (h_len > s.h_out_cap)
        pool_wait(&s.copies);
    // a file in device memory: nothing is read or packed -- the touched frames
    // are decoded where they are, from host-built descriptors (the host has
    // the whole table, and a vectored batch's d_off is a scan over its sparse
    // frame list; they ride in the small upload that carries the segments
    // anyway, so a device-side builder would save no transfer)
    const DeviceImage *const img = r->img;
    // behind the packed compressed bytes and their 256-byte read slack: the
    // descriptors, the zstd host plan, the segments, their prefix sum
    // (the asynchronous zstd read: no host plan, the device's own plan is
    // checked against bounds from the seek table -- zstd_async_bounds)
    const bool zasync = V.async && r->type == ZSEEK_ZSTD;
    const bool zplan = !img && r->type == ZSEEK_ZSTD && n <= kOneMaxFrames && !zasync;
    const BatchLayout L = vectored_layout(csz, n, nseg, img != nullptr, zplan);
    if (!s.reserve(L.up, pack_at + h_len, h_len, n, ck, V.J.err)) {
        V.J.io_failed = true;
        return false;
    }
    uint64_t c_at = 0;
    for (size_t ri = b.r0; ri < b.r1; ri++) {   // one pread per run of adjacent frames (an image: its bounds)
        const uint64_t c0 = st.c_off[P.runs[ri].f0], len = st.c_off[P.runs[ri].f1] - c0;
        if (len && !(img ? image_span(V.J, img, len, c0) : read_span(V.J, s.h_comp + c_at, len, c0))) {
            V.J.io_failed = true;
            return false;
        }
        c_at += len;
    }
    // (the parse kernels address a wave's frames through one 32-bit buffer
    // resource: the planner's span cut keeps a batch far below it unless
    // batch_bytes was set to 512 MiB or more)
    if (img && n && st.c_off[P.frames[b.t1 - 1] + 1] - st.c_off[P.frames[b.t0]] >= 0x7FFFFF00ull) {
        set_error(V.J.err, "vectored read: a batch spans 2 GiB of the device image");
        V.J.io_failed = true;
        return false;
    }
    FrameDesc *const h_desc = reinterpret_cast<FrameDesc *>(s.h_comp + L.doff);
    const FrameDesc *const d_desc = reinterpret_cast<const FrameDesc *>(s.d_comp + L.doff);
    uint32_t max_dsize;
    (void)fill_desc(r, P, b, h_desc, &max_dsize);
    GatherSeg *const h_seg = reinterpret_cast<GatherSeg *>(s.h_comp + L.goff);
    const uint64_t *const cum = P.cum.data() + b.s0 + bi;
    for (size_t i = 0; i < nseg; i++) {
        const PlanSeg &ps = P.segs[b.s0 + i];
        h_seg[i] = {ps.src_off, V.device_dst ? ps.dst_off : cum[i], ps.len, ps.frame};
    }
    memcpy(s.h_comp + L.coff, cum, (nseg + 1) * sizeof(uint64_t));
    s.begin_batch(0, 0, 0, h_len);
    ZstdHostPlan zp{};
    if (zplan)
        zstd_host_plan(h_desc, s.h_comp, (uint32_t)n, reinterpret_cast<uint64_t *>(s.h_comp + L.poff), &zp);
    static const bool host_dma = getenv("ZSEEK_HOST_DMA") != nullptr;
    hipError_t e = hipSuccess;
    if (host_dma)
        e = hipMemcpyAsync(s.d_comp, s.h_comp, L.up, hipMemcpyHostToDevice, q);
    else if (upload_small(s.d_comp, s.h_comp, s.h_comp_dev, L.up, q) != 0)
        e = hipErrorLaunchFailure;
    // (what the kernels read the frames from: the slot's staging, or the image)
    DecodeBatch dec{r->type, q, d_desc, (uint32_t)n, img ? img->base : s.d_comp, max_dsize};
    dec.zplan = zplan ? &zp : nullptr;
    dec.d_plan = reinterpret_cast<const uint64_t *>(s.d_comp + L.poff);
    dec.h_desc = h_desc;
    const ZstdBounds zb = zstd_async_bounds(r, h_desc, n);
    if (zasync)
        dec.zasync = &zb;
    if (ck) {
        for (size_t i = 0; i < n; i++)
            s.h_ck[i] = st.checksum[P.frames[b.t0 + i]];
        dec.d_want = s.d_ck;
    }
    if (e == hipSuccess)
        e = decode_batch(s, dec);
    // the segments of the frames that decoded: into the caller's device
    // buffer, or compacted for the host (the slot's previous batch must have
    // left the bounce first)
    if (e == hipSuccess && h_len)
        pool_wait(&s.copies);
    if (e == hipSuccess && b.out_bytes) {
        const bool mapped = h_len && !host_dma && h_len <= kDownloadSmallMax && s.h_out_dev;
        uint8_t *const dst = V.device_dst ? V.buf : mapped ? static_cast<uint8_t *>(s.h_out_dev) : s.d_out + pack_at;
        if (launch_range_gather(reinterpret_cast<const GatherSeg *>(s.d_comp + L.goff),
                                reinterpret_cast<const uint64_t *>(s.d_comp + L.coff), (uint32_t)nseg, b.out_bytes,
                                s.d_out, dst, s.d_status, q) != 0)
            e = hipErrorLaunchFailure;
        if (e == hipSuccess && h_len && !mapped)
            e = hipMemcpyAsync(s.h_out, s.d_out + pack_at, h_len, hipMemcpyDeviceToHost, q);
    }
    // the statuses: downloaded for finish_gather, or (asynchronous) kept on the
    // device, appended to the call's, which outlive the slot's reuse by a later
    // batch (a range can span batches)
    if (e == hipSuccess && V.async)
        e = hipMemcpyAsync(V.d_call_status + b.t0, s.d_status, n * sizeof(int32_t), hipMemcpyDeviceToDevice, q);
    else if (e == hipSuccess &&
             download_small(reinterpret_cast<uint32_t *>(s.h_status), host_dma ? nullptr : s.h_status_dev,
                            reinterpret_cast<const uint32_t *>(s.d_status), (uint32_t)(2 * n), nullptr, nullptr,
                            s.d_out, 0, q) != 0)
        e = hipErrorLaunchFailure;
    // (asynchronous: whatever was queued, a failed batch's part included, is
    // behind `done`; the slot's next user waits for it, this call does not)
    if (e == hipSuccess || V.async) {
        const hipError_t er = hipEventRecord(s.done, q);
        s.pending = V.async && er == hipSuccess;
        if (e == hipSuccess)
            e = er;
    }
    if (e != hipSuccess) {
        set_error(V.J.err, "GPU decode failed: %s", hipGetErrorString(e));
        V.J.io_failed = true;
        if (!s.pending)
            (void)hipStreamSynchronize(q);
        return false;
    }
    g.count_batch(n, dsz, img ? 0 : csz);
    return true;
}

// Wait for batch bi on slot s: keep its frames' statuses and, for a host
// destination, scatter the bounce into the caller's buffer on the pool (the
// segments of failed frames are left out: the gather skipped them).
bool finish_gather(VecJob &V, Slot &s, size_t bi)
{
    const RangePlan &P = *V.P;
    const PlanBatch &b = P.batches[bi];
    const size_t n = b.t1 - b.t0;
    const hipError_t e = hipEventSynchronize(s.done);
    if (e != hipSuccess) {
        set_error(V.J.err, "GPU decode failed: %s", hipGetErrorString(e));
        V.J.io_failed = true;
        return false;
    }
    for (size_t i = 0; i < n; i++) {
        V.status[b.t0 + i] = s.h_status[i];
        V.fail_at[b.t0 + i] = reinterpret_cast<const uint32_t *>(s.h_status + n)[i];
    }
    if (V.device_dst || !b.out_bytes)
        return true;
    // pieces of >= 256 KiB, about one per pool thread
    const uint64_t piece = std::max<uint64_t>(256u << 10, b.out_bytes / (uint64_t)copy_pool_threads() + 1);
    const uint64_t *const cum = P.cum.data() + b.s0 + bi;
    const PlanSeg *const segs = P.segs.data() + b.s0;
    const int32_t *const status = V.status.data() + b.t0;
    const uint8_t *const bounce = s.h_out;
    uint8_t *const buf = V.buf;
    const size_t nseg = b.s1 - b.s0;
    for (size_t i = 0; i < nseg;) {
        size_t j = i + 1;
        while (j < nseg && cum[j] - cum[i] < piece)
            j++;
        pool_run([=] {
            for (size_t k = i; k < j; k++)
                if (status[segs[k].frame] == ST_OK)
                    memcpy(buf + segs[k].dst_off, bounce + cum[k], segs[k].len);
        }, &s.copies);
        i = j;
    }
    return true;
}

// A vectored call's ranges as the planner's requests and, once the caller
// holds the reader's lock, their plan.
struct VecCall {
    std::vector<RangeReq> req;
    size_t nframes = 0;
    const uint64_t *d_off = nullptr;   // nframes + 1 decoded offsets
    RangePlan P;

    VecCall(const zsk_range_t *ranges, size_t nranges) : req(nranges)
    {
        for (size_t i = 0; i < nranges; i++)
            req[i] = {ranges[i].offset, ranges[i].count, ranges[i].dst_off};
    }

    // false, with the text in errbuf: bytes to deliver but no buffer, or a batch
    // beyond the gather's 32-bit segment count or the decode's 31-bit frame count
    bool plan(const zseek_reader *r, const void *buf, char *errbuf)
    {
        static const uint64_t zero = 0;
        const SeekTable &st = r->st;
        nframes = st.frames();
        d_off = nframes ? st.d_off.data() : &zero;
        // a device image's frames are decoded where they lie: the LZ4 plan lays
        // item slots out by compressed distance and the parse kernels address a
        // wave's frames through one 32-bit resource, so a batch of sparse frames is
        // also cut by the compressed span it covers (4 x batch_bytes: 256 MiB by default)
        P = r->img && nframes ? plan_ranges(req.data(), req.size(), d_off, nframes, r->batch_bytes, st.c_off.data(),
                                            (uint64_t)std::min<size_t>(r->batch_bytes, SIZE_MAX / 4) * 4)
                              : plan_ranges(req.data(), req.size(), d_off, nframes, r->batch_bytes);
        if (!buf && !P.segs.empty()) {
            set_error(errbuf, "invalid buffer");
            return false;
        }
        for (const PlanBatch &b : P.batches)
            if (b.s1 - b.s0 >= 0xFFFFFFFFull || b.t1 - b.t0 >= 0x7FFFFFFFull) {
                set_error(errbuf, "too many ranges");
                return false;
            }
        return true;
    }
};

ssize_t preadv_frames(zseek_reader *r, void *buf, zsk_range_t *ranges, size_t nranges, void *call_data, char *errbuf,
                      bool device_dst)
{
    static_assert(sizeof(zsk_segment_t) == sizeof(GatherSeg), "segment ABI");
    for (size_t i = 0; ranges && i < nranges; i++)
        ranges[i].result = -1;
    if (!r) {
        set_error(errbuf, "invalid reader");
        return -1;
    }
    if (nranges == 0)
        return 0;
    if (!ranges) {
        set_error(errbuf, "invalid ranges");
        return -1;
    }
    VecCall call(ranges, nranges);
    DeviceGuard keep_device;
    std::unique_lock<std::shared_mutex> guard(r->lock);
    PublishStats publish{r};
    if (!call.plan(r, buf, errbuf))
        return -1;
    const RangePlan &P = call.P;
    VecJob V(r, call_data, P, buf, device_dst);
    V.status.assign(P.frames.size(), ST_NOT_RUN);
    V.fail_at.assign(P.frames.size(), 0);
    if (!P.batches.empty()) {
        if (!ensure_lanes(r, errbuf))
            return -1;
        DeviceCtx &g = *r->lanes[0];
        V.J.g = &g;
        (void)hipSetDevice(g.device);
        run_in_flight(
            g,
            [&](Slot &s, size_t bi) {
                return bi == P.batches.size() ? kNoneLeft : submit_gather(V, s, bi) ? kQueued : kQueueFailed;
            },
            [&](Slot &s, size_t bi) { return finish_gather(V, s, bi); });
        if (V.J.io_failed) {
            set_error(errbuf, "%s", V.J.err);
            return -1;
        }
    }
    std::vector<int64_t> result(nranges);
    std::vector<size_t> bad(nranges);
    const size_t ok = range_results(P, call.req.data(), nranges, call.d_off, call.nframes, V.status.data(),
                                    result.data(), bad.data());
    bool reported = false;
    for (size_t i = 0; i < nranges; i++) {
        ranges[i].result = result[i];
        if (bad[i] != SIZE_MAX && !reported) {
            // the lowest-index failed range: a cached reader's text for the frame
            frame_error(r, true, V.status[bad[i]], V.fail_at[bad[i]], P.frames[bad[i]], 0, 0, errbuf);
            reported = true;
        }
    }
    return (ssize_t)ok;
}

// An asynchronous call grows buffers for ALL of the lane's idle slots and call
// tables at once, to what its largest batch needs (submit_gather's sizes, LZ4
// with a device destination): growing waits for the device, and a slot grown
// only when a later call reaches it would make that call wait for the caller's
// stream in the middle of a pipeline that the first call had warmed up.  Slots
// and tables with work in flight are left alone (their turn comes after their
// drain).  Best effort: a failure here is reported by the batch that needs
// the buffer.
void grow_idle_for_async(VecJob &V, DeviceCtx &g, size_t table_up, size_t table_total)
{
    zseek_reader *r = V.J.r;
    const bool ck = r->verify && r->st.checksum_flag;
    const bool zstd = r->type == ZSEEK_ZSTD;
    ZstdBounds zb{0, 0, 0};
    uint64_t up = 0, out = 0, items = 0;
    size_t nmax = 0;
    uint32_t max_dsize;
    std::vector<FrameDesc> desc;
    for (const PlanBatch &b : V.P->batches) {
        const size_t n = b.t1 - b.t0;
        desc.resize(n);
        const uint64_t csz = fill_desc(r, *V.P, b, desc.data(), &max_dsize);
        // (no zstd host plan on this path)
        up = std::max(up, vectored_layout(csz, n, b.s1 - b.s0, r->img != nullptr, false).up);
        out = std::max(out, gather_pack_at(b.d_bytes));
        nmax = std::max(nmax, n);
        if (zstd) {
            const ZstdBounds B = zstd_async_bounds(r, desc.data(), n);
            zb = {std::max(zb.out_bytes, B.out_bytes), std::max(zb.max_blocks, B.max_blocks),
                  std::max(zb.max_sequences, B.max_sequences)};
            continue;
        }
        items = std::max(items, split_items_needed(desc.data(), (uint32_t)n));
    }
    const bool split = !zstd && lz4_pick_engine((uint32_t)nmax) != ENGINE_WAVE;
    char err[ZSEEK_ERRBUF_SIZE];
    for (Slot &s : g.slot) {
        if (s.pending || !nmax)
            continue;
        (void)s.reserve(up, out, 0, nmax, ck, err);
        if (zstd)
            (void)zstd_scratch_reserve(&s.zs, (uint32_t)nmax, zb.out_bytes,
                                       zstd_item_capacity((uint32_t)nmax, zb.max_blocks, zb.max_sequences),
                                       zb.max_blocks, s.stream);
        // (on the slot's own, idle stream: its wait is no wait; the scratch's
        // first memset is complete before the caller's stream uses it)
        if (split && split_scratch_reserve(&s.split, (uint32_t)nmax, items, s.stream) == 0)
            (void)hipStreamSynchronize(s.stream);
        (void)hipGetLastError();
    }
    for (CallTable &c : g.call)
        if (!c.pending)
            (void)c.reserve(table_up, table_total, err);
}

// A stream-ordered call with no ranges: d_result[0] = 0 alone.
ssize_t answer_no_ranges(int64_t *d_result, hipStream_t q, char *errbuf)
{
    if (launch_range_result(nullptr, nullptr, nullptr, 0, d_result, q) == 0)
        return 0;
    set_error(errbuf, "GPU decode failed: %s", hipGetErrorString(hipGetLastError()));
    return -1;
}

// The end of a stream-ordered call that has queued work on q.  A failed call
// (err: why) still leaves the stream's consumer an answer: every result and
// the count -1.  The call table -- and the slot, for a caller whose batch has
// not recorded its own (s: NULL when submit_gather has) -- are in use until the
// stream passes this point; a record that fails is a host wait instead.
ssize_t end_stream_call(bool ok, Slot *s, CallTable &c, int64_t *d_result, size_t nranges, hipStream_t q,
                        const char *err, char *errbuf)
{
    if (!ok)
        (void)hipMemsetAsync(d_result, 0xFF, (nranges + 1) * sizeof(int64_t), q);
    bool recorded = !s || (s->pending = hipEventRecord(s->done, q) == hipSuccess);
    if (c.done)
        recorded = c.pending = recorded && hipEventRecord(c.done, q) == hipSuccess;
    if (!recorded)
        (void)hipStreamSynchronize(q);
    if (ok)
        return 0;
    set_error(errbuf, "%s", err);
    return -1;
}

// zsk_preadv_device_async (zseek_hip.h): preadv_frames' batches queued on the
// caller's stream, one after the other, and behind the last one
// range_result_kernel, which leaves in d_result what range_results computes on
// the host.  Nothing is waited for except a slot or a call table that an
// earlier asynchronous batch still uses (Slot::drain, CallTable::drain) and
// buffers that have to grow.
}   // namespace

extern "C" ZSEEK_EXPORT ssize_t zsk_preadv_device_async(zseek_reader_t *r, void *d_buf, const zsk_range_t *ranges,
                                                        size_t nranges, int64_t *d_result, void *stream,
                                                        void *call_data, char *errbuf)
{
    hipStream_t const q = static_cast<hipStream_t>(stream);
    if (!r) {
        set_error(errbuf, "invalid reader");
        return -1;
    }
    if (refuse_capturing(q, "asynchronous read", errbuf))
        return -1;
    if (r->type != ZSEEK_LZ4 && !(r->type == ZSEEK_ZSTD && r->zstd_async)) {
        // zsk_zstd_decode_frames' plan synchronizes; the stream-ordered decode
        // is opt-in, zsk_reader_set_zstd_async
        set_error(errbuf, "asynchronous read: zstd is not supported");
        return -1;
    }
    if (nranges == 0 && !d_result)
        return 0;
    if (!ranges && nranges) {
        set_error(errbuf, "invalid ranges");
        return -1;
    }
    if (!d_result) {
        set_error(errbuf, "invalid result buffer");
        return -1;
    }
    VecCall call(ranges, nranges);
    DeviceGuard keep_device;
    std::unique_lock<std::shared_mutex> guard(r->lock);
    PublishStats publish{r};
    if (!call.plan(r, d_buf, errbuf))   // (the batches are preadv_frames')
        return -1;
    const RangePlan &P = call.P;
    if (!ensure_lanes(r, errbuf))
        return -1;
    DeviceCtx &g = *r->lanes[0];
    (void)hipSetDevice(g.device);
    if (nranges == 0)
        return answer_no_ranges(d_result, q, errbuf);
    // (from here on every return goes through end_stream_call)
    VecJob V(r, call_data, P, d_buf, true);
    V.async = true;
    V.q = q;
    V.J.g = &g;
    CallTable &c = g.take_call();
    const size_t T = P.frames.size();
    // rows, t_doff (the upload, which moves whole 16-byte pieces), statuses
    const size_t rows_bytes = nranges * sizeof(RangeRow), up = rows_bytes + T * sizeof(uint64_t);
    const size_t st_at = (up + 15) & ~(size_t)15;
    grow_idle_for_async(V, g, up, st_at + T * sizeof(int32_t));
    // (a host wait when this table's previous call, kSlots calls ago, has not
    // finished: the host rewrites its pinned staging)
    bool ok = c.reserve(up, st_at + T * sizeof(int32_t), V.J.err);
    hipError_t e = hipSuccess;
    if (ok) {
        const RangeTable tab = build_range_table(P, call.req.data(), nranges, call.d_off, call.nframes);
        memcpy(c.h, tab.rows.data(), rows_bytes);
        if (T)
            memcpy(c.h + rows_bytes, tab.t_doff.data(), T * sizeof(uint64_t));
        V.d_call_status = reinterpret_cast<int32_t *>(c.d + st_at);
        if (upload_small(c.d, c.h, c.h_dev, up, q) != 0)
            e = hipErrorLaunchFailure;
        // a batch that is never queued reads as failed
        if (e == hipSuccess && T)
            e = hipMemsetD32Async((hipDeviceptr_t)V.d_call_status, ST_NOT_RUN, T, q);
        if (e != hipSuccess) {
            set_error(V.J.err, "GPU decode failed: %s", hipGetErrorString(e));
            ok = false;
        }
    }
    // the batches take the lane's slots round robin; a slot whose earlier
    // asynchronous batch is still in flight is waited for (submit_gather)
    for (size_t bi = 0; ok && bi < P.batches.size(); bi++)
        ok = submit_gather(V, g.take_slot(), bi);
    if (ok && launch_range_result(reinterpret_cast<const RangeRow *>(c.d),
                                  reinterpret_cast<const uint64_t *>(c.d + rows_bytes), V.d_call_status, nranges,
                                  d_result, q) != 0) {
        set_error(V.J.err, "GPU decode failed: %s", hipGetErrorString(hipGetLastError()));
        ok = false;
    }
    // (the slots have recorded in submit_gather)
    return end_stream_call(ok, nullptr, c, d_result, nranges, q, V.J.err, errbuf);
}

// zsk_preadv_device_indirect (zseek_hip.h): a vectored read of a device image
// whose ranges are in device memory.  The plan is computed on the device
// (range_plan_dev.hip) from the resident seek table; the host sizes every
// buffer and grid by its bounds -- nranges, max_frames, the file's largest
// frame -- and sends nothing but kernel arguments.  One batch: the touched
// frames (at most max_frames, then padding descriptors) decoded in place from
// the image into the slot's staging, gathered into d_buf, the results by
// range_result_kernel and the plan's fix kernel.  The slot and the call table
// are taken in turn and left pending like zsk_preadv_device_async's.
extern "C" ZSEEK_EXPORT ssize_t zsk_preadv_device_indirect(zseek_reader_t *r, void *d_buf, size_t buf_size,
                                                           const zsk_range_t *d_ranges, size_t nranges,
                                                           size_t max_frames, int64_t *d_result, void *stream,
                                                           char *errbuf)
{
    hipStream_t const q = static_cast<hipStream_t>(stream);
    if (!r) {
        set_error(errbuf, "invalid reader");
        return -1;
    }
    const DeviceImage *const img = r->img;
    if (!img) {
        set_error(errbuf, "device-planned read: needs a device image");
        return -1;
    }
    // (zstd: the host cannot see the touched frames to size their scratch by;
    // the file's census bounds any max_frames of them, zsk_reader_zstd_census)
    const bool zstd = r->type == ZSEEK_ZSTD;
    if (r->type != ZSEEK_LZ4 && !(zstd && img->has_census.load(std::memory_order_acquire))) {
        set_error(errbuf, "device-planned read: zstd is not supported");
        return -1;
    }
    if (refuse_capturing(q, "device-planned read", errbuf))
        return -1;
    if (nranges == 0 && !d_result)
        return 0;
    if (nranges && !d_ranges) {
        set_error(errbuf, "invalid ranges");
        return -1;
    }
    if (!d_result) {
        set_error(errbuf, "invalid result buffer");
        return -1;
    }
    if (nranges && max_frames == 0) {
        set_error(errbuf, "device-planned read: max_frames is 0");
        return -1;
    }
    if (nranges && buf_size && !d_buf) {
        set_error(errbuf, "invalid buffer");
        return -1;
    }
    // (the gather takes a 32-bit segment count, the decode a 31-bit frame count)
    if (max_frames >= 0x7FFFFFFFull || nranges >= 0xFFFFFFFFull) {
        set_error(errbuf, "too many ranges");
        return -1;
    }
    const SeekTable &st = r->st;
    DeviceGuard keep_device;
    std::unique_lock<std::shared_mutex> guard(r->lock);
    PublishStats publish{r};
    if (nranges && img->max_dsize && max_frames > r->batch_bytes / img->max_dsize) {
        set_error(errbuf, "device-planned read: max_frames frames exceed the batch size");
        return -1;
    }
    // (a range is one segment of the staging, and a segment's length a u32)
    if (nranges && (uint64_t)max_frames * img->max_dsize > 0xFFFFFFFFull) {
        set_error(errbuf, "device-planned read: max_frames frames exceed 4 GiB");
        return -1;
    }
    // zstd: what any max_frames entries of the file need at most, by the census
    // (zstd_caps.h); the decode's own limit on the block bound
    ZstdBounds zb{0, 0, 0};
    if (zstd)
        zstd_census_bounds(max_frames, img->census.max_blocks, img->census.max_sequences, img->max_dsize,
                           &zb.out_bytes, &zb.max_blocks, &zb.max_sequences);
    if (nranges && zb.max_blocks >= (1ull << 29)) {
        set_error(errbuf, "device-planned read: max_frames frames exceed the zstd block bound");
        return -1;
    }
    // (a table that puts frames past the image's end: image_span's refusal,
    // once for the whole table -- its prefix sums only grow)
    if (st.c_off.back() > img->size) {
        set_error(errbuf, "unexpected EOF");
        return -1;
    }
    if (!ensure_lanes(r, errbuf))
        return -1;
    DeviceCtx &g = *r->lanes[0];
    (void)hipSetDevice(g.device);
    if (nranges == 0)
        return answer_no_ranges(d_result, q, errbuf);
    const size_t nframes = st.frames();
    const bool ck = r->verify && st.checksum_flag;
    const PlanLayout L = plan_layout(nranges, max_frames, nframes, ck);
    const PlanTables T{img->d_coff, img->d_doff, ck ? img->d_ck : nullptr, nframes, img->bias};
    const uint32_t M = (uint32_t)max_frames;
    Slot &s = g.take_slot();
    CallTable &c = g.take_call();
    char err[ZSEEK_ERRBUF_SIZE] = {0};
    // (host waits: a slot or table whose earlier asynchronous work has not
    // finished, and buffers that have to grow)
    s.drain();
    bool ok = c.reserve(0, L.total, err) && s.reserve(0, std::max<size_t>((size_t)max_frames * img->max_dsize, 16), 0, max_frames, false, err);
    // the parse scratch by the plan's scan layout: max_frames frames of at most
    // the file's largest compressed size, however far apart they lie
    // (zstd: the decode's scratch by the census bounds, grown here so that a
    // failure is reported before anything is queued)
    int scratch = 0;
    if (ok && zstd)
        scratch = zstd_scratch_reserve(&s.zs, M, zb.out_bytes, zstd_item_capacity(M, zb.max_blocks, zb.max_sequences),
                                       zb.max_blocks, q);
    else if (ok && !lz4_wave_batch(r->type, M))
        scratch = split_scratch_reserve(&s.split, M, (uint64_t)M * slots_of(img->max_csize), q);
    if (scratch != 0) {
        set_error(err, "allocate GPU decode buffers failed");
        ok = false;
    }
    if (!ok) {
        (void)hipGetLastError();
        set_error(errbuf, "%s", err);
        return -1;   // (nothing queued)
    }
    // (from here on every return goes through end_stream_call)
    s.begin_batch(0, 0, 0, 0);
    ok = launch_indirect_plan(c.d, L, T, d_ranges, nranges, buf_size, max_frames, q) == 0;
    // the frames scattered over the image (the plan's scan layout), the scratch
    // reserved above, each frame's size bounded by the file's largest
    DecodeBatch dec{r->type, q, reinterpret_cast<const FrameDesc *>(c.d + L.desc), M, img->base, img->max_dsize};
    dec.in_order = false;
    if (zstd)
        dec.zasync = &zb;   // (the device checks its plan against them: zstd_fit_kernel)
    dec.d_want = ck ? reinterpret_cast<const uint32_t *>(c.d + L.ck) : nullptr;
    ok = ok && decode_batch(s, dec) == hipSuccess;
    // (no host total: the gather's scan launch reads the segments' on the device)
    if (ok && d_buf)
        ok = launch_range_gather(reinterpret_cast<const GatherSeg *>(c.d + L.segs), nullptr, (uint32_t)L.seg_cap, 0,
                                 s.d_out, static_cast<uint8_t *>(d_buf), s.d_status, q) == 0;
    if (ok)
        ok = launch_range_result(reinterpret_cast<const RangeRow *>(c.d + L.rows),
                                 reinterpret_cast<const uint64_t *>(c.d + L.t_doff), s.d_status, nranges, d_result,
                                 q) == 0 &&
             launch_indirect_fix(c.d, L, nranges, d_result, q) == 0;
    if (!ok)
        set_error(err, "GPU decode failed: %s", hipGetErrorString(hipGetLastError()));
    else
        g.count_batch();   // (frames_decoded / bytes_decoded: the host never learns them)
    return end_stream_call(ok, &s, c, d_result, nranges, q, err, errbuf);
}

// zsk_read_frames_indirect (zseek_hip.h): whole frames of a device image by
// an index list in device memory, each decoded straight into the caller's
// buffer.  The plan (frame_list_plan.hip) turns slot i's index into a
// descriptor whose d_off is the slot's own offset of d_buf -- the scan of the
// sizes before it, or i * stride -- so the decode's output base is d_buf itself:
// no staging, no gather.  One batch of nidx descriptors (a slot that decodes
// nothing: padding), sized like the device-planned read's with nidx in place
// of max_frames; the slot (its statuses and decoder scratch) and the call
// table (the plan) are taken in turn and left pending.
extern "C" ZSEEK_EXPORT ssize_t zsk_read_frames_indirect(zseek_reader_t *r, const int64_t *d_idx, size_t nidx,
                                                         size_t stride, void *d_buf, size_t buf_size,
                                                         uint64_t *d_offsets, int64_t *d_result, void *stream,
                                                         char *errbuf)
{
    hipStream_t const q = static_cast<hipStream_t>(stream);
    if (!r) {
        set_error(errbuf, "invalid reader");
        return -1;
    }
    const DeviceImage *const img = r->img;
    if (!img) {
        set_error(errbuf, "frame-list read: needs a device image");
        return -1;
    }
    const bool zstd = r->type == ZSEEK_ZSTD;
    if (r->type != ZSEEK_LZ4 && !(zstd && img->has_census.load(std::memory_order_acquire))) {
        set_error(errbuf, "frame-list read: zstd is not supported");
        return -1;
    }
    if (refuse_capturing(q, "frame-list read", errbuf))
        return -1;
    if (nidx && !d_idx) {
        set_error(errbuf, "invalid index list");
        return -1;
    }
    if (nidx && !d_result) {
        set_error(errbuf, "invalid result buffer");
        return -1;
    }
    if (!stride && !d_offsets) {
        set_error(errbuf, "frame-list read: the packed layout needs d_offsets");
        return -1;
    }
    if (buf_size && !d_buf) {
        set_error(errbuf, "invalid buffer");
        return -1;
    }
    // (the decode kernels take any d_off from an aligned base)
    if ((uintptr_t)d_buf & 15) {
        set_error(errbuf, "frame-list read: d_buf is not 16-byte aligned");
        return -1;
    }
    if (((uintptr_t)d_offsets | (uintptr_t)d_result | (uintptr_t)d_idx) & 7) {
        set_error(errbuf, "frame-list read: misaligned list, offsets or result buffer");
        return -1;
    }
    const SeekTable &st = r->st;
    DeviceGuard keep_device;
    std::unique_lock<std::shared_mutex> guard(r->lock);
    PublishStats publish{r};
    // the decoded span the descriptors can cover: what bounds the parse scratch
    // and the zstd literal scratch, which is addressed by their d_off
    const uint64_t unit = stride ? stride : img->max_dsize;
    if (nidx >= 0x7FFFFFFFull || (unit && nidx > r->batch_bytes / unit)) {
        set_error(errbuf, "frame-list read: the list exceeds the batch size");
        return -1;
    }
    const uint64_t cover = (uint64_t)nidx * unit;
    if (cover > 0xFFFFFFFFull) {
        set_error(errbuf, "frame-list read: the list exceeds 4 GiB");
        return -1;
    }
    // zstd: what any nidx entries of the file need at most, by the census; the
    // literals of slot i lie at its d_off of the scratch, inside the span the
    // fitting slots cover
    ZstdBounds zb{0, 0, 0};
    if (zstd) {
        zstd_census_bounds(nidx, img->census.max_blocks, img->census.max_sequences, img->max_dsize, &zb.out_bytes,
                           &zb.max_blocks, &zb.max_sequences);
        zb.out_bytes = std::min<uint64_t>(buf_size, cover);
    }
    if (nidx && zb.max_blocks >= (1ull << 29)) {
        set_error(errbuf, "frame-list read: the list exceeds the zstd block bound");
        return -1;
    }
    if (st.c_off.back() > img->size) {
        set_error(errbuf, "unexpected EOF");
        return -1;
    }
    if (!ensure_lanes(r, errbuf))
        return -1;
    DeviceCtx &g = *r->lanes[0];
    (void)hipSetDevice(g.device);
    if (nidx == 0) {
        if (!d_result && !d_offsets)
            return 0;
        hipError_t e = d_offsets ? hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), q) : hipSuccess;
        if (e == hipSuccess && d_result)
            return answer_no_ranges(d_result, q, errbuf);
        if (e == hipSuccess)
            return 0;
        set_error(errbuf, "GPU decode failed: %s", hipGetErrorString(e));
        return -1;
    }
    const size_t nframes = st.frames();
    const bool ck = r->verify && st.checksum_flag;
    const FrameListLayout L = frame_list_layout(nidx, ck);
    const PlanTables T{img->d_coff, img->d_doff, ck ? img->d_ck : nullptr, nframes, img->bias};
    const uint32_t M = (uint32_t)nidx;
    Slot &s = g.take_slot();
    CallTable &c = g.take_call();
    char err[ZSEEK_ERRBUF_SIZE] = {0};
    // (host waits: a slot or table whose earlier asynchronous work has not
    // finished, and buffers that have to grow)
    s.drain();
    // (no staging: 16 bytes stand in as the output base of a call without a buffer)
    bool ok = c.reserve(0, L.total, err) && s.reserve(0, 16, 0, nidx, false, err);
    int scratch = 0;
    if (ok && zstd)
        scratch = zstd_scratch_reserve(&s.zs, M, zb.out_bytes, zstd_item_capacity(M, zb.max_blocks, zb.max_sequences),
                                       zb.max_blocks, q);
    else if (ok && !lz4_wave_batch(r->type, M))
        scratch = split_scratch_reserve(&s.split, M, (uint64_t)M * slots_of(img->max_csize), q);
    if (scratch != 0) {
        set_error(err, "allocate GPU decode buffers failed");
        ok = false;
    }
    if (!ok) {
        (void)hipGetLastError();
        set_error(errbuf, "%s", err);
        return -1;   // (nothing queued)
    }
    // (from here on every return goes through end_stream_call)
    s.begin_batch(0, 0, 0, 0);
    ok = launch_frame_list_plan(c.d, L, T, d_idx, nidx, stride, buf_size, d_offsets, d_result, q) == 0;
    DecodeBatch dec{r->type, q, reinterpret_cast<const FrameDesc *>(c.d + L.desc), M, img->base, img->max_dsize};
    dec.in_order = false;
    if (zstd)
        dec.zasync = &zb;   // (the device checks its plan against them: zstd_fit_kernel)
    dec.d_want = ck ? reinterpret_cast<const uint32_t *>(c.d + L.ck) : nullptr;
    dec.out = static_cast<uint8_t *>(d_buf);
    ok = ok && decode_batch(s, dec) == hipSuccess;
    ok = ok && launch_frame_list_result(c.d, L, nidx, s.d_status, d_result, q) == 0;
    if (!ok)
        set_error(err, "GPU decode failed: %s", hipGetErrorString(hipGetLastError()));
    else
        g.count_batch();   // (frames_decoded / bytes_decoded: the host never learns them)
    return end_stream_call(ok, &s, c, d_result, nidx, q, err, errbuf);
}

// Vectored reads (zseek_hip.h): many ranges, one decode grid per batch.
extern "C" ZSEEK_EXPORT ssize_t zsk_preadv(zseek_reader_t *reader, void *buf, zsk_range_t *ranges, size_t nranges,
                                           void *call_data, char *errbuf)
{
    return preadv_frames(reader, buf, ranges, nranges, call_data, errbuf, false);
}

extern "C" ZSEEK_EXPORT ssize_t zsk_preadv_device(zseek_reader_t *reader, void *d_buf, zsk_range_t *ranges,
                                                  size_t nranges, void *call_data, char *errbuf)
{
    return preadv_frames(reader, d_buf, ranges, nranges, call_data, errbuf, true);
}

extern "C" ZSEEK_EXPORT int zsk_gather_segments(const zsk_segment_t *d_seg, uint32_t nseg, const void *d_src,
                                                void *d_dst, const int32_t *d_status, void *stream)
{
    return launch_range_gather(reinterpret_cast<const GatherSeg *>(d_seg), nullptr, nseg, 0,
                               static_cast<const uint8_t *>(d_src), static_cast<uint8_t *>(d_dst), d_status,
                               static_cast<hipStream_t>(stream));
}
