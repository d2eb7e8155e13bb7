// zstd_decode.hip — zstd frame decoding on the GPU (gfx950), the reference's
// ZSTD_decompressDCtx / ZSTD_decompressStream call (decompress.c:434-538;
// libzstd 1.4.9, restated in oracle/zstd_oracle.c): the decode's scratch, its
// pipeline of stages over three streams (launch_zstd_decode) and the content
// checksums.  The stages' kernels are in the files named below.
//
// A zstd frame is serial twice over (Huffman literal streams, FSE sequence
// states), but each serial chain is short and there are many of them, so each
// gets its own lane.  Per batch: zstd_plan_kernel, zstd_scan_kernel
// (zstd_plan.hip: item and block slots per frame, slot offsets) ->
// zstd_frame_kernel (zstd_frame.hip: headers, raw / RLE literals, tables into
// the block slots, Huffman jobs, the op list) -> zstd_huf_kernel beside
// zstd_seq_kernel (zstd_huf_seq.hip: literals into the literal scratch; the op
// list replayed into 8-byte items) -> seq_exec_kernel (seq_exec.hip) ->
// zstd_check_kernel (XXH64 content checksums).
#include <stdlib.h>

#include <algorithm>

#include "xxh64_dev.h"
#include "zstd_caps.h"
#include "zstd_dev.h"
#include "zstd_internal.h"

namespace zsk {
namespace {

using namespace lz4d;
using namespace xxh64d;

// XXH64 of [o0, cap) of a frame's output for frames flagged by the frame
// kernel: lanes 0..3 run the four accumulators over 1 KiB chunks staged in
// LDS by the whole wave; lane 0 merges and finishes.
__global__ __launch_bounds__(256) void zstd_check_kernel(
    const FrameDesc *__restrict__ desc, uint32_t n, const uint8_t *__restrict__ out,
    const uint64_t *__restrict__ ck, const uint8_t *__restrict__ ops, const uint64_t *__restrict__ blk_base,
    int32_t *__restrict__ status, uint32_t *__restrict__ fail_at, uint32_t stop_last, uint32_t f0,
    const uint64_t *__restrict__ fit)
{
    __shared__ uint64_t buf[4][128];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t f = uni(blockIdx.x * 4 + w);   // frames [f0, f0 + n) of the batch
    if (f >= n)
        return;
    // the asynchronous decode, a batch that did not fit its bounds: the
    // call's last kernel names the refusal (zstd_fit_kernel left ST_NOT_RUN,
    // at which the execute kernels return at their top)
    if (fit && *fit) {
        if (lane == 0) {
            status[f] = ST_SCRATCH;
            if (fail_at)
                fail_at[f] = 0;
        }
        return;
    }
    if (!(ck[f] >> 63) || uni((uint32_t)status[f]) != (uint32_t)ST_OK)
        return;
    const FrameDesc d = desc[f];
    // the entry's requests: its OP_FEND ops that the replay marked (a & 4)
    // with the frame's start (e) and length (f), in order
    const uint64_t ob = op_base(blk_base, f0 + f);
    const uint32_t opn = (uint32_t)(op_base(blk_base, f0 + f + 1) - ob);
    const ZOp *op = reinterpret_cast<const ZOp *>(ops) + ob;
    for (uint32_t k = 0; k < opn; k++) {
        const uint32_t kind = uni(op[k].k);
        if (kind == OP_DONE || kind == OP_ERR)
            break;
        if (kind != OP_FEND || !(uni(op[k].a) & 4))
            continue;
        const uint32_t o0 = uni(op[k].e), len = uni(op[k].f), want = uni(op[k].d);
        // (a no-cache read's last entry executed only up to the request's end:
        // libzstd's streaming decoder never reaches this frame's end and its
        // checksum there either, nor a later frame's)
        if (f + 1 == n && stop_last < o0 + len)
            break;
        const uint8_t *p = out + d.d_off + o0;
        uint32_t bad = 0;
        const Span sp = make_span(p, len);
        uint64_t acc = lane == 0 ? P64_1 + P64_2 : lane == 1 ? P64_2 : lane == 2 ? 0 : 0ull - P64_1;
        const uint32_t stripes = len / 32;
        for (uint32_t s0 = 0; s0 < stripes; s0 += 32) {
            // 32 stripes = 1 KiB: 16 bytes per lane
            const u32x4 v = load16u(sp.r, sp.s0 + 1024 * (s0 / 32) + 16 * lane);
            *reinterpret_cast<u32x4 *>(&buf[w][2 * lane]) = v;
            const uint32_t m = stripes - s0 < 32 ? stripes - s0 : 32;
            if (lane < 4)
                for (uint32_t i = 0; i < m; i++)
                    acc = xround(acc, buf[w][4 * i + lane]);
        }
        uint64_t h;
        const uint64_t a1 = __shfl(acc, 1, 64), a2 = __shfl(acc, 2, 64), a3 = __shfl(acc, 3, 64);
        if (len >= 32) {
            h = rotl64(acc, 1) + rotl64(a1, 7) + rotl64(a2, 12) + rotl64(a3, 18);
            h = xmerge(h, acc);
            h = xmerge(h, a1);
            h = xmerge(h, a2);
            h = xmerge(h, a3);
        } else {
            h = P64_5;
        }
        h += len;
        if (lane == 0) {
            uint32_t i = stripes * 32;
            for (; i + 8 <= len; i += 8) {
                uint64_t k = 0;
                for (int b = 0; b < 8; b++)
                    k |= (uint64_t)p[i + b] << (8 * b);
                h ^= xround(0, k);
                h = rotl64(h, 27) * P64_1 + P64_4;
            }
            for (; i + 4 <= len; i += 4) {
                const uint64_t k = (uint64_t)p[i] | (uint64_t)p[i + 1] << 8 | (uint64_t)p[i + 2] << 16 |
                                   (uint64_t)p[i + 3] << 24;
                h ^= k * P64_1;
                h = rotl64(h, 23) * P64_2 + P64_3;
            }
            for (; i < len; i++) {
                h ^= p[i] * P64_5;
                h = rotl64(h, 11) * P64_1;
            }
            bad = (uint32_t)xavalanche(h) != want;
        }
        if (uni((uint32_t)__shfl((int)bad, 0, 64))) {
            if (lane == 0) {
                status[f] = zerr(ZE_CHECKSUM);
                if (fail_at)
                    fail_at[f] = o0 + len;   // checked at the frame's end
            }
            break;
        }
    }
}

}   // namespace

// The Huffman kernel's side stream and its two events belong to the scratch.
// Teardown (zstd_scratch_free) drains the side stream and destroys it before
// its events and before the caller's stream goes: the side stream's wait on
// an event recorded on the caller's stream is released while that stream is
// still alive.
void zstd_scratch_drop_streams(ZstdScratch *s)
{
    for (hipStream_t *q : {&s->side, &s->sq})
        if (*q) {
            (void)hipStreamSynchronize(*q);
            hip_stream_put(*q);
            *q = nullptr;
        }
}

namespace {
template <typename T>
int grow(T **p, uint64_t &cap, uint64_t want, uint64_t unit)
{
    if (want <= cap)
        return 0;
    if (*p)
        (void)hipFree(*p);
    *p = nullptr;
    cap = 0;
    if (hipMalloc((void **)p, want * unit) != hipSuccess)
        return -1;
    cap = want;
    return 0;
}

// streams first, then the events recorded on them
void side_destroy(ZstdScratch *s)
{
    zstd_scratch_drop_streams(s);
    for (int c = 0; c < ZstdScratch::kChunks; c++)
        for (hipEvent_t *e : {&s->ev_f[c], &s->ev_s[c], &s->ev_h[c]})
            if (*e) {
                hip_event_put(*e);
                *e = nullptr;
            }
}

int side_create(ZstdScratch *s)
{
    // the Huffman stream at the lowest priority: the sequence kernel, the
    // longer of the two, gets the CUs' LDS first (10.9 -> 10.6 ms per launch
    // at config 5; launching the sequence kernel first made no difference)
    (void)hipGetDevice(&s->side_dev);
    bool ok = hip_stream_get(&s->side, true) == hipSuccess && hip_stream_get(&s->sq, false) == hipSuccess;
    for (int c = 0; ok && c < ZstdScratch::kChunks; c++)
        for (hipEvent_t *e : {&s->ev_f[c], &s->ev_s[c], &s->ev_h[c]})
            ok = ok && (*e || hip_event_get(e) == hipSuccess);
    if (!ok) {   // partly created, nothing recorded on it yet
        side_destroy(s);
        return -1;
    }
    return 0;
}
}   // namespace

// Chunks a decode of n frames runs in (frames [n c / k, n (c + 1) / k)): the
// frame kernel of chunk c + 1 and the execute of chunk c - 1 run beside the
// sequence and Huffman kernels of chunk c, which leave most of each CU's
// issue slots idle.  Env ZSEEK_ZSTD_CHUNKS (A/B runs).  Config
// 5 (65,536 frames), same box, after the round-3 kernel changes: 2 chunks
// 9.50 / 9.57 ms, 3 8.71 / 8.73, 4 9.04 / 9.03, 6 10.07 / 10.17.
uint32_t zstd_chunks(uint32_t n)
{
    static const int forced = getenv("ZSEEK_ZSTD_CHUNKS") ? atoi(getenv("ZSEEK_ZSTD_CHUNKS")) : 0;
    uint32_t k = n >= 16384 ? 3 : n >= 4096 ? 2 : 1;
    if (forced > 0)
        k = (uint32_t)forced;
    if (k > (uint32_t)ZstdScratch::kChunks)
        k = ZstdScratch::kChunks;
    return k > n ? (n ? n : 1) : k;
}

int zstd_scratch_reserve(ZstdScratch *s, uint32_t frames, uint64_t out_bytes, uint64_t items,
                         uint64_t blocks, hipStream_t stream)
{
    (void)stream;
    if (!s->side && side_create(s) != 0)
        return -1;
    if (frames + 1 > s->frames_cap) {
        const uint32_t cap = frames + 1 < 4096 ? 4096 : frames + 1;
        for (void *p : {(void *)s->bound, (void *)s->bblk, (void *)s->rec_base, (void *)s->blk_base,
                        (void *)s->nitems, (void *)s->ck, (void *)s->stop, (void *)s->d_total})
            if (p)
                (void)hipFree(p);
        if (s->total)
            (void)hipHostFree(s->total);
        s->bound = s->bblk = s->nitems = s->stop = nullptr;
        s->rec_base = s->blk_base = s->ck = s->d_total = s->total = nullptr;
        s->frames_cap = 0;
        if (hipMalloc((void **)&s->bound, sizeof(uint32_t) * cap) != hipSuccess ||
            hipMalloc((void **)&s->bblk, sizeof(uint32_t) * cap) != hipSuccess ||
            hipMalloc((void **)&s->rec_base, sizeof(uint64_t) * (cap + 1)) != hipSuccess ||
            hipMalloc((void **)&s->blk_base, sizeof(uint64_t) * (cap + 1)) != hipSuccess ||
            hipMalloc((void **)&s->nitems, sizeof(uint32_t) * cap) != hipSuccess ||
            hipMalloc((void **)&s->ck, sizeof(uint64_t) * cap) != hipSuccess ||
            hipMalloc((void **)&s->stop, sizeof(uint32_t) * cap) != hipSuccess ||
            hipMalloc((void **)&s->d_total, ZstdScratch::kTotalWords * sizeof(uint64_t)) != hipSuccess ||
            hipMemset(s->d_total, 0, ZstdScratch::kTotalWords * sizeof(uint64_t)) != hipSuccess ||
            hipHostMalloc((void **)&s->total, (5 + ZstdScratch::kChunks) * sizeof(uint64_t), hipHostMallocDefault) !=
                hipSuccess)
            return -1;
        s->total[0] = s->total[1] = s->total[2] = 0;
        s->frames_cap = cap;
    }
    if (grow(&s->lit, s->lit_cap, out_bytes + 64, 1) != 0 || grow(&s->items, s->items_cap, items, 8) != 0)
        return -1;
    if (blocks > s->blocks_cap) {
        uint64_t c0 = s->blocks_cap, c1 = s->blocks_cap, c2 = s->blocks_cap;
        if (grow(&s->hjobs, c0, blocks, 4 * sizeof(HufJob)) != 0 ||
            grow(&s->hbad, c1, blocks, 4) != 0 || grow(&s->slots, c2, blocks, kZSlot) != 0)
            return -1;
        s->blocks_cap = blocks;
    }
    // op lists: 4 per block + 4 per frame
    return grow(&s->ops, s->ops_cap, blocks + frames, 4 * sizeof(ZOp));
}

size_t zstd_block_scratch_bytes(const ZstdScratch *s)
{
    return s->blocks_cap * (kZSlot + 4 * sizeof(HufJob) + 4) + s->ops_cap * 4 * sizeof(ZOp);
}

void zstd_scratch_release_memory(ZstdScratch *s)
{
    for (hipStream_t q : {s->side, s->sq})
        if (q)
            (void)hipStreamSynchronize(q);
    for (void *p : {(void *)s->bound, (void *)s->bblk, (void *)s->rec_base, (void *)s->blk_base,
                    (void *)s->nitems, (void *)s->ck, (void *)s->stop, (void *)s->lit, (void *)s->items,
                    (void *)s->ops, (void *)s->hjobs, (void *)s->slots, (void *)s->hbad, (void *)s->d_total})
        if (p)
            (void)hipFree(p);
    if (s->total)
        (void)hipHostFree(s->total);
    s->bound = s->bblk = s->nitems = s->stop = nullptr;
    s->rec_base = s->blk_base = s->ck = s->d_total = s->total = nullptr;
    s->lit = s->slots = s->hbad = nullptr;
    s->items = nullptr;
    s->ops = s->hjobs = nullptr;
    s->frames_cap = 0;
    s->lit_cap = s->items_cap = s->blocks_cap = s->ops_cap = 0;
}

// memory (its streams drained), then streams, then events
void zstd_scratch_free(ZstdScratch *s)
{
    zstd_scratch_release_memory(s);
    side_destroy(s);
    *s = ZstdScratch();
}

// Frame kernel -> Huffman kernel beside the sequence kernel -> literal fix-up
// -> execute -> checksums, in zstd_chunks(n) chunks of frames pipelined over
// three streams: the caller's stream runs every chunk's frame kernel, then
// each chunk's fix-up, execute and checksums once its sequence (s->sq) and
// Huffman (s->side) kernels are done; those start on a chunk as soon as its
// frame kernel is.  s must hold the last plan of these frames.
// async (the stream-ordered form): the plan's totals never reach the host.
// Every chunk's Huffman grid covers the call's block capacity and takes its
// job range from d_total, every chunk is treated as having Huffman blocks,
// the checksum kernel always runs, the largest frame is max_dsize, and each
// stage returns at its top when zstd_fit_kernel's verdict says the batch did
// not fit.
int launch_zstd_decode(const FrameDesc *d_desc, uint32_t nframes, const uint8_t *d_comp,
                       uint8_t *d_out, int32_t *d_status, ZstdScratch *s, hipStream_t stream,
                       uint32_t *d_fail_at, uint32_t stop_last, bool cks, const ZstdBounds *async,
                       uint32_t max_dsize)
{
    if (nframes == 0)
        return 0;
    if (async ? async->max_blocks > s->blocks_cap : s->total[2] > s->blocks_cap)
        return -1;
    if (async)
        cks = true;
    else
        max_dsize = (uint32_t)std::min<uint64_t>(s->total[3], 0xFFFFFFFFu);
    const uint32_t K = zstd_chunks(nframes);
    static const bool serial = getenv("ZSEEK_ZSTD_SERIAL") != nullptr;   // diagnostics: one stream
    // the one-frame route (a request's few frames): the execute a workgroup
    // per frame (env ZSEEK_ONE_ROUTE=0: the wave kernels, as round 4)
    static const bool one_off = env_is_zero("ZSEEK_ONE_ROUTE");
    const bool one = !one_off && nframes <= kOneMaxFrames;
    // (the one-frame route's sequence replay on the caller's stream, right
    // behind the frame kernel: a cross-stream hand-off cost ~30 us each way;
    // with its Huffman jobs in the same launch, zstd_one_kernel -- env
    // ZSEEK_ONE_FUSE=0: the Huffman kernel on the side stream, as before)
    static const bool fuse_off = env_is_zero("ZSEEK_ONE_FUSE");
    const bool fuse = one && !fuse_off;
    hipStream_t const hs = serial ? stream : s->side, qs = serial || one ? stream : s->sq;
    const uint64_t *const fit = async ? s->d_total + ZstdScratch::kFitWord : nullptr;
    const ZstdCall C{d_desc, d_comp, d_status, d_fail_at, fit};
    auto drain = [&] {   // an enqueue failed: nothing may still write the scratch
        (void)hipStreamSynchronize(stream);
        (void)hipStreamSynchronize(s->side);
        (void)hipStreamSynchronize(s->sq);
        return -1;
    };
    auto chunk = [&](uint32_t c) {
        const uint32_t f0 = (uint32_t)((uint64_t)nframes * c / K), f1 = (uint32_t)((uint64_t)nframes * (c + 1) / K);
        if (async)
            return ZstdChunk{c, f0, f1, 0, async->max_blocks, s->d_total + 4 + c};
        return ZstdChunk{c, f0, f1, s->total[4 + c], s->total[5 + c], nullptr};
    };
    for (uint32_t c = 0; c < K; c++) {
        const ZstdChunk ch = chunk(c);
        if (ch.f1 == ch.f0)
            continue;
        hipEvent_t tf = kernel_span_begin(stream);   // (per-kernel spans: timing on only)
        launch_zstd_frame(C, s, ch, one, stream);
        kernel_span_end(SPAN_ZFRAME, tf, stream);
        if (fuse) {
            hipEvent_t tq = kernel_span_begin(stream);
            launch_zstd_one(C, s, ch, stream);
            kernel_span_end(SPAN_ZSEQ, tq, stream);
            zstd_seq_timers(stream);
            continue;
        }
        if (hipEventRecord(s->ev_f[c], stream) != hipSuccess || hipStreamWaitEvent(qs, s->ev_f[c], 0) != hipSuccess)
            return drain();
        // the Huffman streams decode beside the sequence replay (neither reads
        // the other's output); zstd_lit_fix_kernel joins them
        if (ch.b1 > ch.b0) {
            if (hipStreamWaitEvent(hs, s->ev_f[c], 0) != hipSuccess)
                return drain();
            hipEvent_t th = kernel_span_begin(hs);
            launch_zstd_huf(C, s, ch, one, hs);
            kernel_span_end(SPAN_ZHUF, th, hs);
            if (hipEventRecord(s->ev_h[c], hs) != hipSuccess)
                return drain();
        }
        hipEvent_t tq = kernel_span_begin(qs);
        launch_zstd_seq(C, s, ch, one, qs);
        kernel_span_end(SPAN_ZSEQ, tq, qs);
        if (hipEventRecord(s->ev_s[c], qs) != hipSuccess)
            return drain();
    }
    stage_mark(2, stream);
    int rc = 0;
    for (uint32_t c = 0; c < K; c++) {
        const ZstdChunk ch = chunk(c);
        const uint32_t f0 = ch.f0, m = ch.f1 - ch.f0;
        if (m == 0)
            continue;
        const bool huf = ch.b1 > ch.b0;
        if (!fuse && (hipStreamWaitEvent(stream, s->ev_s[c], 0) != hipSuccess ||
                      (huf && hipStreamWaitEvent(stream, s->ev_h[c], 0) != hipSuccess)))
            return drain();
        if (huf && !fuse)   // (fused: the last workgroup's)
            launch_zstd_lit_fix(C, s, ch, stream);
        hipEvent_t tx = kernel_span_begin(stream);
        const uint32_t stop = c + 1 == K ? stop_last : 0xFFFFFFFFu;   // (the batch's last frame)
        if (launch_seq_exec_lit(d_desc + f0, m, s->lit, d_out, s->rec_base + f0, s->items, s->nitems + f0,
                                d_status + f0, stream, one, max_dsize, stop) != 0)
            rc = -1;
        kernel_span_end(SPAN_ZEXEC, tx, stream);
        if (cks)   // (a host plan that met no content checksum: nothing to check)
            hipLaunchKernelGGL(zstd_check_kernel, dim3((m + 3) / 4), dim3(256), 0, stream, d_desc + f0, m, d_out,
                               s->ck + f0, s->ops, s->blk_base, d_status + f0,
                               d_fail_at ? d_fail_at + f0 : nullptr, stop, f0, fit);
    }
    stage_mark(3, stream);
    stage_mark(4, stream);
    return rc == 0 && hipGetLastError() == hipSuccess ? 0 : -1;
}

// Plan, wait for the totals, size the scratch, decode.  The one
// synchronization point of the zstd path: the item slots and table slots of a
// frame are only known once its block headers and sequence counts are read.
int zstd_decode_frames(const FrameDesc *d_desc, uint32_t nframes, const uint8_t *d_comp,
                       uint8_t *d_out, int32_t *d_status, ZstdScratch *s, hipStream_t stream,
                       uint32_t *d_fail_at, uint32_t stop_last)
{
    if (nframes == 0)
        return 0;
    (void)hipGetLastError();   // a stale error of an earlier call is not this launch's
    if (zstd_scratch_reserve(s, nframes, 0, 0, 0, stream) != 0)
        return -1;
    stage_mark(0, stream);
    if (launch_zstd_plan(d_desc, nframes, d_comp, s, stream) != 0)
        return -1;
    stage_mark(1, stream);
    if (hipStreamSynchronize(stream) != hipSuccess)
        return -1;
    if (zstd_scratch_reserve(s, nframes, s->total[1], s->total[0], s->total[2], stream) != 0)
        return -1;
    return launch_zstd_decode(d_desc, nframes, d_comp, d_out, d_status, s, stream, d_fail_at, stop_last);
}

// The stream-ordered form: reserve from the bounds (the only host wait: a
// scratch that has to grow), plan, verdict, decode -- nothing comes back.
int zstd_decode_frames_async(const FrameDesc *d_desc, uint32_t nframes, const uint8_t *d_comp, uint8_t *d_out,
                             int32_t *d_status, ZstdScratch *s, hipStream_t stream, const ZstdBounds &B,
                             uint32_t *d_fail_at, uint32_t stop_last, uint32_t max_dsize)
{
    if (nframes == 0)
        return 0;
    (void)hipGetLastError();   // a stale error of an earlier call is not this launch's
    const uint64_t items = zstd_item_capacity(nframes, B.max_blocks, B.max_sequences);
    // (4 * max_blocks Huffman jobs a grid; bounds past that are no scratch a device holds)
    if (items == ~0ull || B.max_blocks >= (1ull << 29) || B.out_bytes >= (1ull << 58))
        return -1;
    if (zstd_scratch_reserve(s, nframes, B.out_bytes, items, B.max_blocks, stream) != 0)
        return -1;
    stage_mark(0, stream);
    if (launch_zstd_plan_async(d_desc, nframes, d_comp, s, d_status, items, B, stream) != 0)
        return -1;
    stage_mark(1, stream);
    return launch_zstd_decode(d_desc, nframes, d_comp, d_out, d_status, s, stream, d_fail_at, stop_last, true, &B,
                              max_dsize);
}

int zstd_decode_frames_planned(const ZstdHostPlan &P, const uint64_t *d_plan, const FrameDesc *d_desc,
                               uint32_t nframes, const uint8_t *d_comp, uint8_t *d_out, int32_t *d_status,
                               ZstdScratch *s, hipStream_t stream, uint32_t *d_fail_at, uint32_t stop_last)
{
    if (nframes == 0)
        return 0;
    if (nframes > kOneMaxFrames || zstd_chunks(nframes) != 1)
        return zstd_decode_frames(d_desc, nframes, d_comp, d_out, d_status, s, stream, d_fail_at, stop_last);
    (void)hipGetLastError();   // a stale error of an earlier call is not this launch's
    stage_mark(0, stream);
    if (zstd_scratch_reserve(s, nframes, P.extent, P.items, P.blocks, stream) != 0)
        return -1;
    s->total[0] = P.items;
    s->total[1] = P.extent;
    s->total[2] = P.blocks;
    s->total[3] = P.dmax;
    s->total[4] = 0;   // one chunk: blocks [0, blocks)
    s->total[5] = P.blocks;
    stage_mark(1, stream);
    // this launch's kernels take both offset arrays from the plan's upload
    // (the scratch's own arrays are left alone)
    uint64_t *const keep_rb = s->rec_base, *const keep_bb = s->blk_base;
    s->rec_base = const_cast<uint64_t *>(d_plan);
    s->blk_base = const_cast<uint64_t *>(d_plan) + nframes + 1;
    const int rc =
        launch_zstd_decode(d_desc, nframes, d_comp, d_out, d_status, s, stream, d_fail_at, stop_last, P.cks);
    s->rec_base = keep_rb;
    s->blk_base = keep_bb;
    return rc;
}

}   // namespace zsk
