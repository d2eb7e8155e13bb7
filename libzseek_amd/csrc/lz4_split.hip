// lz4_split.hip — the two-phase LZ4-frame decoder's launcher (gfx950).
//
// Replaces the per-frame liblz4 call of the reference hot path
// (/root/reference/src/decompress.c:752-773, LZ4F_decompress in a loop) with
// one stream-ordered sequence of launches over every frame a zseek_pread
// range covers:
//
//   plan     lz4_plan_direct_kernel (lane per frame): each frame's slots in
//            the item scratch, straight from its compressed offset; frames out
//            of file order fall back to a scan by its last workgroup;
//   parse    ONE LANE PER FRAME for 64 KiB-class frames (lz4_lean.hip,
//            lz4_scan.hip for short frames) or ONE WAVE PER FRAME for big
//            frames and small batches (lz4_chunk.hip): the serial token chain
//            with liblz4 1.9.3's validation, one 8-byte item per sequence;
//   execute  ONE WAVE PER FRAME (seq_exec.hip): items in batches of 64, output
//            staged in LDS and written as whole aligned 16-byte chunks;
//   hand-off frames the parse declined (block / content checksums, zero
//            offsets, item overflow) go to the wave-per-frame decoder
//            (lz4_wave.hip), which checks XXH32 as it decodes.
//
// Which of these a batch gets is decided in lz4_route.h (lz4_plan, plain C++,
// tested on the CPU); launch_lz4_split below reserves and launches what the
// plan lists.  This file also holds the plan kernels and the scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_dev.h"
#include "pool.h"
#include "zsk_internal.h"

namespace zsk {

namespace {

using namespace lz4d;

// ---- block route plan ---------------------------------------------------------
// Lane per frame: a frame of > 64 KiB decoded and >= min_csize compressed
// bytes whose header passes every check lz4_lean_kernel's hdr_status makes
// (no checksum flags; content size, when present, equal to the seek table's
// dSize) and whose block headers chain to an end mark at exactly c_size, with
// at most kMaxBlockJobs blocks and a dSize those blocks can hold, gets one job
// per block (reserved with one atomic, written in block order).  Every other
// frame keeps kNoJob and the chunk parse decodes it as before; a reservation
// past the job slots marks the slots it got as no job.
__device__ __forceinline__ uint32_t xxh32_short(const uint8_t *c, uint32_t p, uint32_t n)
{
    uint32_t acc = 0x165667B1u + n, i = 0;
    for (; i + 4 <= n; i += 4) {
        const uint32_t w = c[p + i] | c[p + i + 1] << 8 | c[p + i + 2] << 16 | (uint32_t)c[p + i + 3] << 24;
        acc += w * 0xC2B2AE3Du;
        acc = ((acc << 17) | (acc >> 15)) * 0x27D4EB2Fu;
    }
    for (; i < n; i++) {
        acc += c[p + i] * 0x165667B1u;
        acc = ((acc << 11) | (acc >> 21)) * 0x9E3779B1u;
    }
    acc ^= acc >> 15;
    acc *= 0x85EBCA77u;
    acc ^= acc >> 13;
    acc *= 0xC2B2AE3Du;
    acc ^= acc >> 16;
    return acc;
}

struct BlockPlanArgs {
    const uint8_t *comp;
    uint32_t min_csize;
    uint32_t *bfirst, *bcount, *njobs;
    BlockJob *jobs;
    uint32_t jobs_cap, max_bsid;
};

__device__ void block_plan_frame(uint32_t f, const FrameDesc *__restrict__ desc, const BlockPlanArgs &A)
{
    const uint8_t *__restrict__ comp = A.comp;
    uint32_t *__restrict__ bfirst = A.bfirst, *__restrict__ bcount = A.bcount, *__restrict__ njobs = A.njobs;
    BlockJob *__restrict__ jobs = A.jobs;
    const uint32_t min_csize = A.min_csize, jobs_cap = A.jobs_cap, max_bsid = A.max_bsid;
    const FrameDesc d = desc[f];
    bfirst[f] = kNoJob;
    bcount[f] = 0;
    const uint32_t clen = d.c_size;
    if (d.d_size <= 65536 || clen < min_csize || clen < 15 || clen > 0x3FFFFFFFu)   // item positions: 30 bits
        return;
    const uint8_t *c = comp + d.c_off;
    auto r32 = [&](uint32_t p) -> uint32_t {
        return c[p] | c[p + 1] << 8 | c[p + 2] << 16 | (uint32_t)c[p + 3] << 24;
    };
    if (r32(0) != kLz4Magic)
        return;
    const uint32_t flg = c[4], bd = c[5];
    if ((flg & 0xC0) != 0x40 || (flg & 0x16) || (bd & 0x8F) || ((bd >> 4) & 7) < 4 || ((bd >> 4) & 7) > max_bsid)
        return;
    const uint32_t csz = (flg >> 3) & 1, dictid = flg & 1;
    const uint32_t hdr = 7 + 8 * csz + 4 * dictid;
    if (clen < hdr + 4 || ((xxh32_short(c, 4, hdr - 5) >> 8) & 0xFF) != c[hdr - 1])
        return;
    if (csz && (r32(6) != d.d_size || r32(10) != 0))
        return;
    const uint32_t bsid = (bd >> 4) & 7, max_block = 1u << (8 + 2 * bsid);
    uint32_t p = hdr, nb = 0;
    for (;;) {
        if (clen - p < 4)
            return;
        const uint32_t h = r32(p);
        if (h == 0) {
            if (clen - p != 4)
                return;
            break;
        }
        const uint32_t sz = h & 0x7FFFFFFFu;
        if (sz == 0 || sz > max_block || sz > clen - p - 8 || ++nb > kMaxBlockJobs)
            return;
        p += 4 + sz;
    }
    if ((uint64_t)(nb - 1) * max_block >= d.d_size || (uint64_t)nb * max_block < d.d_size)
        return;
    const uint32_t base = atomicAdd(njobs, nb);
    if (base >= jobs_cap || nb > jobs_cap - base) {
        for (uint32_t i = base; i < jobs_cap && i - base < nb; i++)
            jobs[i].f = kNoJob;
        return;
    }
    const uint32_t info = bsid | ((flg >> 5) & 1) << 8;
    p = hdr;
    for (uint32_t j = 0; j < nb; j++) {
        const uint32_t q = p + 4 + (r32(p) & 0x7FFFFFFFu);
        const uint32_t so = j ? (p >> 3) & ~3u : 0;
        const uint32_t se = j + 1 < nb ? (q >> 3) & ~3u : slots_of(clen);
        jobs[base + j] = BlockJob{f, p, q, so, se - so, info, j * max_block, 0};
        p = q;
    }
    bfirst[f] = base;
    bcount[f] = nb;
}

__global__ __launch_bounds__(256) void lz4_block_plan_kernel(const FrameDesc *__restrict__ desc, uint32_t n,
                                                              BlockPlanArgs A)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f < n)
        block_plan_frame(f, desc, A);
}


// ---- plan: per-frame item slot offsets ------------------------------------
// Slot offsets without a scan (the usual case): when the frames lie in order
// in the input (c_off[f+1] >= c_off[f] + c_size[f], as in every batch the
// reader builds), frame f's slots start at ceil4((c_off[f] - c_off[0]) / 8 +
// 40 f), and the gap to frame f+1 is >= c_size/8 + 37 > slots_of(c_size).  A
// frame out of order sets redo[0]; the workgroup that finishes last (redo[1]
// counts finished workgroups) then lays the slots out by a scan of
// slots_of(c_size) instead, and clears both words for the next launch on this
// scratch (zeroed at allocation).  Round 3 ran the scan as its own launch
// behind a flag memset: two launches that did nothing in the usual batch.
__global__ __launch_bounds__(256) void lz4_plan_direct_kernel(const FrameDesc *__restrict__ desc,
                                                               uint32_t n, uint64_t *__restrict__ rec_base,
                                                               uint64_t *__restrict__ total,
                                                               uint32_t *__restrict__ redo,
                                                               int32_t *__restrict__ status,
                                                               uint32_t *__restrict__ fail_at,
                                                               BlockPlanArgs bp, uint32_t by_scan)
{
    __shared__ uint64_t part[256];
    __shared__ uint32_t last;
    // the block plan's job count zeroed (bp.njobs): the block plan runs next,
    // or -- one workgroup and bp.bfirst set -- here, a lane per frame, behind
    // a barrier (one launch less: a small batch's block plan is one lane's
    // walk over a frame's block headers)
    if (bp.njobs && blockIdx.x == 0 && threadIdx.x == 0)
        *bp.njobs = 0;
    if (bp.bfirst && gridDim.x == 1) {
        __syncthreads();
        for (uint32_t f = threadIdx.x; f < n; f += 256)
            block_plan_frame(f, desc, bp);
    }
    // at most kPlanGroups workgroups (the finish counter is one atomic per
    // workgroup: 4,096 of them cost 0.11 ms at 1,048,576 frames), each thread
    // striding over its frames
    const uint64_t c0 = desc[0].c_off;
    for (uint32_t f = blockIdx.x * 256 + threadIdx.x; f < n; f += gridDim.x * 256) {
        // every frame starts as not run (a parse kernel then owns it), with no
        // failing block: the reader needs no fills of its own
        status[f] = ST_NOT_RUN;
        if (fail_at)
            fail_at[f] = 0;
        const FrameDesc d = desc[f];
        const uint64_t r = (((d.c_off - c0) >> 3) + 40ull * f + 3) & ~3ull;
        rec_base[f] = r;
        if (d.c_off < c0 || (f + 1 < n && desc[f + 1].c_off < d.c_off + d.c_size))
            atomicOr(&redo[0], 1u);
        if (f + 1 == n)
            *total = r + slots_of(d.c_size);
    }
    if (n == 1)   // one frame is always in order
        return;
    // by_scan: the caller's frames lie anywhere in the input (sparse frames of
    // a device image, padding descriptors among them): the slots by the scan
    // whatever their order, so the scratch they take is the sum of
    // slots_of(c_size) and never the compressed distance they span
    if (by_scan && threadIdx.x == 0)
        atomicOr(&redo[0], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(&redo[1], 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!last)
        return;
    __threadfence();
    if (atomicOr(&redo[0], 0u)) {
        const uint32_t t = threadIdx.x;
        const uint32_t chunk = (n + 255) / 256;
        const uint32_t i0 = t * chunk < n ? t * chunk : n;
        const uint32_t i1 = i0 + chunk < n ? i0 + chunk : n;
        uint64_t sum = 0;
        for (uint32_t i = i0; i < i1; i++)
            sum += slots_of(desc[i].c_size);
        part[t] = sum;
        __syncthreads();
        for (uint32_t k = 1; k < 256; k <<= 1) {
            const uint64_t v = t >= k ? part[t - k] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        uint64_t run = part[t] - sum;
        for (uint32_t i = i0; i < i1; i++) {
            rec_base[i] = run;
            run += slots_of(desc[i].c_size);
        }
        if (t == 255)
            *total = part[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        redo[0] = 0;
        redo[1] = 0;
    }
}


}   // namespace

// ---- scratch -----------------------------------------------------------------

uint64_t split_items_needed(const FrameDesc *h_desc, uint32_t n)
{
    uint64_t s = 0;
    for (uint32_t i = 0; i < n; i++)
        s += slots_of(h_desc[i].c_size);
    // where lz4_plan_direct_kernel's layout ends (frames in order)
    if (n && h_desc[n - 1].c_off >= h_desc[0].c_off) {
        const uint64_t last = (((h_desc[n - 1].c_off - h_desc[0].c_off) >> 3) + 40ull * (n - 1) + 3) & ~3ull;
        const uint64_t d = last + slots_of(h_desc[n - 1].c_size);
        if (d > s)
            s = d;
    }
    return s;
}

uint64_t split_items_default(const SplitScratch *s, uint32_t nframes, uint64_t known)
{
    uint64_t want = known;
    if (!want) {
        want = (uint64_t)nframes * slots_of(65536 + 64);
        if (want > (512ull << 20))
            want = 512ull << 20;
    }
    if (s->total && *s->total > want)
        want = *s->total;
    return want;
}

namespace {
template <class T> void drop(T *&p)   // device memory freed and forgotten
{
    if (p)
        (void)hipFree(p);
    p = nullptr;
}
}   // namespace

void split_scratch_free(SplitScratch *s)
{
    drop(s->rec_base);
    drop(s->nitems);
    drop(s->items);
    if (s->total)
        (void)hipHostFree(s->total);
    drop(s->redo);
    drop(s->bfirst);
    drop(s->bcount);
    drop(s->njobs);
    drop(s->jobs);
    drop(s->jres);
    drop(s->borg);
    drop(s->btaint);
    *s = SplitScratch();
}

namespace {
// block route scratch for (frames, jobs); stream-ordered like the rest
int block_scratch_reserve(SplitScratch *s, uint32_t frames, uint32_t jobs, hipStream_t stream)
{
    if (!s->njobs && hipMalloc((void **)&s->njobs, sizeof(uint32_t)) != hipSuccess)
        return -1;
    if (frames > s->bframes_cap) {
        const uint32_t cap = frames < 1024 ? 1024 : frames;
        (void)hipStreamSynchronize(stream);
        drop(s->bfirst);
        drop(s->bcount);
        s->bframes_cap = 0;
        if (hipMalloc((void **)&s->bfirst, (size_t)cap * 4) != hipSuccess ||
            hipMalloc((void **)&s->bcount, (size_t)cap * 4) != hipSuccess)
            return -1;
        s->bframes_cap = cap;
    }
    if (jobs > s->jobs_cap) {
        (void)hipStreamSynchronize(stream);
        drop(s->jobs);
        drop(s->jres);
        s->jobs_cap = 0;
        if (hipMalloc((void **)&s->jobs, (size_t)jobs * sizeof(BlockJob)) != hipSuccess ||
            hipMalloc((void **)&s->jres, (size_t)jobs * sizeof(BlockRes)) != hipSuccess)
            return -1;
        s->jobs_cap = jobs;
    }
    return 0;
}

// the block-parallel execute's scratch for `jobs` jobs (136 KiB each)
int origin_scratch_reserve(SplitScratch *s, uint32_t jobs, hipStream_t stream)
{
    if (jobs <= s->borg_cap)
        return 0;
    (void)hipStreamSynchronize(stream);
    drop(s->borg);
    drop(s->btaint);
    s->borg_cap = 0;
    const uint32_t cap = jobs < 16 ? 16 : jobs;
    if (hipMalloc((void **)&s->borg, (size_t)cap * 65536 * sizeof(uint16_t)) != hipSuccess ||
        hipMalloc((void **)&s->btaint, (size_t)cap * 2048 * sizeof(uint32_t)) != hipSuccess)
        return -1;
    s->borg_cap = cap;
    return 0;
}
}   // namespace

int split_scratch_reserve(SplitScratch *s, uint32_t frames, uint64_t items, hipStream_t stream)
{
    if (!s->total) {
        if (hipHostMalloc((void **)&s->total, sizeof(uint64_t), hipHostMallocMapped) != hipSuccess)
            return -1;
        *s->total = 0;
    }
    if (!s->redo) {   // [out-of-order flag, plan workgroups done]: zero between launches
        if (hipMalloc((void **)&s->redo, 2 * sizeof(uint32_t)) != hipSuccess)
            return -1;
        if (hipMemsetAsync(s->redo, 0, 2 * sizeof(uint32_t), stream) != hipSuccess) {
            drop(s->redo);
            return -1;
        }
    }
    if (frames > s->frames_cap) {
        uint32_t cap = frames < 4096 ? 4096 : frames;
        (void)hipStreamSynchronize(stream);
        drop(s->rec_base);
        drop(s->nitems);
        s->frames_cap = 0;
        if (hipMalloc((void **)&s->rec_base, (size_t)cap * 8) != hipSuccess ||
            hipMalloc((void **)&s->nitems, (size_t)cap * 4) != hipSuccess)
            return -1;
        s->frames_cap = cap;
    }
    if (items > s->items_cap) {
        uint64_t cap = items + items / 8;
        (void)hipStreamSynchronize(stream);
        drop(s->items);
        s->items_cap = 0;
        if (hipMalloc((void **)&s->items, cap * 8 + 64) != hipSuccess)
            return -1;
        s->items_cap = cap;
    }
    return 0;
}

// ---- routing: lz4_route.h over this process's switches -------------------------

const Lz4Switches &lz4_switches()
{
    static const Lz4Switches w = lz4_switches_env();
    return w;
}

const char *parse_kernel_name(uint32_t nframes, uint32_t c_size, int route)
{
    return lz4_parse_kernel_name(nframes, c_size, route, lz4_switches());
}

int lz4_pick_engine(uint32_t nframes)
{
    return lz4_pick_engine(nframes, lz4_switches());
}

const char *lz4_kernel_name(uint32_t nframes)
{
    return lz4_exec_kernel_name(nframes, lz4_switches());
}

// ---- the launcher --------------------------------------------------------------
// Plan (lz4_route.h), reserve what the plan asks for, re-plan without what
// was denied, then the plan's steps in order.
int launch_lz4_split(const Lz4Request &rq, const Lz4Buffers &b, hipStream_t stream, SplitScratch *s,
                     const HostPost *post, bool *posted)
{
    if (posted)
        *posted = false;
    const uint32_t n = rq.nframes;
    if (n == 0)
        return 0;
    if (s->frames_cap < n || !s->rec_base || !s->redo)
        return -1;
    (void)hipGetLastError();   // a stale error of an earlier call is not this launch's
    uint64_t *total_dev = nullptr;
    (void)hipHostGetDevicePointer((void **)&total_dev, s->total, 0);
    Lz4Request q = rq;
    Lz4Plan P = lz4_plan(q, lz4_switches());
    if (P.block.on && block_scratch_reserve(s, n, P.jlanes, stream) != 0) {
        q.block_denied = true;
        P = lz4_plan(q, lz4_switches());
    }
    if (P.origin_jobs && origin_scratch_reserve(s, P.origin_jobs, stream) != 0) {
        q.origin_denied = true;
        P = lz4_plan(q, lz4_switches());
    }
    SplitScratch *const blk = P.block.on ? s : nullptr;
    const uint64_t cap = s->items_cap;

    stage_mark(0, stream);
    if (P.plan) {
        BlockPlanArgs bp{b.d_comp, P.block.min_csize, nullptr, nullptr, nullptr, nullptr, P.jlanes, P.block.max_bsid};
        if (blk) {
            bp.bfirst = s->bfirst;
            bp.bcount = s->bcount;
            bp.njobs = s->njobs;
            bp.jobs = s->jobs;
        }
        // (a block plan behind the plan: the plan only zeroes its job count)
        BlockPlanArgs pbp = bp;
        if (P.block_plan != BLOCK_PLAN_INSIDE)
            pbp.bfirst = nullptr;
        hipLaunchKernelGGL(lz4_plan_direct_kernel, dim3(P.plan_groups), dim3(256), 0, stream, b.d_desc, n, s->rec_base,
                           total_dev, s->redo, b.d_status, b.d_fail_at, pbp, P.scan_layout ? 1u : 0u);
        if (P.block_plan == BLOCK_PLAN_SEPARATE)
            hipLaunchKernelGGL(lz4_block_plan_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, b.d_desc, n, bp);
    }
    stage_mark(1, stream);
    if (P.job_parse)
        launch_lz4_job_parse(b.d_desc, b.d_comp, s->rec_base, cap, s->items, s, P.jlanes, stream);
    if (P.lean_blocks)
        launch_lz4_lean_blocks(b.d_desc, b.d_comp, s->rec_base, cap, s->items, s, P.jlanes, P.block.min_jobs, stream);
    if (P.lean)
        launch_lz4_lean(b.d_desc, n, b.d_comp, s->rec_base, cap, s->items, s->nitems, b.d_status, b.d_fail_at, stream,
                        P.lean_max, P.lean_diag, P.lean_min);
    if (P.scan)
        launch_lz4_scan(b.d_desc, n, b.d_comp, s->rec_base, cap, s->items, s->nitems, b.d_status, b.d_fail_at, stream,
                        P.scan_max);
    if (P.chunk)
        launch_lz4_chunk(b.d_desc, n, b.d_comp, s->rec_base, cap, s->items, s->nitems, b.d_status, b.d_fail_at, stream,
                         P.parse.chunk_min, blk, P.block.min_jobs, P.chunk_one, P.chunk_solo ? total_dev : nullptr);
    stage_mark(2, stream);
    if (P.exec_frames)
        launch_seq_exec_frames(b.d_desc, n, b.d_comp, b.d_out, s->rec_base, s->items, s->nitems, b.d_status,
                               b.d_fail_at, stream, rq.stop_last, P.handoff, nullptr, P.post_here ? post : nullptr);
    if (P.post_here && posted)
        *posted = true;
    if (P.exec_blocks)
        launch_seq_exec_blocks(b.d_desc, n, b.d_comp, b.d_out, s->rec_base, s->items, stream, rq.stop_last, s,
                               P.jlanes);
    if (P.exec_big)
        launch_seq_exec_big(b.d_desc, n, b.d_comp, b.d_out, s->rec_base, s->items, s->nitems, b.d_status, b.d_fail_at,
                            stream, rq.stop_last, P.handoff, s, P.big_skip_origin ? s->borg_cap : 0u);
    if (P.exec_wave)
        launch_seq_exec(b.d_desc, n, b.d_comp, b.d_out, s->rec_base, s->items, s->nitems, b.d_status, stream,
                        P.wave_version, P.wave_blk ? s : nullptr, rq.stop_last, P.wave_min_dsize);
    stage_mark(3, stream);
    if (hipGetLastError() != hipSuccess) {
        // a plan cut short may leave its finish counter or out-of-order flag
        // set: the next plan on this scratch must start from zero
        (void)hipMemsetAsync(s->redo, 0, 2 * sizeof(uint32_t), stream);
        (void)hipGetLastError();
        stage_mark(4, stream);
        return -1;
    }
    int rc = 0;
    if (P.deferred)
        rc = launch_lz4_wave_deferred(b.d_desc, n, b.d_comp, b.d_out, b.d_status, b.d_fail_at, stream);
    stage_mark(4, stream);
    return rc;
}

// Public device API (zsk_lz4_decode_frames): the host does not see the
// descriptors, so scratch comes from a per-device pool and is sized before
// the plan runs: from the compressed bytes d_comp's allocation can hold past
// d_comp (hipMemGetAddressRange) -- the plan lays frames out at
// (c_off - c_off[0]) / 8 + 40 f, so span / 8 + 44 n + 64 slots always fit
// frames stored in file order in that span, whatever their size -- capped at
// what n frames of up to 4 MiB compressed can use (a caller's span may sit in
// a multi-GiB arena: a few frames must not reserve GiBs), else for 64 KiB
// frames (split_items_default); and never below the item total the previous
// plan on that set reported.  Frames that still do not fit go to the wave
// kernel and the next call grows.  (Round 3 sized a first call for 64 KiB
// frames only, so a first call over 1 MiB frames handed every frame to the
// wave kernel.)
// `route` (ROUTE_*) forces one production decoder for every frame (tests).
int launch_lz4_frames(const FrameDesc *d_desc, uint32_t nframes, const uint8_t *d_comp,
                      uint8_t *d_out, int32_t *d_status, uint32_t *d_fail_at, hipStream_t stream,
                      int route, int tune)
{
    if (nframes == 0)
        return 0;
    Lz4Request rq;
    rq.nframes = nframes;
    rq.route = route;
    rq.tune = tune;
    if (lz4_plan(rq, lz4_switches()).klass == LZ4_WAVE_ENGINE)
        return launch_lz4_wave(d_desc, nframes, d_comp, d_out, d_status, d_fail_at, stream);
    static ScratchPool<SplitScratch> pool;
    SplitScratch *s = pool.acquire(stream);
    if (!s)
        return -1;
    uint64_t known = 0;
    hipDeviceptr_t base = 0;
    size_t bytes = 0;
    if (hipMemGetAddressRange(&base, &bytes, (hipDeviceptr_t)d_comp) == hipSuccess && bytes &&
        (uintptr_t)d_comp >= (uintptr_t)base && (uintptr_t)d_comp < (uintptr_t)base + bytes) {
        const uint64_t span = (uintptr_t)base + bytes - (uintptr_t)d_comp;
        uint64_t by_span = span / 8 + 44ull * nframes + 64;
        const uint64_t by_frames = (uint64_t)nframes * slots_of((4u << 20) + 64) + 64;
        if (by_span > by_frames)
            by_span = by_frames;
        if (by_span <= (1ull << 30))   // up to 8 GiB of items
            known = by_span;
    }
    (void)hipGetLastError();   // (a failed range query is not this launch's error)
    int rc;
    if (split_scratch_reserve(s, nframes, split_items_default(s, nframes, known), stream) != 0) {
        (void)hipGetLastError();   // the failed allocation is not the wave launch's error
        rc = launch_lz4_wave(d_desc, nframes, d_comp, d_out, d_status, d_fail_at, stream);
    }
    else
        rc = launch_lz4_split(rq, {d_desc, d_comp, d_out, d_status, d_fail_at}, stream, s);
    pool.release(s, stream);
    return rc;
}

}   // namespace zsk
