// zstd_plan.hip -- the zstd decoder's plan: per entry the item and block slots
// it needs (zstd_plan.h's walk), their scans into slot offsets, the block
// offsets at the chunk boundaries; the same on the host for a few frames; and
// the census of a whole file in device memory (the walk's maxima).
#include <algorithm>

#include "lz4_dev.h"
#include "zstd_internal.h"
#include "zstd_plan.h"

namespace zsk {
namespace {

using namespace lz4d;

// zstd_plan.h's walk over the c_size bytes at p, through a buffer resource of
// the entry's own: a byte at or past c_size reads as 0 and nothing outside the
// entry is loaded
__device__ __forceinline__ ZstdFramePlan entry_plan(const uint8_t *p, uint32_t c_size)
{
    const Span sp = make_span(p, c_size);
    return zstd_frame_plan(
        [&](uint32_t i) -> uint32_t {
            return i < c_size ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(sp.r, sp.s0 + i, 0, 0) : 0u;
        },
        c_size);
}

// item bound per frame (lane per frame): 2 items per sequence + padding + 4 per
// block; and the frame's block count (its table slots and op list)
__global__ __launch_bounds__(256) void zstd_plan_kernel(
    const FrameDesc *__restrict__ desc, uint32_t n, const uint8_t *__restrict__ comp,
    uint32_t *__restrict__ bound, uint32_t *__restrict__ bblk, unsigned long long *__restrict__ extent)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    FrameDesc d = {0, 0, 0, 0};
    if (f < n)
        d = desc[f];
    // the output extent max(d_off + d_size), a wave at a time (the scan then
    // reads no descriptors)
    // (and the largest frame, extent[2]: whether the one-frame route's
    // execute needs a wave kernel beside its workgroups)
    const uint64_t wx = wave_max64(f < n ? d.d_off + d.d_size : 0ull);
    const uint64_t wd = wave_max64(f < n ? d.d_size : 0ull);
    if ((threadIdx.x & 63) == 0 && wx)
        atomicMax(extent, (unsigned long long)wx);
    if ((threadIdx.x & 63) == 0 && wd)
        atomicMax(extent + 2, (unsigned long long)wd);
    if (f >= n)
        return;
    const ZstdFramePlan P = entry_plan(comp + d.c_off, d.c_size);
    bound[f] = P.bound;
    bblk[f] = P.blocks;
}

// The census of a whole file in device memory (zsk_reader_zstd_census): a lane
// per seek-table entry, entry f the image's bytes [c_off[f], c_off[f + 1]);
// the largest item bound, block count and sequence count of any one entry,
// a wave at a time, into words[0..2] (zeroed by the launcher).
__global__ __launch_bounds__(256) void zstd_census_kernel(
    const uint64_t *__restrict__ c_off, uint32_t n, const uint8_t *__restrict__ image,
    unsigned long long *__restrict__ words)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    ZstdFramePlan P = {0, 0, false, 0};
    if (f < n) {
        const uint64_t c0 = c_off[f];
        P = entry_plan(image + c0, (uint32_t)(c_off[f + 1] - c0));
    }
    // (every lane of the wave is here again: a lane past n holds zeros)
    const uint64_t wi = wave_max64(P.bound), wb = wave_max64(P.blocks), ws = wave_max64(P.sequences);
    if ((threadIdx.x & 63) != 0)
        return;
    if (wi)
        atomicMax(words, (unsigned long long)wi);
    if (wb)
        atomicMax(words + 1, (unsigned long long)wb);
    if (ws)
        atomicMax(words + 2, (unsigned long long)ws);
}

// exclusive scans of the per-frame item bounds and block counts ->
// rec_base[0..n], blk_base[0..n]; item total, output extent max(d_off +
// d_size) and block total into total[0..2] (device memory, copied to the host
// by the launcher; one workgroup)
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(1024) void zstd_scan_kernel(
    const uint32_t *__restrict__ bound, const uint32_t *__restrict__ bblk, uint32_t n,
    uint64_t *__restrict__ rec_base, uint64_t *__restrict__ blk_base, uint64_t *__restrict__ total)
{
    // tiles of 4096 frames, four per thread, loaded 16 bytes at a time
    // (coalesced) and scanned a wave at a time; a thread per frame chunk with
    // a dependent load per element cost ~0.3 ms at 65,536 frames
    __shared__ uint64_t wsum[16], wsumb[16];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint64_t carry = 0, carryb = 0;
    auto load4 = [&](const uint32_t *a, uint32_t x) -> u32x4 {
        if (x + 4 <= n)
            return *reinterpret_cast<const u32x4 *>(a + x);
        u32x4 v = {0, 0, 0, 0};
        for (uint32_t q = 0; q < 4; q++)
            if (x + q < n)
                v[q] = a[x + q];
        return v;
    };
    const uint32_t x0 = 4 * t;
    u32x4 a = load4(bound, x0), c = load4(bblk, x0);
    for (uint32_t b = 0; b < n; b += 4096) {
        const uint32_t x = b + x0;
        const u32x4 ca = a, cc = c;
        if (b + 4096 < n) {   // the next tile's loads in flight during this one's scan
            a = load4(bound, x + 4096);
            c = load4(bblk, x + 4096);
        }
        const uint64_t s = (uint64_t)ca.x + ca.y + ca.z + ca.w;
        const uint64_t sb = (uint64_t)cc.x + cc.y + cc.z + cc.w;
        uint64_t is = s, isb = sb;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t v = __shfl_up(is, d, 64), vb = __shfl_up(isb, d, 64);
            if (lane >= d) {
                is += v;
                isb += vb;
            }
        }
        if (lane == 63) {
            wsum[w] = is;
            wsumb[w] = isb;
        }
        __syncthreads();
        uint64_t pre = carry, preb = carryb, tot = carry, totb = carryb;
        for (uint32_t k = 0; k < 16; k++) {
            pre += k < w ? wsum[k] : 0;
            preb += k < w ? wsumb[k] : 0;
            tot += wsum[k];
            totb += wsumb[k];
        }
        __syncthreads();   // wsum free for the next tile
        uint64_t r = pre + is - s, rb = preb + isb - sb;
        if (x < n) {
            const uint64_t r1 = r + ca.x, r2 = r1 + ca.y, r3 = r2 + ca.z;
            const uint64_t q1 = rb + cc.x, q2 = q1 + cc.y, q3 = q2 + cc.z;
            if (x + 4 <= n) {
                *reinterpret_cast<u64x2 *>(rec_base + x) = (u64x2){r, r1};
                *reinterpret_cast<u64x2 *>(rec_base + x + 2) = (u64x2){r2, r3};
                *reinterpret_cast<u64x2 *>(blk_base + x) = (u64x2){rb, q1};
                *reinterpret_cast<u64x2 *>(blk_base + x + 2) = (u64x2){q2, q3};
            } else {
                const uint64_t rr[4] = {r, r1, r2, r3}, qq[4] = {rb, q1, q2, q3};
                for (uint32_t q = 0; x + q < n; q++) {
                    rec_base[x + q] = rr[q];
                    blk_base[x + q] = qq[q];
                }
            }
        }
        carry = tot;
        carryb = totb;
    }
    if (t == 0) {
        rec_base[n] = carry;
        blk_base[n] = carryb;
        total[0] = carry;
        total[2] = carryb;
    }
}

// blk_base at the decode's chunk boundaries (zstd_chunks) -> out[0..k]
__global__ void zstd_bounds_kernel(const uint64_t *__restrict__ blk_base, uint32_t n, uint32_t k,
                                   uint64_t *__restrict__ out)
{
    const uint32_t c = threadIdx.x;
    if (c <= k)
        out[c] = blk_base[(uint64_t)n * c / k];
}

// The asynchronous decode's verdict, behind the scan (a thread per frame; every
// thread reads the three totals, wave-uniform): the batch fits when its item
// total, block total and output extent are within what the host reserved.
// Then zstd_bounds_kernel's chunk boundaries, else boundaries of 0 (no Huffman
// job anywhere), the verdict word set and every status ST_NOT_RUN, at which
// the execute kernels return at their top; zstd_check_kernel, the call's last,
// turns it into ST_SCRATCH.  (total[0..2] are only read here, total[4..] and
// the verdict only written.)
__global__ __launch_bounds__(256) void zstd_fit_kernel(
    const uint64_t *__restrict__ blk_base, uint32_t n, uint32_t k, uint64_t *total, uint64_t items_cap,
    uint64_t max_blocks, uint64_t out_bytes, int32_t *__restrict__ status)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    const bool fits = total[0] <= items_cap && total[2] <= max_blocks && total[1] <= out_bytes;
    if (f <= k)
        total[4 + f] = fits ? blk_base[(uint64_t)n * f / k] : 0;
    if (f == 0)
        total[ZstdScratch::kFitWord] = fits ? 0 : 1;
    if (!fits && f < n)
        status[f] = ST_NOT_RUN;
}

int plan_kernels(const FrameDesc *d_desc, uint32_t nframes, const uint8_t *d_comp, ZstdScratch *s,
                 hipStream_t stream)
{
    if (hipMemsetAsync(s->d_total, 0, 4 * sizeof(uint64_t), stream) != hipSuccess)
        return -1;
    hipLaunchKernelGGL(zstd_plan_kernel, dim3((nframes + 255) / 256), dim3(256), 0, stream, d_desc,
                       nframes, d_comp, s->bound, s->bblk, reinterpret_cast<unsigned long long *>(s->d_total + 1));
    hipLaunchKernelGGL(zstd_scan_kernel, dim3(1), dim3(1024), 0, stream, s->bound, s->bblk, nframes,
                       s->rec_base, s->blk_base, s->d_total);
    return 0;
}

}   // namespace

int launch_zstd_plan_async(const FrameDesc *d_desc, uint32_t nframes, const uint8_t *d_comp, ZstdScratch *s,
                           int32_t *d_status, uint64_t items_cap, const ZstdBounds &B, hipStream_t stream)
{
    if (nframes == 0)
        return 0;
    if (plan_kernels(d_desc, nframes, d_comp, s, stream) != 0)
        return -1;
    // (a grid of at least kChunks + 1 threads: the boundaries)
    hipLaunchKernelGGL(zstd_fit_kernel, dim3((nframes + 255) / 256), dim3(256), 0, stream, s->blk_base, nframes,
                       zstd_chunks(nframes), s->d_total, items_cap, B.max_blocks, B.out_bytes, d_status);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The census kernel over the n entries of the image whose table is d_coff
// (n + 1 offsets), behind a memset of its three words.
int launch_zstd_census(const uint64_t *d_coff, uint32_t n, const uint8_t *d_image, uint64_t *d_words,
                       hipStream_t stream)
{
    if (hipMemsetAsync(d_words, 0, kCensusWords * sizeof(uint64_t), stream) != hipSuccess)
        return -1;
    if (n == 0)
        return 0;
    hipLaunchKernelGGL(zstd_census_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_coff, n, d_image,
                       reinterpret_cast<unsigned long long *>(d_words));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Plan only: bounds + offsets, then the item total, output extent and block
// total copied into s->total (pinned host memory), valid once the stream
// reaches it.
int launch_zstd_plan(const FrameDesc *d_desc, uint32_t nframes, const uint8_t *d_comp,
                     ZstdScratch *s, hipStream_t stream)
{
    if (nframes == 0)
        return 0;
    if (plan_kernels(d_desc, nframes, d_comp, s, stream) != 0)
        return -1;
    const uint32_t k = zstd_chunks(nframes);
    hipLaunchKernelGGL(zstd_bounds_kernel, dim3(1), dim3(64), 0, stream, s->blk_base, nframes, k, s->d_total + 4);
    if (hipGetLastError() != hipSuccess)
        return -1;
    return hipMemcpyAsync(s->total, s->d_total, (5 + k) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream) ==
                   hipSuccess
               ? 0
               : -1;
}

// The plan of a request's few frames on the host, from the reader's pinned
// copy of their bytes: zstd_plan_kernel's bounds and zstd_scan_kernel's sums.
void zstd_host_plan(const FrameDesc *h_desc, const uint8_t *h_comp, uint32_t nframes, uint64_t *h_plan,
                    ZstdHostPlan *P)
{
    uint64_t items = 0, blocks = 0, extent = 0, dmax = 0;
    uint64_t *const rb = h_plan, *const bb = h_plan + nframes + 1;
    bool cks = false;
    for (uint32_t f = 0; f < nframes; f++) {
        const FrameDesc &d = h_desc[f];
        const uint8_t *c = h_comp + d.c_off;
        const ZstdFramePlan fp =
            zstd_frame_plan([&](uint32_t p) -> uint32_t { return p < d.c_size ? (uint32_t)c[p] : 0u; }, d.c_size);
        rb[f] = items;
        bb[f] = blocks;
        items += fp.bound;
        blocks += fp.blocks;
        cks = cks || fp.cks;
        extent = std::max<uint64_t>(extent, d.d_off + d.d_size);
        dmax = std::max<uint64_t>(dmax, d.d_size);
    }
    rb[nframes] = items;
    bb[nframes] = blocks;
    *P = ZstdHostPlan{items, blocks, extent, dmax, cks};
}

}   // namespace zsk
