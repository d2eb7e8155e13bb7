// range_gather.hip — the segmented byte copy behind zsk_preadv and
// zsk_gather_segments (gfx950).
//
// A launch copies src[src_off, +len) to dst[dst_off, +len) for every segment
// (zsk_segment_t) whose frame decoded cleanly.  Segments come in any number
// (one to hundreds of thousands), any length (0 .. 4 GiB - 1) and at any byte
// alignment on both sides, so the work is split by BYTES: the segments'
// lengths are laid end to end (their prefix sum, `cum`), that stream is cut
// into tiles of kTile bytes, and a workgroup takes tiles in a grid-stride loop
// (the tile count is read on the device: the caller of zsk_gather_segments
// never synchronizes to learn it).  One 64 MiB segment is 4,096 tiles; 4,000
// segments of 40 bytes share ten.
//
// Inside a tile the unit is a 16-byte-aligned DESTINATION chunk.  The tile's
// segments are taken kGatherT at a time (one per thread): each thread cuts its
// segment to the tile, counts the chunks its part touches, a workgroup scan
// turns the counts into a flat chunk index, and the threads then take the
// chunks kGatherT apart -- consecutive lanes on consecutive 16-byte chunks of
// a long segment (coalesced dwordx4 on both sides), or on the few chunks of
// many short ones.  A chunk wholly inside its segment is one 16-byte store,
// fed by one 16-byte load when source and destination are co-aligned mod 16,
// else by four or five aligned dwords realigned with v_alignbyte (the window
// d2h_small_kernel uses, host_io.hip); every one of those dwords holds at
// least one byte of the chunk, so no load leaves the 4-byte words that
// contain the segment.  A part's first and last chunk, when partial, go byte
// by byte.  Nothing outside [dst_off, dst_off + len) is written: there is no
// read-modify-write and no rounded-up store.  Plain vector loads and stores
// only.
//
// Zero-length and skipped segments cost a slot of their pass and nothing else
// (the reader's planner emits no empty segment).
//
// A thread loads up to kGatherU chunks before it stores the first (memory
// parallelism; the compiler may not reorder them itself: src and dst can
// alias for all it knows).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "block_scan.h"
#include "pool.h"
#include "zsk_internal.h"

namespace zsk {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kGatherT = 256;      // threads per workgroup
constexpr uint32_t kTile = 16384;       // bytes of the segment stream per tile (1,024 chunks: 4 per thread)
constexpr uint32_t kGatherU = 4;        // chunks a thread has in flight
constexpr uint32_t kGatherGrid = 2048;  // most workgroups (8 per CU: every wave slot of 256 CUs)
constexpr uint32_t kScanT = 1024;

// cum[0 .. nseg]: the prefix sum of the segments' lengths, by one workgroup
// (each thread a contiguous share of the segments).
__global__ __launch_bounds__(kScanT) void range_scan_kernel(const GatherSeg *__restrict__ seg, uint32_t nseg,
                                                            uint64_t *__restrict__ cum)
{
    __shared__ uint64_t s_sum[kScanT];
    const uint32_t t = threadIdx.x;
    uint32_t a, b;
    block_share<kScanT>(nseg, t, &a, &b);
    uint64_t sum = 0;
    for (uint32_t i = a; i < b; i++)
        sum += seg[i].len;
    uint64_t run = block_scan_inclusive<kScanT>(s_sum, t, sum) - sum;   // (block_scan.h)
    if (t == 0)
        cum[0] = 0;
    for (uint32_t i = a; i < b; i++) {
        run += seg[i].len;
        cum[i + 1] = run;
    }
}

__global__ __launch_bounds__(kGatherT) void range_gather_kernel(const GatherSeg *__restrict__ seg,
                                                                const uint64_t *__restrict__ cum, uint32_t nseg,
                                                                const uint8_t *src, uint8_t *dst,
                                                                const int32_t *__restrict__ status)
{
    // the parts (segment cut to the tile) of this pass: source and destination
    // address of the part's first byte, its length, its first flat chunk
    __shared__ uint64_t s_src[kGatherT], s_dst[kGatherT];
    __shared__ uint32_t s_len[kGatherT], s_first[kGatherT + 1], s_wave[kGatherT / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t total = cum[nseg];
    const uint64_t ntiles = (total + kTile - 1) / kTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * kTile, t1 = std::min<uint64_t>(total, t0 + kTile);
        // the first segment that reaches past t0 (t0 < total: there is one)
        uint32_t lo = 0, hi = nseg;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (cum[mid + 1] > t0)
                hi = mid;
            else
                lo = mid + 1;
        }
        for (uint32_t s0 = lo;;) {
            const uint32_t s = s0 + t;
            uint32_t nch = 0, len = 0;
            uint64_t sa = 0, da = 0;
            if (s < nseg) {
                const uint64_t c0 = cum[s], c1 = cum[s + 1];
                if (c0 < t1 && c1 > c0) {
                    const GatherSeg g = seg[s];
                    if (!status || status[g.frame] == 0) {
                        const uint64_t a = std::max<uint64_t>(c0, t0) - c0, b = std::min<uint64_t>(c1, t1) - c0;
                        len = (uint32_t)(b - a);
                        sa = reinterpret_cast<uint64_t>(src) + g.src_off + a;
                        da = reinterpret_cast<uint64_t>(dst) + g.dst_off + a;
                        nch = (uint32_t)(((da + len + 15) >> 4) - (da >> 4));
                    }
                }
            }
            s_src[t] = sa;
            s_dst[t] = da;
            s_len[t] = len;
            uint32_t x = nch;   // inclusive scan of the chunk counts: the wave, then the waves
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x, d);
                if (lane >= d)
                    x += y;
            }
            if (lane == 63)
                s_wave[wave] = x;
            __syncthreads();
            uint32_t base = 0;
            for (uint32_t w = 0; w < wave; w++)
                base += s_wave[w];
            s_first[t] = base + x - nch;
            if (t == kGatherT - 1)
                s_first[kGatherT] = base + x;
            __syncthreads();
            const uint32_t chunks = s_first[kGatherT];
            for (uint32_t i0 = t; i0 < chunks; i0 += kGatherT * kGatherU) {
                u32x4 v[kGatherU];
                uint64_t cs[kGatherU], cd[kGatherU];   // source / destination address of the chunk's first byte
                uint32_t cn[kGatherU];                 // its bytes (16: one aligned store; 0: none)
#pragma unroll
                for (uint32_t k = 0; k < kGatherU; k++) {
                    const uint32_t i = i0 + k * kGatherT;
                    cn[k] = 0;
                    if (i >= chunks)
                        continue;
                    uint32_t p = 0, q = kGatherT;   // the last part whose first chunk is <= i
                    while (p + 1 < q) {
                        const uint32_t m = (p + q) / 2;
                        if (s_first[m] <= i)
                            p = m;
                        else
                            q = m;
                    }
                    const uint64_t d0 = s_dst[p], d1 = d0 + s_len[p];
                    const uint64_t c = (d0 & ~15ull) + 16ull * (i - s_first[p]);
                    const uint64_t from = std::max(c, d0), to = std::min(c + 16, d1);
                    cd[k] = from;
                    cs[k] = s_src[p] + (from - d0);
                    cn[k] = (uint32_t)(to - from);
                    if (cn[k] != 16)
                        continue;
                    if (!(cs[k] & 15)) {
                        v[k] = *reinterpret_cast<const u32x4 *>(cs[k]);
                    } else {
                        const uint32_t sh = (uint32_t)(cs[k] & 3);
                        const uint32_t *w = reinterpret_cast<const uint32_t *>(cs[k] - sh);
                        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
                        const uint32_t w4 = sh ? w[4] : 0;   // (sh == 0: the chunk ends with w3)
                        v[k].x = __builtin_amdgcn_alignbyte(w1, w0, sh);
                        v[k].y = __builtin_amdgcn_alignbyte(w2, w1, sh);
                        v[k].z = __builtin_amdgcn_alignbyte(w3, w2, sh);
                        v[k].w = __builtin_amdgcn_alignbyte(w4, w3, sh);
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < kGatherU; k++) {
                    if (cn[k] == 16) {
                        *reinterpret_cast<u32x4 *>(cd[k]) = v[k];
                    } else {
                        const uint8_t *ps = reinterpret_cast<const uint8_t *>(cs[k]);
                        uint8_t *pd = reinterpret_cast<uint8_t *>(cd[k]);
                        for (uint32_t b = 0; b < cn[k]; b++)
                            pd[b] = ps[b];
                    }
                }
            }
            __syncthreads();   // (the next pass rewrites the parts)
            s0 += kGatherT;
            if (s0 >= nseg || cum[s0] >= t1)
                break;
        }
    }
}

struct GatherScratch {
    uint64_t *cum = nullptr;
    size_t cap = 0;
};

}   // namespace

int launch_range_gather(const GatherSeg *d_seg, const uint64_t *d_cum, uint32_t nseg, uint64_t total,
                        const uint8_t *d_src, uint8_t *d_dst, const int32_t *d_status, hipStream_t stream)
{
    if (nseg == 0 || (d_cum && total == 0))
        return 0;
    if (!d_seg || !d_src || !d_dst)
        return -1;
    uint32_t grid = kGatherGrid;
    if (d_cum) {
        grid = (uint32_t)std::min<uint64_t>((total + kTile - 1) / kTile, kGatherGrid);
        hipLaunchKernelGGL(range_gather_kernel, dim3(grid), dim3(kGatherT), 0, stream, d_seg, d_cum, nseg, d_src, d_dst,
                           d_status);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    // no prefix sum from the caller: one scan launch into pooled scratch
    static ScratchPool<GatherScratch> pool;
    GatherScratch *s = pool.acquire(stream);
    if (!s)
        return -1;
    int rc = 0;
    if (s->cap < (size_t)nseg + 1) {
        (void)hipFree(s->cum);
        s->cum = nullptr;
        s->cap = 0;
        const size_t want = std::max<size_t>((size_t)nseg + 1, 4096);
        if (hipMalloc((void **)&s->cum, want * sizeof(uint64_t)) == hipSuccess)
            s->cap = want;
        else
            rc = -1;
    }
    if (rc == 0) {
        hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(kScanT), 0, stream, d_seg, nseg, s->cum);
        hipLaunchKernelGGL(range_gather_kernel, dim3(grid), dim3(kGatherT), 0, stream, d_seg, s->cum, nseg, d_src, d_dst,
                           d_status);
        rc = hipGetLastError() == hipSuccess ? 0 : -1;
    }
    pool.release(s, stream);
    return rc;
}

}   // namespace zsk
