// image_build.hip — seekable files that live in device memory (gfx950): the
// glue kernels between the seek table and the decode / compress / gather
// kernels, and zsk_lz4_build_image / zsk_zstd_build_image (one builder over
// the codec: Codec below).
//
// Reading side (zsk_reader_open_device, reader.cpp): image_desc_kernel writes
// a contiguous batch's FrameDesc[n] from the reader's device-resident prefix
// sums, so such a batch uploads nothing.
//
// Writing side (build_image): per batch of frames, on one stream and
// with no host wait in between,
//   image_cdesc_kernel   the batch's compressor descriptors (frame i reads
//                        d_src at i * frame_size, writes slot i)
//   the codec's frame compressor, launch_src_checksums   (unchanged kernels;
//                        zstd frames that carry a content checksum take the
//                        word launch_src_checksums computed)
//   image_plan_kernel    one workgroup: a 64-bit exclusive scan of the batch's
//                        compressed sizes on top of the running file offset
//                        (device memory, so batches chain in stream order);
//                        one segment per frame, slot -> file offset; the
//                        frame's seek-table entry at its global index
//   range_gather_kernel  (unchanged) packs the slots into the image
// then image_table_kernel writes the seek table at the running offset, byte by
// byte (the image has any alignment), and the file's size and the failure
// flag come down in one 24-byte copy: the call's only synchronization.
// Plain vector loads and stores only.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "block_scan.h"
#include "host.h"
#include "pool.h"
#include "zsk_internal.h"

namespace zsk {

namespace {

constexpr uint32_t kPlanT = 1024;
constexpr uint32_t kMaxFrames = 0x8000000u;   // ZSTD_SEEKABLE_MAXFRAMES (ref seek_table.c:17)
constexpr uint32_t kSkippableMagic = 0x184D2A5Eu, kSeekMagic = 0x8F92EAB1u;
constexpr size_t kBatchSmall = 256u << 20;   // frames of <= 64 KiB (writer.cpp kGpuDeviceBatch)
constexpr size_t kBatchLinked = 1u << 30;    // linked frames: a launch costs one frame's chain
constexpr size_t kTableBytes = 65536;        // compressor scratch per frame
constexpr size_t kMaxBatchFrames = 65536;

__global__ __launch_bounds__(256) void image_desc_kernel(const uint64_t *__restrict__ coff,
                                                         const uint64_t *__restrict__ doff, uint64_t f0, uint32_t n,
                                                         uint64_t c_bias, FrameDesc *__restrict__ desc)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t c = coff[f0 + i], c1 = coff[f0 + i + 1];
    const uint64_t d = doff[f0 + i], d1 = doff[f0 + i + 1];
    FrameDesc o;
    o.c_off = c + c_bias;
    o.d_off = d - doff[f0];
    o.c_size = (uint32_t)(c1 - c);
    o.d_size = (uint32_t)(d1 - d);
    desc[i] = o;
}

// Frame i of the batch: input d_src[src0 + i * fs, + min(fs, len - ...)), slot
// i.  A piece shorter than fs is the file's last: the writer's buffered frame,
// whose header carries the content size.
__global__ __launch_bounds__(256) void image_cdesc_kernel(zsk_compress_desc_t *__restrict__ desc, uint32_t n,
                                                          uint64_t src0, uint64_t fs, uint64_t len, uint64_t slot,
                                                          uint32_t flags, uint32_t tail_flags)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t at = src0 + (uint64_t)i * fs;
    const uint64_t sz = len - at < fs ? len - at : fs;
    zsk_compress_desc_t o;
    o.src_off = at;
    o.dst_off = (uint64_t)i * slot;
    o.src_size = (uint32_t)sz;
    o.flags = flags | (sz < fs ? tail_flags : 0u);
    desc[i] = o;
}

// state[0]: the running file offset; state[1]: some frame was refused
// (c_size 0); state[2]: the file's size (image_table_kernel).
__global__ __launch_bounds__(kPlanT) void image_plan_kernel(const uint32_t *__restrict__ csize,
                                                            const zsk_compress_desc_t *__restrict__ cdesc,
                                                            const uint32_t *__restrict__ sums, uint32_t n,
                                                            uint64_t frame0, uint32_t ew, uint64_t *state,
                                                            GatherSeg *__restrict__ seg, uint64_t *__restrict__ cum,
                                                            uint32_t *__restrict__ entries)
{
    __shared__ uint64_t s_sum[kPlanT];
    const uint32_t t = threadIdx.x;
    const uint64_t base = state[0];
    uint32_t a, b;
    block_share<kPlanT>(n, t, &a, &b);
    uint64_t sum = 0;
    bool refused = false;
    for (uint32_t i = a; i < b; i++) {
        sum += csize[i];
        refused |= csize[i] == 0;
    }
    // (range_gather.hip's scan, block_scan.h; its first barrier also orders
    // every thread's read of state[0] before the write below)
    const uint64_t incl = block_scan_inclusive<kPlanT>(s_sum, t, sum);
    uint64_t run = incl - sum;
    if (t == 0)
        cum[0] = 0;
    for (uint32_t i = a; i < b; i++) {
        const zsk_compress_desc_t d = cdesc[i];
        GatherSeg g;
        g.src_off = d.dst_off;
        g.dst_off = base + run;
        g.len = csize[i];
        g.frame = i;
        seg[i] = g;
        run += csize[i];
        cum[i + 1] = run;
        uint32_t *e = entries + (frame0 + i) * ew;
        e[0] = csize[i];
        e[1] = d.src_size;
        if (ew == 3)
            e[2] = sums[i];
    }
    if (refused)
        state[1] = 1;
    if (t == kPlanT - 1)
        state[0] = base + incl;
}

// The seek table at state[0] (ref seek_table.c:365-419): skippable header,
// frames x {cSize, dSize[, checksum]}, the frame count, the descriptor byte,
// the magic -- each thread one byte at a time.
__global__ __launch_bounds__(256) void image_table_kernel(uint8_t *__restrict__ image, uint64_t *state,
                                                          const uint32_t *__restrict__ entries, uint32_t frames,
                                                          uint32_t ew)
{
    const uint64_t at = state[0];
    const uint64_t body = 4ull * ew * frames, size = 8 + body + 9;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < size; j += (uint64_t)gridDim.x * 256) {
        uint32_t w, k;
        if (j < 8) {
            w = j < 4 ? kSkippableMagic : (uint32_t)(size - 8);
            k = (uint32_t)j & 3;
        } else if (j < 8 + body) {
            w = entries[(j - 8) >> 2];
            k = (uint32_t)(j - 8) & 3;
        } else {
            const uint32_t x = (uint32_t)(j - 8 - body);
            w = x < 4 ? frames : x == 4 ? (ew == 3 ? 0x80u : 0u) : kSeekMagic;
            k = x < 4 ? x : x == 4 ? 0 : x - 5;
        }
        image[at + j] = (uint8_t)(w >> (8 * k));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        state[2] = at + size;
}

// Per-call scratch of zsk_lz4_build_image, pooled per device (pool.h).
struct ImageScratch {
    uint8_t *slots = nullptr;
    size_t slots_cap = 0;
    uint8_t *tables = nullptr;   // the compressor's scratch
    size_t tables_cap = 0;
    uint8_t *frames = nullptr;   // per batch frame: cdesc, seg, cum, csize, sums
    size_t frames_cap = 0;
    uint8_t *entries = nullptr;    // the whole file's seek-table entries (u32 words)
    size_t entries_cap = 0;
    uint64_t *state = nullptr;     // device, 3 words
    uint64_t *h_state = nullptr;   // pinned
};

bool grow(uint8_t **p, size_t *cap, size_t want)
{
    if (want <= *cap)
        return true;
    if (*p)
        (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    if (hipMalloc((void **)p, want) != hipSuccess)
        return false;
    *cap = want;
    return true;
}

// What the builder asks of a codec.
struct Codec {
    bool zstd;
    uint64_t max_frame;
    int format;   // zstd: ZSK_ZSTD_FORMAT_*
    uint64_t bound(uint64_t n) const { return zstd ? ZSK_ZSTD_COMPRESS_BOUND(n) : ZSK_LZ4_COMPRESS_BOUND(n); }
    size_t scratch(uint32_t nframes) const
    {
        return zstd ? zstd_compress_scratch_size(nframes, format) : zsk_lz4_compress_scratch_size(nframes);
    }
};
constexpr Codec kLz4{false, ZSK_LZ4_COMPRESS_MAX_FRAME, 0},
    kZstd{true, ZSK_ZSTD_COMPRESS_MAX_FRAME, ZSK_ZSTD_FORMAT_SUBSET},
    kZstdFull{true, ZSK_ZSTD_COMPRESS_MAX_FRAME, ZSK_ZSTD_FORMAT_FULL},
    kZstdWide{true, ZSK_ZSTD_COMPRESS_MAX_FRAME, ZSK_ZSTD_FORMAT_FULL_WIDE};

struct Geometry {
    uint64_t frames, full, tail, entry, bound;
};

bool geometry(const Codec &c, size_t len, size_t fs, unsigned flags, Geometry *g)
{
    if (fs == 0)
        return false;
    g->full = len / fs;
    g->tail = len % fs;
    g->frames = g->full + (g->tail ? 1 : 0);
    g->entry = (flags & ZSK_IMAGE_CHECKSUMS) ? 12 : 8;
    g->bound = g->full * c.bound(fs) + (g->tail ? c.bound(g->tail) : 0) + 8 +
               g->entry * g->frames + 9;
    return true;
}

bool device_pointer(const void *p, int *dev)
{
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return false;
    }
    *dev = a.device;
    return true;
}

}   // namespace

int launch_image_desc(const uint64_t *d_coff, const uint64_t *d_doff, uint64_t f0, uint32_t n, uint64_t c_bias,
                      FrameDesc *d_desc, hipStream_t stream)
{
    if (n == 0)
        return 0;
    if (!d_coff || !d_doff || !d_desc)
        return -1;
    hipLaunchKernelGGL(image_desc_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_coff, d_doff, f0, n, c_bias,
                       d_desc);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}   // namespace zsk

using namespace zsk;

namespace {

ssize_t build_image(const Codec &codec, const void *d_src, size_t len, size_t frame_size, int level, unsigned flags,
                    size_t batch_bytes, void *d_image, size_t capacity, char *errbuf)
{
    Geometry g;
    if (frame_size > codec.max_frame || !geometry(codec, len, frame_size, flags, &g)) {
        set_error(errbuf, "build image: invalid frame size");
        return -1;
    }
    if (level >= 3) {
        set_error(errbuf, "build image: HC levels are not supported");
        return -1;
    }
    if (g.frames > kMaxFrames) {
        set_error(errbuf, "build image: Frame index is too large");
        return -1;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        set_error(errbuf, "no HIP device available");
        return -1;
    }
    int dev = -1, src_dev = -1;
    if (!device_pointer(d_image, &dev) || (len && (!device_pointer(d_src, &src_dev) || src_dev != dev))) {
        set_error(errbuf, "build image: not device memory of one device");
        return -1;
    }
    if (capacity < g.bound) {
        set_error(errbuf, "build image: buffer too small");
        return -1;
    }
    if (batch_bytes == 0)
        batch_bytes = !codec.zstd && frame_size > 65536 ? kBatchLinked : kBatchSmall;
    // frames per batch: batch_bytes of input, and the compressor's scratch
    // (64 KiB per frame) within batch_bytes too, as the writer's GPU mode
    const uint64_t cap_frames = std::min<uint64_t>(kMaxBatchFrames, std::max<uint64_t>(16, batch_bytes / kTableBytes));
    const uint32_t per = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, batch_bytes / frame_size),
                                                      std::min<uint64_t>(cap_frames, std::max<uint64_t>(g.frames, 1)));
    const uint64_t slot = codec.bound(frame_size);
    const uint32_t ew = (uint32_t)(g.entry / 4);
    // zstd frames that end with their content checksum take the seek table's word
    const bool in_frame = codec.zstd && (flags & ZSK_IMAGE_CONTENT_CHECKSUMS);
    const bool ck = ew == 3 || in_frame;
    const uint32_t cflags = in_frame ? ZSK_COMPRESS_CONTENT_CHECKSUM : 0u;
    const uint32_t tail_flags = codec.zstd ? 0u : ZSK_COMPRESS_CONTENT_SIZE;

    DeviceGuard keep;
    hipStream_t stream = nullptr;
    if (hipSetDevice(dev) != hipSuccess || hip_stream_get(&stream, false) != hipSuccess) {
        (void)hipGetLastError();
        set_error(errbuf, "build image: create HIP stream failed");
        return -1;
    }
    static ScratchPool<ImageScratch> pool;
    ImageScratch *s = pool.acquire(stream);
    if (!s) {
        hip_stream_put(stream);
        set_error(errbuf, "build image: scratch allocation failed");
        return -1;
    }
    // per batch frame: cdesc (24), seg (24), cum (8, one more), csize, sums (4 + 4)
    const size_t per_frame = sizeof(zsk_compress_desc_t) + sizeof(GatherSeg) + 8 + 4 + 4;
    bool ok = grow(&s->slots, &s->slots_cap, g.frames ? per * slot : 0) &&
              grow(&s->tables, &s->tables_cap, g.frames ? codec.scratch(per) : 0) &&
              grow(&s->frames, &s->frames_cap, g.frames ? per * per_frame + 64 : 0) &&
              grow(&s->entries, &s->entries_cap, std::max<size_t>(g.frames * g.entry, 16));
    if (ok && !s->state)
        ok = hipMalloc((void **)&s->state, 3 * sizeof(uint64_t)) == hipSuccess &&
             hipHostMalloc((void **)&s->h_state, 3 * sizeof(uint64_t), hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        pool.release(s, stream);
        hip_stream_put(stream);
        set_error(errbuf, "build image: scratch allocation failed");
        return -1;
    }
    // (8-byte members first: cum, cdesc, seg; then the words)
    uint64_t *const d_cum = reinterpret_cast<uint64_t *>(s->frames);
    zsk_compress_desc_t *const d_cdesc = reinterpret_cast<zsk_compress_desc_t *>(d_cum + per + 1);
    GatherSeg *const d_seg = reinterpret_cast<GatherSeg *>(d_cdesc + per);
    uint32_t *const d_csize = reinterpret_cast<uint32_t *>(d_seg + per);
    uint32_t *const d_sums = d_csize + per;
    uint32_t *const d_entries = reinterpret_cast<uint32_t *>(s->entries);
    const uint8_t *const src = static_cast<const uint8_t *>(d_src);
    uint8_t *const image = static_cast<uint8_t *>(d_image);

    ok = hipMemsetAsync(s->state, 0, 3 * sizeof(uint64_t), stream) == hipSuccess;
    for (uint64_t f = 0; ok && f < g.frames; f += per) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(per, g.frames - f);
        hipLaunchKernelGGL(image_cdesc_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_cdesc, n,
                           f * (uint64_t)frame_size, (uint64_t)frame_size, (uint64_t)len, slot, cflags, tail_flags);
        ok = hipGetLastError() == hipSuccess && (!ck || launch_src_checksums(d_cdesc, n, src, d_sums, stream) == 0) &&
             (codec.zstd ? launch_zstd_compress(d_cdesc, n, src, s->slots, d_csize, s->tables, s->tables_cap,
                                                in_frame ? d_sums : nullptr, stream, codec.format)
                         : zsk_lz4_compress_frames(d_cdesc, n, src, s->slots, d_csize, level, s->tables, stream)) == 0;
        if (!ok)
            break;
        hipLaunchKernelGGL(image_plan_kernel, dim3(1), dim3(kPlanT), 0, stream, d_csize, d_cdesc, d_sums, n, f, ew,
                           s->state, d_seg, d_cum, d_entries);
        // (the gather reads the bytes' total from d_cum; the bound only sizes its grid)
        ok = hipGetLastError() == hipSuccess &&
             launch_range_gather(d_seg, d_cum, n, (uint64_t)n * slot, s->slots, image, nullptr, stream) == 0;
    }
    if (ok) {
        const uint64_t bytes = 8 + g.entry * g.frames + 9;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((bytes + 255) / 256, 2048);
        hipLaunchKernelGGL(image_table_kernel, dim3(grid), dim3(256), 0, stream, image, s->state, d_entries,
                           (uint32_t)g.frames, ew);
        ok = hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(s->h_state, s->state, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream) == hipSuccess;
    }
    // the call's one synchronization (also drains what a failed step queued)
    const hipError_t e = hipStreamSynchronize(stream);
    const uint64_t size = ok && e == hipSuccess ? s->h_state[2] : 0;
    const bool refused = ok && e == hipSuccess && s->h_state[1] != 0;
    pool.release(s, stream);
    hip_stream_put(stream);
    if (!ok || e != hipSuccess) {
        (void)hipGetLastError();
        set_error(errbuf, "build image: %s", e != hipSuccess ? hipGetErrorString(e) : "GPU launch failed");
        return -1;
    }
    if (refused) {
        set_error(errbuf, "build image: GPU compression failed");
        return -1;
    }
    return (ssize_t)size;
}

}   // namespace

extern "C" ZSEEK_EXPORT size_t zsk_lz4_image_bound(size_t len, size_t frame_size, unsigned flags)
{
    Geometry g;
    return geometry(kLz4, len, frame_size, flags, &g) ? (size_t)g.bound : 0;
}

extern "C" ZSEEK_EXPORT ssize_t zsk_lz4_build_image(const void *d_src, size_t len, size_t frame_size, int level,
                                                    unsigned flags, size_t batch_bytes, void *d_image,
                                                    size_t capacity, char *errbuf)
{
    return build_image(kLz4, d_src, len, frame_size, level, flags, batch_bytes, d_image, capacity, errbuf);
}

extern "C" ZSEEK_EXPORT size_t zsk_zstd_image_bound(size_t len, size_t frame_size, unsigned flags)
{
    Geometry g;
    return geometry(kZstd, len, frame_size, flags, &g) ? (size_t)g.bound : 0;
}

extern "C" ZSEEK_EXPORT ssize_t zsk_zstd_build_image(const void *d_src, size_t len, size_t frame_size, unsigned flags,
                                                     size_t batch_bytes, void *d_image, size_t capacity, char *errbuf)
{
    // (the wide search implies the full format)
    const Codec &codec = (flags & ZSK_IMAGE_ZSTD_WIDE) ? kZstdWide : (flags & ZSK_IMAGE_ZSTD_FULL) ? kZstdFull : kZstd;
    return build_image(codec, d_src, len, frame_size, 0, flags, batch_bytes, d_image, capacity, errbuf);
}
