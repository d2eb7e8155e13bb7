// frame_check.hip — seek-table frame checksums verified and computed on the
// GPU (gfx950).
//
// The seekable format's per-frame checksum (descriptor bit 7) is the low 32
// bits of XXH64(seed 0) of the frame's decompressed bytes; the reference
// parses it (src/seek_table.c:95-97, seekEntry_t.checksum :36-40; writer
// :392-396) and never checks it.  Here it is checked over the decoded frames
// already in HBM, after the decode grid, on the same stream.
//
// Mapping: four lanes per frame, one per XXH64 accumulator (16 frames per
// wave).  Lane k of a frame reads 8-byte word k of each 32-byte stripe, so a
// frame's four lanes together read consecutive 32-byte stripes and each line
// they touch is consumed whole over four consecutive stripes; four stripes'
// loads are issued before the dependent rounds.  The tail (< 32 bytes) and
// the avalanche run on the frame's lane 0, serially, as XXH64 defines them.
// Algorithmic bytes per frame: d_size read once.
//
// The writer needs the same hash the other way round: the checksum of each
// frame it compresses, stored instead of compared (zsk_frame_checksums, and
// launch_src_checksums over the compressor's descriptors).  Both kernels call
// one frame_xxh64 body.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/zseek_hip.h"
#include "xxh64_dev.h"
#include "zsk_internal.h"

namespace zsk {

namespace {

using namespace xxh64d;

typedef uint64_t u64_ua __attribute__((aligned(1)));
typedef uint32_t u32_ua __attribute__((aligned(1)));

__device__ __forceinline__ uint64_t ld8(const uint8_t *p)
{
    return *reinterpret_cast<const u64_ua *>(p);
}

// XXH64(seed 0) of p[0, len), low 32 bits, by the frame's four lanes (k =
// 0..3, consecutive lanes of one wave; every lane of the wave calls this, a
// lane with on == false passes len 0 and reads nothing).  The frame's lane 0
// hands the result to sink(h32); the other lanes return without one.  The one
// XXH64 body: the verify and compute kernels differ only in their sink.
template <typename Sink>
__device__ __forceinline__ void frame_xxh64(const uint8_t *p, uint32_t len, bool on, uint32_t k, Sink sink)
{
    const uint32_t stripes = len / 32;
    uint64_t acc = k == 0 ? P64_1 + P64_2 : k == 1 ? P64_2 : k == 2 ? 0 : 0ull - P64_1;
    const uint8_t *q = p + 8 * k;
    uint32_t s = 0;
    for (; s + 4 <= stripes; s += 4) {
        const uint64_t v0 = ld8(q + 32 * s), v1 = ld8(q + 32 * s + 32);
        const uint64_t v2 = ld8(q + 32 * s + 64), v3 = ld8(q + 32 * s + 96);
        acc = xround(acc, v0);
        acc = xround(acc, v1);
        acc = xround(acc, v2);
        acc = xround(acc, v3);
    }
    for (; s < stripes; s++)
        acc = xround(acc, ld8(q + 32 * s));
    // accumulators 1..3 of this frame to its lane 0 (every lane shuffles)
    const int base = (int)(threadIdx.x & 60u);
    const uint64_t a1 = __shfl(acc, base + 1, 64), a2 = __shfl(acc, base + 2, 64),
                   a3 = __shfl(acc, base + 3, 64);
    if (!on || k != 0)
        return;
    uint64_t h;
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
    uint32_t i = stripes * 32;
    for (; i + 8 <= len; i += 8) {
        h ^= xround(0, ld8(p + i));
        h = rotl64(h, 27) * P64_1 + P64_4;
    }
    if (i + 4 <= len) {
        h ^= (uint64_t)*reinterpret_cast<const u32_ua *>(p + i) * P64_1;
        h = rotl64(h, 23) * P64_2 + P64_3;
        i += 4;
    }
    for (; i < len; i++) {
        h ^= p[i] * P64_5;
        h = rotl64(h, 11) * P64_1;
    }
    sink((uint32_t)xavalanche(h));
}

__global__ __launch_bounds__(256) void frame_xxh64_kernel(const FrameDesc *__restrict__ desc, uint32_t n,
                                                          const uint8_t *__restrict__ out,
                                                          const uint32_t *__restrict__ want,
                                                          int32_t *__restrict__ status)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t f = t >> 2, k = t & 3;
    // the four lanes of a frame agree on `on`: they read the same status
    const bool on = f < n && status[f] == ST_OK;
    uint32_t len = 0;
    const uint8_t *p = out;
    if (on) {
        const FrameDesc d = desc[f];
        len = d.d_size;
        p = out + d.d_off;
    }
    frame_xxh64(p, len, on, k, [&](uint32_t h) {
        if (h != want[f])
            status[f] = ST_SEEK_CHECKSUM;
    });
}

// The compute form: sums[f] = the checksum of data[off_f, off_f + size_f),
// the u64 offset and u32 size of frame f read at `stride` bytes per frame from
// off0 / size0 (zsk_frame_desc_t's d_off / d_size, or zsk_compress_desc_t's
// src_off / src_size: no descriptors are repacked for it).
__global__ __launch_bounds__(256) void frame_xxh64_store_kernel(const uint8_t *__restrict__ off0,
                                                                const uint8_t *__restrict__ size0, uint32_t stride,
                                                                uint32_t n, const uint8_t *__restrict__ data,
                                                                uint32_t *__restrict__ sums)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t f = t >> 2, k = t & 3;
    const bool on = f < n;
    uint32_t len = 0;
    const uint8_t *p = data;
    if (on) {
        len = *reinterpret_cast<const uint32_t *>(size0 + (size_t)f * stride);
        p = data + *reinterpret_cast<const uint64_t *>(off0 + (size_t)f * stride);
    }
    frame_xxh64(p, len, on, k, [&](uint32_t h) { sums[f] = h; });
}

int launch_store(const uint8_t *off0, const uint8_t *size0, uint32_t stride, uint32_t nframes, const uint8_t *d_data,
                 uint32_t *d_sums, hipStream_t stream)
{
    if (!d_sums)
        return -1;
    const uint32_t blocks = (uint32_t)(((uint64_t)nframes * 4 + 255) / 256);
    hipLaunchKernelGGL(frame_xxh64_store_kernel, dim3(blocks), dim3(256), 0, stream, off0, size0, stride, nframes,
                       d_data, d_sums);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}   // namespace

int launch_frame_checksums(const FrameDesc *d_desc, uint32_t nframes, const uint8_t *d_out,
                           const uint32_t *d_want, int32_t *d_status, hipStream_t stream)
{
    if (nframes == 0)
        return 0;
    const uint32_t blocks = (uint32_t)(((uint64_t)nframes * 4 + 255) / 256);
    hipLaunchKernelGGL(frame_xxh64_kernel, dim3(blocks), dim3(256), 0, stream, d_desc, nframes, d_out,
                       d_want, d_status);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_frame_checksums_compute(const FrameDesc *d_desc, uint32_t nframes, const uint8_t *d_data,
                                   uint32_t *d_sums, hipStream_t stream)
{
    if (nframes == 0)
        return 0;
    if (!d_desc)
        return -1;
    const uint8_t *b = reinterpret_cast<const uint8_t *>(d_desc);
    return launch_store(b + offsetof(FrameDesc, d_off), b + offsetof(FrameDesc, d_size), sizeof(FrameDesc), nframes,
                        d_data, d_sums, stream);
}

int launch_src_checksums(const zsk_compress_desc_t *d_desc, uint32_t nframes, const uint8_t *d_src,
                         uint32_t *d_sums, hipStream_t stream)
{
    if (nframes == 0)
        return 0;
    if (!d_desc)
        return -1;
    const uint8_t *b = reinterpret_cast<const uint8_t *>(d_desc);
    return launch_store(b + offsetof(zsk_compress_desc_t, src_off), b + offsetof(zsk_compress_desc_t, src_size),
                        sizeof(zsk_compress_desc_t), nframes, d_src, d_sums, stream);
}

}   // namespace zsk

extern "C" ZSEEK_EXPORT int zsk_frame_checksums(const zsk_frame_desc_t *d_desc, uint32_t nframes, const void *d_data,
                                                uint32_t *d_checksums, void *stream)
{
    return zsk::launch_frame_checksums_compute(reinterpret_cast<const zsk::FrameDesc *>(d_desc), nframes,
                                               static_cast<const uint8_t *>(d_data), d_checksums,
                                               static_cast<hipStream_t>(stream));
}

extern "C" ZSEEK_EXPORT int zsk_verify_frame_checksums(const zsk_frame_desc_t *d_desc, uint32_t nframes,
                                                       const void *d_out, const uint32_t *d_checksums,
                                                       int32_t *d_status, void *stream)
{
    return zsk::launch_frame_checksums(reinterpret_cast<const zsk::FrameDesc *>(d_desc), nframes,
                                       static_cast<const uint8_t *>(d_out), d_checksums, d_status,
                                       static_cast<hipStream_t>(stream));
}
