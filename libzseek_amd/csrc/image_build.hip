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
//
// The stream-ordered builds (build_image_pieces: zsk_lz4_build_image_pieces,
// zsk_zstd_build_image_pieces) queue the same batches on the caller's stream
// and wait for nothing: image_table_kernel leaves the answer in the caller's
// d_result.  With a piece list in device memory image_pieces_kernel takes
// image_cdesc_kernel's place: one workgroup that scans the batch's sizes on top
// of the running SOURCE offset, which joins the file offset in the chained
// state, and validates them (image_pieces.h; a sticky flag in that state turns
// the pieces after an invalid one into nothing).
//
// The appends (zsk_lz4_append_image_pieces, zsk_zstd_append_image_pieces) are
// a build from pieces behind a prologue, image_append.h holding the rules:
//   image_stash_kernel         copies the existing table's entries out of the
//                              image into the entries scratch and sums their
//                              compressed sizes
//   image_append_check_kernel  one workgroup: accepts the file or sets a sticky
//                              flag; on acceptance the running file offset
//                              starts at the old table's position
// The batches then number their frames from the old count on, and
// image_table_kernel writes the table over all frames -- or, when the call
// failed after the old table was overwritten, the old table back from the stash.
// Plain vector loads, stores and atomics only.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "block_scan.h"
#include "host.h"
#include "image_append.h"
#include "image_pieces.h"
#include "pool.h"
#include "zsk_internal.h"

namespace zsk {

namespace {

constexpr uint32_t kPlanT = 1024;
constexpr uint32_t kMaxFrames = 0x8000000u;   // ZSTD_SEEKABLE_MAXFRAMES (ref seek_table.c:17)
constexpr size_t kBatchSmall = 256u << 20;   // frames of <= 64 KiB (writer.cpp kGpuDeviceBatch)
constexpr size_t kBatchLinked = 1u << 30;    // linked frames: a launch costs one frame's chain
constexpr size_t kTableBytes = 65536;        // compressor scratch per frame
constexpr size_t kMaxBatchFrames = 65536;
constexpr size_t kStateWords = 7;            // the chained state (image_plan_kernel)

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

// The batch's descriptors of a build from device-listed pieces (image_pieces.h
// holds the rule): one workgroup, image_plan_kernel's shape.  A 64-bit
// exclusive scan of the batch's sizes on top of the running source offset
// (state[3]) gives piece i its offset; the first piece that is not valid there
// is found with it, and from that piece on (from 0 when an earlier batch set
// the flag) every piece is the refused one, which reads no source byte.  The
// offset stops at the first invalid piece and the flag stays set.  An append's
// refused file (kStateBadImage, kStateNoRoom) refuses every piece the same way.
__global__ __launch_bounds__(kPlanT) void image_pieces_kernel(const uint32_t *__restrict__ sizes, uint32_t n,
                                                              uint64_t max_piece, uint64_t src_len, uint64_t slot,
                                                              uint32_t flags, uint64_t *state,
                                                              zsk_compress_desc_t *__restrict__ desc)
{
    __shared__ uint64_t s_sum[kPlanT];
    __shared__ uint32_t s_bad;
    const uint32_t t = threadIdx.x;
    const uint64_t fl = state[1], base = state[3];
    const bool sticky = (fl & kStateDrop) != 0;
    if (t == 0)
        s_bad = sticky ? 0u : kNoBadPiece;
    uint32_t a, b;
    block_share<kPlanT>(n, t, &a, &b);
    uint64_t sum = 0;
    for (uint32_t i = a; i < b; i++)
        sum += sizes[i];
    // (the scan's first barrier also orders s_bad's start value and every
    // thread's reads of the state before the writes below)
    const uint64_t incl = block_scan_inclusive<kPlanT>(s_sum, t, sum);
    const uint64_t first = base + (incl - sum);
    // up to the list's first invalid piece the scanned offsets are the true
    // ones; what follows it is never used
    uint32_t bad = kNoBadPiece;
    uint64_t off = first, bad_off = 0;
    for (uint32_t i = a; i < b && bad == kNoBadPiece; i++) {
        if (!piece_valid(sizes[i], off, max_piece, src_len)) {
            bad = i;
            bad_off = off;
        }
        off = piece_advance(off, sizes[i]);
    }
    if (bad != kNoBadPiece)
        atomicMin(&s_bad, bad);
    __syncthreads();
    const uint32_t first_bad = s_bad;
    off = first;
    for (uint32_t i = a; i < b; i++) {
        const PieceSpan p = piece_span(i, sizes[i], off, first_bad);
        zsk_compress_desc_t o;
        o.src_off = p.src_off;
        o.dst_off = (uint64_t)i * slot;
        o.src_size = p.size;
        o.flags = flags;
        desc[i] = o;
        off = piece_advance(off, sizes[i]);
    }
    if (sticky)
        return;
    if (first_bad == kNoBadPiece) {
        if (t == kPlanT - 1)
            state[3] = base + incl;
    } else if (bad == first_bad) {   // (one thread: shares are disjoint)
        state[3] = bad_off;
        state[1] = fl | kStateBadPieces;
    }
}

// state[0]: the running file offset; state[1]: kStateRefused, some frame was
// refused (c_size 0), and kStateBadPieces (image_pieces_kernel), kStateBadImage
// and kStateNoRoom (image_append_check_kernel), under which every frame packs
// as nothing and the offset stays; state[2]: the file's size
// (image_table_kernel); state[3]: the running source offset of a build from
// pieces; of an append, state[4]: the sum of the old entries' compressed sizes
// (image_stash_kernel), state[5]: the old table's offset and state[6]: its
// descriptor byte, for the restore.
__global__ __launch_bounds__(kPlanT) void image_plan_kernel(const uint32_t *__restrict__ csize,
                                                            const zsk_compress_desc_t *__restrict__ cdesc,
                                                            const uint32_t *__restrict__ sums, uint32_t n,
                                                            uint64_t frame0, uint32_t ew, uint64_t *state,
                                                            GatherSeg *__restrict__ seg, uint64_t *__restrict__ cum,
                                                            uint32_t *__restrict__ entries)
{
    __shared__ uint64_t s_sum[kPlanT];
    const uint32_t t = threadIdx.x;
    const uint64_t base = state[0], fl = state[1];
    const bool drop = (fl & kStateDrop) != 0;
    uint32_t a, b;
    block_share<kPlanT>(n, t, &a, &b);
    uint64_t sum = 0;
    bool refused = false;
    for (uint32_t i = a; i < b; i++) {
        const uint32_t c = drop ? 0u : csize[i];
        sum += c;
        refused |= c == 0 && !drop;
    }
    // (range_gather.hip's scan, block_scan.h; its first barrier also orders
    // every thread's read of state[0] before the write below)
    const uint64_t incl = block_scan_inclusive<kPlanT>(s_sum, t, sum);
    uint64_t run = incl - sum;
    if (t == 0)
        cum[0] = 0;
    for (uint32_t i = a; i < b; i++) {
        const zsk_compress_desc_t d = cdesc[i];
        const uint32_t c = drop ? 0u : csize[i];
        GatherSeg g;
        g.src_off = d.dst_off;
        g.dst_off = base + run;
        g.len = c;
        g.frame = i;
        seg[i] = g;
        run += c;
        cum[i + 1] = run;
        uint32_t *e = entries + (frame0 + i) * ew;
        e[0] = c;
        e[1] = d.src_size;
        if (ew == 3)
            e[2] = sums[i];
    }
    if (refused)
        state[1] = fl | kStateRefused;
    if (t == kPlanT - 1)
        state[0] = base + incl;
}

// An append's stash: the existing table's entries, prev_frames x ew words at
// any byte alignment in the image, into entries[0, prev_frames * ew), and the
// sum of their cSize words into state[4] (a workgroup's partial sums meet in
// LDS; one atomic per workgroup).  The size comes from @prev in device memory,
// so every workgroup applies the window itself before it forms an address: a
// file outside it is not read at all, and image_append_check_kernel refuses it.
// @prev may be the call's own result words: nothing writes those before the
// table kernel.
__global__ __launch_bounds__(256) void image_stash_kernel(const uint8_t *__restrict__ image, uint64_t capacity,
                                                          const int64_t *prev, uint32_t prev_frames, uint32_t ew,
                                                          uint32_t *__restrict__ entries, uint64_t *state)
{
    __shared__ uint64_t s_sum[256];
    const int64_t size = prev[0];
    if (!append_window(size, capacity, prev_frames, ew == 3))
        return;
    const uint8_t *const tab = image + append_table_at(size, prev_frames, ew == 3) + kTableHeader;
    const bool words_aligned = (reinterpret_cast<uintptr_t>(tab) & 3) == 0;
    const uint64_t words = (uint64_t)prev_frames * ew;   // (< 2^29)
    uint64_t sum = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < words; j += (uint64_t)gridDim.x * 256) {
        uint32_t w;
        if (words_aligned)
            w = reinterpret_cast<const uint32_t *>(tab)[j];
        else
            w = append_le32(tab + 4 * j);
        entries[j] = w;
        if ((uint32_t)j % ew == 0)
            sum += w;
    }
    const uint64_t total = block_scan_inclusive<256>(s_sum, threadIdx.x, sum);
    if (threadIdx.x == 255 && total != 0)
        atomicAdd(reinterpret_cast<unsigned long long *>(state + 4), (unsigned long long)total);
}

// An append's check, one workgroup behind the stash: the rule of
// image_append.h on d_prev, the table's 17 header and footer bytes, the stash's
// sum and the file's first word.  An accepted file with room starts the running
// file offset at its table (kept in state[5], with the descriptor byte in
// state[6], for the restore); anything else sets its sticky flag and the call
// writes nothing to the image.
__global__ __launch_bounds__(64) void image_append_check_kernel(const uint8_t *__restrict__ image, uint64_t capacity,
                                                                const int64_t *prev, uint32_t prev_frames,
                                                                uint32_t checksums, uint32_t zstd, uint64_t src_len,
                                                                uint64_t npieces, uint64_t *state)
{
    __shared__ uint8_t s_b[kTableEnds + 4];
    const uint32_t t = threadIdx.x;
    const int64_t size = prev[0], count = prev[1];
    const bool ck = checksums != 0;
    const bool window = append_window(size, capacity, prev_frames, ck);
    if (t < kTableEnds + 4) {
        uint8_t b = 0;
        if (window) {
            // (inside the window: the table is the file's last bytes, and a
            // file with a frame in its table is longer than 4 bytes)
            if (t < kTableHeader)
                b = image[append_table_at(size, prev_frames, ck) + t];
            else if (t < kTableEnds)
                b = image[(uint64_t)size - kTableEnds + t];
            else if (prev_frames > 0)
                b = image[t - kTableEnds];
        }
        s_b[t] = b;
    }
    __syncthreads();
    if (t != 0)
        return;
    uint8_t ends[kTableEnds];
    for (uint32_t i = 0; i < kTableEnds; i++)
        ends[i] = s_b[i];
    const uint64_t verdict = append_verdict(size, count, capacity, prev_frames, ck, zstd != 0, ends, state[4],
                                            append_le32(s_b + kTableEnds), src_len, npieces);
    if (verdict) {
        state[1] = verdict;
    } else {
        const uint64_t at = append_table_at(size, prev_frames, ck);
        state[0] = at;
        state[5] = at;
        state[6] = ends[kTableHeader + 4];
    }
}

// The seek table at state[0] (ref seek_table.c:365-419): skippable header,
// frames x {cSize, dSize[, checksum]}, the frame count, the descriptor byte,
// the magic -- each thread one byte at a time.  With @result (the stream-ordered
// builds) the call's answer is written here too: the file's size or the
// failure, the frame count, and the source bytes consumed (state[3] for a
// build from pieces, else @consumed); an invalid piece list writes no table.
// @append (an append over @prev_frames old frames): a refused file writes
// nothing; an invalid piece list or a refused frame writes the old table, the
// stash's entries, back where it was.
__global__ __launch_bounds__(256) void image_table_kernel(uint8_t *__restrict__ image, uint64_t *state,
                                                          const uint32_t *__restrict__ entries, uint32_t frames,
                                                          uint32_t ew, int64_t *__restrict__ result, uint64_t consumed,
                                                          uint32_t pieces, uint32_t append, uint32_t prev_frames)
{
    const uint64_t fl = result ? state[1] : 0;
    const bool restore = append && (fl & (kStateBadPieces | kStateRefused)) != 0;
    const bool nothing = (fl & (kStateBadImage | kStateNoRoom)) != 0 || ((fl & kStateBadPieces) != 0 && !append);
    const uint32_t count = restore ? prev_frames : frames;
    const uint32_t desc = restore ? (uint32_t)state[6] : (ew == 3 ? 0x80u : 0u);
    const uint64_t at = restore ? state[5] : state[0];
    const uint64_t body = 4ull * ew * count, size = nothing ? 0 : 8 + body + 9;
    if (result && blockIdx.x == 0 && threadIdx.x == 0) {
        result[0] = (fl & kStateBadImage)    ? kImageBadImage
                    : (fl & kStateNoRoom)    ? kImageNoRoom
                    : (fl & kStateBadPieces) ? kImageBadPieces
                    : (fl & kStateRefused)   ? kImageFailed
                                             : (int64_t)(at + size);
        result[1] = frames;
        result[2] = (int64_t)(pieces ? state[3] : consumed);
    }
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
            w = x < 4 ? count : x == 4 ? desc : kSeekMagic;
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
    uint64_t *state = nullptr;     // device, kStateWords words
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

// One pool for the four builder entry points.
ScratchPool<ImageScratch> &image_pool()
{
    static ScratchPool<ImageScratch> pool;
    return pool;
}

// How a build is cut into batches and what its frames carry.
struct Layout {
    uint64_t frames, entry, slot;
    uint64_t first;   // an append: the frames the image already holds (else 0)
    uint32_t per, ew, cflags, tail_flags;
    bool in_frame, ck;
};

// What an append adds to a build from pieces (queue_image).
struct Append {
    const int64_t *d_prev;
    uint64_t capacity;
};

// @frame_size: the frame size, or the largest piece of a build from pieces.
Layout layout(const Codec &codec, uint64_t frames, size_t frame_size, unsigned flags, size_t batch_bytes)
{
    Layout L;
    L.frames = frames;
    L.first = 0;
    L.entry = (flags & ZSK_IMAGE_CHECKSUMS) ? 12 : 8;
    if (batch_bytes == 0)
        batch_bytes = !codec.zstd && frame_size > 65536 ? kBatchLinked : kBatchSmall;
    // frames per batch: batch_bytes of input, and the compressor's scratch
    // (64 KiB per frame) within batch_bytes too, as the writer's GPU mode
    const uint64_t cap_frames = std::min<uint64_t>(kMaxBatchFrames, std::max<uint64_t>(16, batch_bytes / kTableBytes));
    L.per = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, batch_bytes / frame_size),
                                         std::min<uint64_t>(cap_frames, std::max<uint64_t>(frames, 1)));
    L.slot = codec.bound(frame_size);
    L.ew = (uint32_t)(L.entry / 4);
    // zstd frames that end with their content checksum take the seek table's word
    L.in_frame = codec.zstd && (flags & ZSK_IMAGE_CONTENT_CHECKSUMS);
    L.ck = L.ew == 3 || L.in_frame;
    L.cflags = L.in_frame ? ZSK_COMPRESS_CONTENT_CHECKSUM : 0u;
    L.tail_flags = codec.zstd ? 0u : ZSK_COMPRESS_CONTENT_SIZE;
    return L;
}

// The set sized for the build (hipFree, when a buffer grows, waits for the device).
bool size_scratch(ImageScratch *s, const Codec &codec, const Layout &L)
{
    // per batch frame: cdesc (24), seg (24), cum (8, one more), csize, sums (4 + 4)
    const size_t per_frame = sizeof(zsk_compress_desc_t) + sizeof(GatherSeg) + 8 + 4 + 4;
    bool ok = grow(&s->slots, &s->slots_cap, L.frames ? L.per * L.slot : 0) &&
              grow(&s->tables, &s->tables_cap, L.frames ? codec.scratch(L.per) : 0) &&
              grow(&s->frames, &s->frames_cap, L.frames ? L.per * per_frame + 64 : 0) &&
              grow(&s->entries, &s->entries_cap, std::max<size_t>((L.first + L.frames) * L.entry, 16));
    if (ok && !s->state)
        ok = hipMalloc((void **)&s->state, kStateWords * sizeof(uint64_t)) == hipSuccess &&
             hipHostMalloc((void **)&s->h_state, 3 * sizeof(uint64_t), hipHostMallocDefault) == hipSuccess;
    if (!ok)
        (void)hipGetLastError();
    return ok;
}

// The whole build queued on @stream, no host wait: the state cleared, the
// batches, the table.  @d_sizes: the piece list (frame_size is then the largest
// piece), or NULL for frames of @frame_size.  @d_result: where the table kernel
// leaves the answer, or NULL (the synchronous builders read the state).
// @ap: an append to the file of L.first frames that @image holds, or NULL.
bool queue_image(const Codec &codec, const Layout &L, ImageScratch *s, const uint8_t *src, uint64_t len,
                 uint64_t frame_size, const uint32_t *d_sizes, int level, uint8_t *image, int64_t *d_result,
                 hipStream_t stream, const Append *ap = nullptr)
{
    const uint32_t per = L.per;
    // (8-byte members first: cum, cdesc, seg; then the words)
    uint64_t *const d_cum = reinterpret_cast<uint64_t *>(s->frames);
    zsk_compress_desc_t *const d_cdesc = reinterpret_cast<zsk_compress_desc_t *>(d_cum + per + 1);
    GatherSeg *const d_seg = reinterpret_cast<GatherSeg *>(d_cdesc + per);
    uint32_t *const d_csize = reinterpret_cast<uint32_t *>(d_seg + per);
    uint32_t *const d_sums = d_csize + per;
    uint32_t *const d_entries = reinterpret_cast<uint32_t *>(s->entries);

    bool ok = hipMemsetAsync(s->state, 0, kStateWords * sizeof(uint64_t), stream) == hipSuccess;
    if (ok && ap) {
        const uint64_t words = L.first * L.ew;
        if (words) {
            const uint32_t grid = (uint32_t)std::min<uint64_t>((words + 255) / 256, 2048);
            hipLaunchKernelGGL(image_stash_kernel, dim3(grid), dim3(256), 0, stream, image, ap->capacity, ap->d_prev,
                               (uint32_t)L.first, L.ew, d_entries, s->state);
        }
        hipLaunchKernelGGL(image_append_check_kernel, dim3(1), dim3(64), 0, stream, image, ap->capacity, ap->d_prev,
                           (uint32_t)L.first, L.ew == 3 ? 1u : 0u, codec.zstd ? 1u : 0u, len, L.frames, s->state);
        ok = hipGetLastError() == hipSuccess;
    }
    for (uint64_t f = 0; ok && f < L.frames; f += per) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(per, L.frames - f);
        if (d_sizes)
            hipLaunchKernelGGL(image_pieces_kernel, dim3(1), dim3(kPlanT), 0, stream, d_sizes + f, n, frame_size, len,
                               L.slot, L.cflags, s->state, d_cdesc);
        else
            hipLaunchKernelGGL(image_cdesc_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_cdesc, n,
                               f * frame_size, frame_size, len, L.slot, L.cflags, L.tail_flags);
        ok = hipGetLastError() == hipSuccess &&
             (!L.ck || launch_src_checksums(d_cdesc, n, src, d_sums, stream) == 0) &&
             (codec.zstd ? launch_zstd_compress(d_cdesc, n, src, s->slots, d_csize, s->tables, s->tables_cap,
                                                L.in_frame ? d_sums : nullptr, stream, codec.format)
                         : zsk_lz4_compress_frames(d_cdesc, n, src, s->slots, d_csize, level, s->tables, stream)) == 0;
        if (!ok)
            break;
        hipLaunchKernelGGL(image_plan_kernel, dim3(1), dim3(kPlanT), 0, stream, d_csize, d_cdesc, d_sums, n, L.first + f,
                           L.ew, s->state, d_seg, d_cum, d_entries);
        // (the gather reads the bytes' total from d_cum; the bound only sizes its grid)
        ok = hipGetLastError() == hipSuccess &&
             launch_range_gather(d_seg, d_cum, n, (uint64_t)n * L.slot, s->slots, image, nullptr, stream) == 0;
    }
    if (ok) {
        const uint64_t bytes = 8 + L.entry * (L.first + L.frames) + 9;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((bytes + 255) / 256, 2048);
        hipLaunchKernelGGL(image_table_kernel, dim3(grid), dim3(256), 0, stream, image, s->state, d_entries,
                           (uint32_t)(L.first + L.frames), L.ew, d_result, len, d_sizes ? 1u : 0u, ap ? 1u : 0u,
                           (uint32_t)L.first);
        ok = hipGetLastError() == hipSuccess;
    }
    return ok;
}

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
    const Layout L = layout(codec, g.frames, frame_size, flags, batch_bytes);

    DeviceGuard keep;
    hipStream_t stream = nullptr;
    if (hipSetDevice(dev) != hipSuccess || hip_stream_get(&stream, false) != hipSuccess) {
        (void)hipGetLastError();
        set_error(errbuf, "build image: create HIP stream failed");
        return -1;
    }
    ScratchPool<ImageScratch> &pool = image_pool();
    ImageScratch *s = pool.acquire(stream);
    if (!s) {
        hip_stream_put(stream);
        set_error(errbuf, "build image: scratch allocation failed");
        return -1;
    }
    if (!size_scratch(s, codec, L)) {
        pool.release(s, stream);
        hip_stream_put(stream);
        set_error(errbuf, "build image: scratch allocation failed");
        return -1;
    }
    const bool ok = queue_image(codec, L, s, static_cast<const uint8_t *>(d_src), len, frame_size, nullptr, level,
                                static_cast<uint8_t *>(d_image), nullptr, stream) &&
                    hipMemcpyAsync(s->h_state, s->state, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream) == hipSuccess;
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

// zsk_lz4_build_image_pieces / zsk_zstd_build_image_pieces: the same build
// queued on the caller's stream, the answer left in d_result by the table
// kernel.  Every refusal below comes before anything is queued.
int build_image_pieces(const Codec &codec, const void *d_src, size_t src_len, const uint32_t *d_sizes, size_t npieces,
                       size_t max_piece, int level, unsigned flags, size_t batch_bytes, void *d_image,
                       size_t capacity, int64_t *d_result, void *stream, char *errbuf)
{
    hipStream_t const q = static_cast<hipStream_t>(stream);
    if (refuse_capturing(q, "build image", errbuf))
        return -1;
    if (!d_result) {
        set_error(errbuf, "build image: NULL result");
        return -1;
    }
    if (max_piece == 0 || max_piece > codec.max_frame) {
        set_error(errbuf, "build image: invalid piece size");
        return -1;
    }
    if (level >= 3) {
        set_error(errbuf, "build image: HC levels are not supported");
        return -1;
    }
    if (npieces > kMaxFrames) {
        set_error(errbuf, "build image: Frame index is too large");
        return -1;
    }
    if (!d_sizes && npieces != src_len / max_piece + (src_len % max_piece ? 1 : 0)) {
        set_error(errbuf, "build image: invalid piece count");
        return -1;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        set_error(errbuf, "no HIP device available");
        return -1;
    }
    int dev = -1, other = -1;
    if (!device_pointer(d_image, &dev) || !device_pointer(d_result, &other) || other != dev ||
        (src_len && (!device_pointer(d_src, &other) || other != dev)) ||
        (d_sizes && (!device_pointer(d_sizes, &other) || other != dev))) {
        set_error(errbuf, "build image: not device memory of one device");
        return -1;
    }
    if ((reinterpret_cast<uintptr_t>(d_result) & 7) || (reinterpret_cast<uintptr_t>(d_sizes) & 3)) {
        set_error(errbuf, "build image: misaligned sizes or result");
        return -1;
    }
    const bool sums = (flags & ZSK_IMAGE_CHECKSUMS) != 0;
    if (capacity < (codec.zstd ? zstd_pieces_bound(src_len, npieces, sums) : lz4_pieces_bound(src_len, npieces, sums))) {
        set_error(errbuf, "build image: buffer too small");
        return -1;
    }
    const Layout L = layout(codec, npieces, max_piece, flags, batch_bytes);

    DeviceGuard keep;
    if (hipSetDevice(dev) != hipSuccess) {
        (void)hipGetLastError();
        set_error(errbuf, "build image: set HIP device failed");
        return -1;
    }
    ScratchPool<ImageScratch> &pool = image_pool();
    ImageScratch *s = pool.acquire(q);
    if (!s) {
        set_error(errbuf, "build image: scratch allocation failed");
        return -1;
    }
    if (!size_scratch(s, codec, L)) {
        pool.release(s, q);
        set_error(errbuf, "build image: scratch allocation failed");
        return -1;
    }
    // (an empty source has no byte to read: every listed piece is then invalid,
    // and the launchers only want a pointer that is not NULL)
    uint8_t *const image = static_cast<uint8_t *>(d_image);
    const uint8_t *const src = src_len ? static_cast<const uint8_t *>(d_src) : image;
    const bool ok = queue_image(codec, L, s, src, src_len, max_piece, d_sizes, level, image, d_result, q);
    if (!ok) {
        // all ones in the three words: ZSK_IMAGE_FAILED, behind whatever was queued
        (void)hipGetLastError();
        (void)hipMemsetAsync(d_result, 0xFF, 3 * sizeof(int64_t), q);
        (void)hipGetLastError();
        set_error(errbuf, "build image: GPU launch failed");
    }
    pool.release(s, q);
    return ok ? 0 : -1;
}

uint64_t append_bound(const Codec &codec, uint64_t prev_size, uint64_t prev_frames, uint64_t src_len, uint64_t npieces,
                      unsigned flags)
{
    const bool sums = (flags & ZSK_IMAGE_CHECKSUMS) != 0;
    return codec.zstd ? zstd_append_bound(prev_size, prev_frames, src_len, npieces, sums)
                      : lz4_append_bound(prev_size, prev_frames, src_len, npieces, sums);
}

// zsk_lz4_append_image_pieces / zsk_zstd_append_image_pieces: a build from
// pieces behind the file that @d_image holds, queued on the caller's stream.
// Every refusal below comes before anything is queued, and every argument
// check before the device is asked for.
int append_image_pieces(const Codec &codec, const void *d_src, size_t src_len, const uint32_t *d_sizes, size_t npieces,
                        size_t max_piece, int level, unsigned flags, size_t batch_bytes, void *d_image,
                        size_t capacity, const int64_t *d_prev, size_t prev_frames, int64_t *d_result, void *stream,
                        char *errbuf)
{
    hipStream_t const q = static_cast<hipStream_t>(stream);
    if (refuse_capturing(q, "append image", errbuf))
        return -1;
    if (!d_result) {
        set_error(errbuf, "append image: NULL result");
        return -1;
    }
    if (!d_prev) {
        set_error(errbuf, "append image: NULL prev");
        return -1;
    }
    if (!d_sizes) {
        set_error(errbuf, "append image: needs a piece list");
        return -1;
    }
    if (max_piece == 0 || max_piece > codec.max_frame) {
        set_error(errbuf, "append image: invalid piece size");
        return -1;
    }
    if (level >= 3) {
        set_error(errbuf, "append image: HC levels are not supported");
        return -1;
    }
    if (prev_frames > kMaxFrames || npieces > kMaxFrames - prev_frames) {
        set_error(errbuf, "append image: Frame index is too large");
        return -1;
    }
    if ((reinterpret_cast<uintptr_t>(d_result) & 7) || (reinterpret_cast<uintptr_t>(d_prev) & 7) ||
        (reinterpret_cast<uintptr_t>(d_sizes) & 3)) {
        set_error(errbuf, "append image: misaligned sizes, prev or result");
        return -1;
    }
    // the smallest file that could be there is its table alone
    const uint64_t least = pieces_table_bytes(prev_frames, (flags & ZSK_IMAGE_CHECKSUMS) != 0);
    if (capacity < append_bound(codec, least, prev_frames, src_len, npieces, flags)) {
        set_error(errbuf, "append image: buffer too small");
        return -1;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        set_error(errbuf, "no HIP device available");
        return -1;
    }
    int dev = -1, other = -1;
    if (!device_pointer(d_image, &dev) || !device_pointer(d_result, &other) || other != dev ||
        !device_pointer(d_prev, &other) || other != dev || !device_pointer(d_sizes, &other) || other != dev ||
        (src_len && (!device_pointer(d_src, &other) || other != dev))) {
        set_error(errbuf, "append image: not device memory of one device");
        return -1;
    }
    Layout L = layout(codec, npieces, max_piece, flags, batch_bytes);
    L.first = prev_frames;

    DeviceGuard keep;
    if (hipSetDevice(dev) != hipSuccess) {
        (void)hipGetLastError();
        set_error(errbuf, "append image: set HIP device failed");
        return -1;
    }
    ScratchPool<ImageScratch> &pool = image_pool();
    ImageScratch *s = pool.acquire(q);
    if (!s) {
        set_error(errbuf, "append image: scratch allocation failed");
        return -1;
    }
    if (!size_scratch(s, codec, L)) {
        pool.release(s, q);
        set_error(errbuf, "append image: scratch allocation failed");
        return -1;
    }
    uint8_t *const image = static_cast<uint8_t *>(d_image);
    const uint8_t *const src = src_len ? static_cast<const uint8_t *>(d_src) : image;
    const Append ap{d_prev, capacity};
    const bool ok = queue_image(codec, L, s, src, src_len, max_piece, d_sizes, level, image, d_result, q, &ap);
    if (!ok) {
        // (as build_image_pieces: ZSK_IMAGE_FAILED behind whatever was queued)
        (void)hipGetLastError();
        (void)hipMemsetAsync(d_result, 0xFF, 3 * sizeof(int64_t), q);
        (void)hipGetLastError();
        set_error(errbuf, "append image: GPU launch failed");
    }
    pool.release(s, q);
    return ok ? 0 : -1;
}

const Codec &zstd_codec(unsigned flags)
{
    // (the wide search implies the full format)
    return (flags & ZSK_IMAGE_ZSTD_WIDE) ? kZstdWide : (flags & ZSK_IMAGE_ZSTD_FULL) ? kZstdFull : kZstd;
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
    return build_image(zstd_codec(flags), d_src, len, frame_size, 0, flags, batch_bytes, d_image, capacity, errbuf);
}

extern "C" ZSEEK_EXPORT size_t zsk_lz4_pieces_bound(size_t src_len, size_t npieces, unsigned flags)
{
    return (size_t)lz4_pieces_bound(src_len, npieces, (flags & ZSK_IMAGE_CHECKSUMS) != 0);
}

extern "C" ZSEEK_EXPORT size_t zsk_zstd_pieces_bound(size_t src_len, size_t npieces, unsigned flags)
{
    return (size_t)zstd_pieces_bound(src_len, npieces, (flags & ZSK_IMAGE_CHECKSUMS) != 0);
}

extern "C" ZSEEK_EXPORT int zsk_lz4_build_image_pieces(const void *d_src, size_t src_len, const uint32_t *d_sizes,
                                                       size_t npieces, size_t max_piece, int level, unsigned flags,
                                                       size_t batch_bytes, void *d_image, size_t capacity,
                                                       int64_t *d_result, void *stream, char *errbuf)
{
    return build_image_pieces(kLz4, d_src, src_len, d_sizes, npieces, max_piece, level, flags, batch_bytes, d_image,
                              capacity, d_result, stream, errbuf);
}

extern "C" ZSEEK_EXPORT int zsk_zstd_build_image_pieces(const void *d_src, size_t src_len, const uint32_t *d_sizes,
                                                        size_t npieces, size_t max_piece, unsigned flags,
                                                        size_t batch_bytes, void *d_image, size_t capacity,
                                                        int64_t *d_result, void *stream, char *errbuf)
{
    return build_image_pieces(zstd_codec(flags), d_src, src_len, d_sizes, npieces, max_piece, 0, flags, batch_bytes,
                              d_image, capacity, d_result, stream, errbuf);
}

extern "C" ZSEEK_EXPORT size_t zsk_lz4_append_bound(size_t prev_size, size_t prev_frames, size_t src_len,
                                                    size_t npieces, unsigned flags)
{
    return (size_t)append_bound(kLz4, prev_size, prev_frames, src_len, npieces, flags);
}

extern "C" ZSEEK_EXPORT size_t zsk_zstd_append_bound(size_t prev_size, size_t prev_frames, size_t src_len,
                                                     size_t npieces, unsigned flags)
{
    return (size_t)append_bound(kZstd, prev_size, prev_frames, src_len, npieces, flags);
}

extern "C" ZSEEK_EXPORT int zsk_lz4_append_image_pieces(const void *d_src, size_t src_len, const uint32_t *d_sizes,
                                                        size_t npieces, size_t max_piece, int level, unsigned flags,
                                                        size_t batch_bytes, void *d_image, size_t capacity,
                                                        const int64_t *d_prev, size_t prev_frames, int64_t *d_result,
                                                        void *stream, char *errbuf)
{
    return append_image_pieces(kLz4, d_src, src_len, d_sizes, npieces, max_piece, level, flags, batch_bytes, d_image,
                               capacity, d_prev, prev_frames, d_result, stream, errbuf);
}

extern "C" ZSEEK_EXPORT int zsk_zstd_append_image_pieces(const void *d_src, size_t src_len, const uint32_t *d_sizes,
                                                         size_t npieces, size_t max_piece, unsigned flags,
                                                         size_t batch_bytes, void *d_image, size_t capacity,
                                                         const int64_t *d_prev, size_t prev_frames, int64_t *d_result,
                                                         void *stream, char *errbuf)
{
    return append_image_pieces(zstd_codec(flags), d_src, src_len, d_sizes, npieces, max_piece, 0, flags, batch_bytes,
                               d_image, capacity, d_prev, prev_frames, d_result, stream, errbuf);
}
