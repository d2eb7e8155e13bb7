// reader_internal.h — what reader.cpp (open / close, the contiguous pipeline,
// stats, setters) and reader_vec.cpp (the vectored reads) share.
#ifndef ZSK_READER_INTERNAL_H
#define ZSK_READER_INTERNAL_H

#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>

#include "../../include/zseek_hip.h"
#include "batch_layout.h"
#include "host.h"

// A seekable file in device memory (zsk_reader_open_device): the frames are
// decoded where they are.  The decode kernels get `base`, the image's start
// rounded down to 256 bytes (the alignment of the hipMalloc'd staging they
// otherwise read: the zstd kernels align their spans by c_off alone, so the base
// itself must be 16-byte aligned), and descriptors whose c_off carry `bias`.
struct DeviceImage {
    const uint8_t *ptr = nullptr;    // the caller's image (not owned)
    size_t size = 0;
    int device = -1;
    const uint8_t *base = nullptr;   // ptr rounded down to 256
    uint64_t bias = 0;               // ptr - base
    // the seek table, uploaded at open: c_off[n + 1], d_off[n + 1], then the
    // n checksums when the file carries them
    uint64_t *d_table = nullptr;
    size_t table_bytes = 0;
    const uint64_t *d_coff = nullptr, *d_doff = nullptr;
    const uint32_t *d_ck = nullptr;
    // the file's largest frame, decoded and compressed: what a device-planned
    // read (zsk_preadv_device_indirect) sizes its staging and its parse scratch by
    uint32_t max_dsize = 0, max_csize = 0;
    // zsk_reader_zstd_census' result, stored under the reader's exclusive lock
    // and published by has_census (read before the lock is taken): what a
    // device-planned read of a zstd image sizes its zstd scratch by
    zsk_zstd_census_t census = {};
    std::atomic<bool> has_census{false};
};

struct zseek_reader {
    zseek_read_file_t user_file;
    DeviceImage *img = nullptr;   // NULL: the file comes through user_file
    zseek_compression_type_t type;
    // the reference's rwlock (decompress.c:38): shared for cache hits
    // (:699-706), exclusive for misses, no-cache reads and GPU batches
    // (:714-720); lru_lock orders the MRU promotion of concurrent hits (the
    // reference promotes under its read lock, cache.c:125)
    std::shared_mutex lock;
    std::mutex lru_lock;
    // zseek_reader_stats' changing fields, published under the exclusive
    // lock after every change, read without the reader lock: a stats call
    // never waits behind a multi-GiB GPU read (the reference takes its read
    // lock, :850-875, and waits at most one frame decode)
    std::atomic<size_t> snap_cache_memory{0}, snap_cached_frames{0}, snap_buffered{0};
    std::mutex io_lock;   // one user pread callback at a time (lanes run in threads)
    zsk::SeekTable st;
    zsk::FrameCache *cache = nullptr;   // NULL when cache_size == 0 (ref :219-227)
    std::mutex cursor_lock;             // zseek_read: cursor read, pread, advance as one step
    size_t pos = 0;                     // zseek_read cursor (ref :826-835)
    size_t batch_bytes = 64u << 20;     // decoded bytes per batch
    int io_threads = 1;    // > 1: the caller allows concurrent pread callbacks
    bool verify = false;   // check seek-table frame checksums (the reference never does)
    // zsk_reader_set_zstd_async: 0 = zsk_preadv_device_async refuses a zstd
    // reader; >= 3: it decodes each batch with zstd_decode_frames_async, its
    // sequence bound the batch's decoded bytes / zstd_async
    unsigned zstd_async = 0;
    std::vector<int> devices;                            // lane i decodes on devices[i]
    std::vector<std::unique_ptr<zsk::DeviceCtx>> lanes;  // created at first use
};

namespace zsk {

static_assert(sizeof(FrameDesc) == kDescBytes && sizeof(GatherSeg) == kSegBytes, "batch_layout.h's sizes");

struct CacheItem {
    size_t frame;
    uint8_t *data;   // malloc'd, owned until inserted
    size_t len;
};

// One lane's share of a request: frames [fa, fb); bytes [offset, end) of the
// decoded range go to buf at (x - offset).
struct LaneJob {
    zseek_reader *r = nullptr;
    DeviceCtx *g = nullptr;
    size_t fa = 0, fb = 0;
    uint64_t offset = 0, end = 0;
    uint8_t *buf = nullptr;
    bool device_dst = false;
    int dst_dev = -1;
    void *call_data = nullptr;
    size_t cache_cap = 0;   // keep the last cache_cap good frames' bytes
    // results
    bool io_failed = false;   // pread / HIP failure (err holds the text)
    char err[ZSEEK_ERRBUF_SIZE] = {0};
    size_t first_bad = SIZE_MAX;   // first failed frame, if any
    int32_t status = ST_OK;
    uint32_t fail_at = 0;
    uint64_t good_end = 0;   // the lane's bytes before good_end are in buf
    std::deque<CacheItem> cached;
};

void frame_error(zseek_reader *r, bool cached, int32_t st, uint32_t fail_at, size_t frame, size_t offset_in_frame,
                 size_t count, char *errbuf);
bool read_span(LaneJob &J, uint8_t *dst, uint64_t len, uint64_t off);
bool image_span(LaneJob &J, const DeviceImage *img, uint64_t len, uint64_t off);
bool ensure_lanes(zseek_reader *r, char *errbuf);
void publish_stats(zseek_reader *r);

// The stats snapshot once a request is done: declared under the exclusive lock.
struct PublishStats {
    zseek_reader *r;
    ~PublishStats() { publish_stats(r); }
};

// Queue the decode of one batch -- n frames by the descriptors d_desc, read
// from comp, into s.d_out (or `out`), their statuses and fail_at words into s.d_status --
// on stream q: the wave engine's presets, the decode, the checksum pass.
struct DecodeBatch {
    zseek_compression_type_t type;
    hipStream_t q;
    const FrameDesc *d_desc;
    uint32_t n;
    const uint8_t *comp;
    uint32_t max_dsize;                  // the largest frame's decoded size (or a bound)
    uint32_t stop_last = 0xFFFFFFFFu;    // the last frame executed only so far
    // zstd, a few frames planned on the host: the plan and its device copy
    const ZstdHostPlan *zplan = nullptr;
    const uint64_t *d_plan = nullptr;
    // zstd, the stream-ordered form (zstd_decode_frames_async) by these bounds
    const ZstdBounds *zasync = nullptr;
    // LZ4 split engine: the host's descriptors, by which the scratch is
    // reserved here (NULL: the caller has reserved it); laid out in order in
    // comp, or scattered (the plan's scan layout); the one-frame route's post
    const FrameDesc *h_desc = nullptr;
    bool in_order = true;
    const HostPost *post = nullptr;
    bool *posted = nullptr;
    // the checksum pass: the batch's seek-table words (NULL: no pass; s.d_ck:
    // uploaded here from s.h_ck, behind the decode)
    const uint32_t *d_want = nullptr;
    // where the descriptors' d_off count from (NULL: the slot's d_out): the
    // decode launchers' and the checksum pass' output base
    uint8_t *out = nullptr;
};
inline bool lz4_wave_batch(zseek_compression_type_t type, size_t n)   // the batch takes the wave engine
{
    return type == ZSEEK_LZ4 && lz4_pick_engine((uint32_t)n) == ENGINE_WAVE;
}
// hipErrorOutOfMemory: the scratch reserve failed; hipErrorLaunchFailure: a launch
hipError_t decode_batch(Slot &s, const DecodeBatch &a);

enum Queued { kNoneLeft, kQueued, kQueueFailed };

// Up to kSlots batches in flight on g's slots, taken in turn and finished in
// order: submit(slot, k) queues the k-th batch, finish(slot, k) waits for it
// and returns false when it failed.  After a failure of either nothing more
// is submitted and the batches still in flight are drained, nothing of them
// kept.  Returns once the slots' host copies are done.
template <class Submit, class Finish> void run_in_flight(DeviceCtx &g, Submit submit, Finish finish)
{
    size_t queued = 0, finished = 0;
    bool more = true, stop = false;
    for (;;) {
        if (more && queued - finished < (size_t)kSlots) {
            const Queued q = submit(g.slot[queued % kSlots], queued);
            if (q == kQueued)
                queued++;
            else
                more = false, stop = q == kQueueFailed;
            continue;
        }
        if (finished == queued)
            break;
        Slot &s = g.slot[finished % kSlots];
        const size_t k = finished++;
        if (stop)
            (void)hipEventSynchronize(s.done);
        else if (!finish(s, k))
            more = false, stop = true;
    }
    for (Slot &s : g.slot)
        pool_wait(&s.copies);
}

}   // namespace zsk

#endif
