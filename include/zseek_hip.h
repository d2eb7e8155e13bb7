/*
 * zseek_hip.h — GPU extensions of the MI355X-native libzseek (C ABI).
 *
 * Plain pointers and sizes only (no HIP or torch types): device pointers are
 * hipMalloc'd (or torch-allocated) memory on the reader's device, and a
 * stream is a hipStream_t passed as void* (NULL = the library's own stream).
 *
 * Reference interfaces these replace / extend:
 *   zsk_lz4_decode_frames  — the per-frame LZ4F_decompress loop of
 *                            /root/reference/src/decompress.c:752-773 (and
 *                            :627-664 for the no-cache variant), batched over
 *                            every frame of a request in one grid.
 *   zsk_zstd_decode_frames — ZSTD_decompressDCtx (decompress.c:537) /
 *                            ZSTD_decompressStream (:414-454), batched the
 *                            same way.
 *   zsk_zstd_decode_frames_async — the same decode without its host wait:
 *                            scratch sized from bounds the caller states
 *                            (zsk_zstd_bounds_default: a policy), the plan
 *                            checked against them on the device.
 *   zsk_reader_frames      — the seek-table accessors frame_offset_c/d and
 *                            frame_size_c/d, seek_table.c:204-226.
 *   zsk_pread_device       — zseek_pread (decompress.c:806-824) with the
 *                            decoded bytes left in device memory.
 *   zsk_preadv, zsk_preadv_device — a caller's loop of zseek_pread calls over
 *                            scattered ranges (the reference has no vectored
 *                            read), as one call: the touched frames decoded
 *                            in one grid per batch; zsk_gather_segments is
 *                            its device-side segmented copy.
 *   zsk_preadv_device_async — the same read queued on the caller's stream,
 *                            its per-range results left in device memory
 *                            (a zstd reader: after zsk_reader_set_zstd_async).
 *   zsk_preadv_device_indirect — ... with the range list in device memory
 *                            too, planned by kernels from the seek table a
 *                            device-image reader keeps resident (a zstd
 *                            reader: after zsk_reader_zstd_census).
 *   zsk_read_frames_indirect — a caller's loop of zseek_pread calls over
 *                            whole frames picked by index, the indices in
 *                            device memory, each frame decoded in place into
 *                            a packed or padded-rows batch.
 *   zsk_reader_zstd_census — no reference function: the largest scratch need
 *                            of any one entry of a zstd file in device
 *                            memory, from one walk over the whole file; what
 *                            bounds the device-planned read's zstd scratch.
 *   zsk_verify_frame_checksums — the seek table's per-frame checksum,
 *                            parsed by seek_table.c:95-97 and never checked
 *                            there, checked on the GPU.
 *   zsk_lz4_compress_frames, zsk_writer_set_gpu_compress — the writer's
 *                            per-frame LZ4F_compressFrame call
 *                            (compress.c:750 direct frames, :483 buffered
 *                            ones; prefs compress.c:203-207), batched over
 *                            frames of <= 4 MiB in one grid.
 *   zsk_frame_checksums, zsk_writer_set_checksums — the seek table's
 *                            per-frame checksum on the writing side
 *                            (ZSTD_seekable_logFrame's XXH64 and the 12-byte
 *                            entries of seek_table.c:374-407, which the
 *                            reference's writer never turns on), hashed on
 *                            the GPU for frames that are compressed there.
 *   zsk_write_device       — zseek_write (compress.c:650-833) for bytes that
 *                            are already in device memory.
 *   zsk_zstd_compress_frames, zsk_zstd_build_image — no reference function:
 *                            zstd frames written on the GPU in a fixed format
 *                            subset (valid zstd, not libzstd's bytes), and a
 *                            seekable zstd file built from them in device
 *                            memory.
 *   zsk_lz4_build_image_pieces, zsk_zstd_build_image_pieces — the two image
 *                            builders queued on the caller's stream, their
 *                            answer left in device memory; with a list of
 *                            piece sizes in device memory, one frame per piece
 *                            (a writer's loop of one zseek_write per record,
 *                            compress.c:650-833, planned where the list is).
 *                            zsk_lz4_pieces_bound, zsk_zstd_pieces_bound: their
 *                            capacity, from the piece count alone.
 *   zsk_lz4_append_image_pieces, zsk_zstd_append_image_pieces — a writer that
 *                            stays open (zseek_write as data arrives, the table
 *                            at close, compress.c:650-833) for a file in device
 *                            memory: new frames behind an image's last frame
 *                            and a new table over all of them, on the caller's
 *                            stream.  zsk_lz4_append_bound,
 *                            zsk_zstd_append_bound: the capacity.
 */
#ifndef ZSEEK_HIP_H
#define ZSEEK_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "zseek.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One seek-table frame of a device batch. */
typedef struct {
    uint64_t c_off;   /* compressed frame start in d_comp                  */
    uint64_t d_off;   /* decoded frame start in d_out                      */
    uint32_t c_size;  /* compressed size (seek-table cSize)                */
    uint32_t d_size;  /* decoded size (seek-table dSize); the frame writes */
                      /* exactly [d_off, d_off + d_size) of d_out          */
} zsk_frame_desc_t;

/* Per-frame status codes written to d_status (low 16 bits).  Values 1..19
 * follow liblz4's LZ4F error numbering (see zsk_status_string). */
#define ZSK_OK 0
#define ZSK_ERR_DST_OVERFLOW 100  /* frame decodes past its dSize        */
#define ZSK_ERR_SHORT_FRAME 101   /* frame decodes to less than dSize    */
#define ZSK_ERR_TRUNCATED 102     /* compressed frame ends mid-block     */
#define ZSK_STATUS_DIRECT 0x10000 /* liblz4 would have used its direct path */
#define ZSK_STATUS_BLOCK 0x20000  /* the failure is inside an LZ4 block   */
/* bits 24-25: LZ4 block size id - 4 of a frame that failed in a block */

/*
 * Decode @nframes independent LZ4 frames on the GPU, asynchronously on
 * @stream.  @d_desc, @d_comp, @d_out, @d_status are device pointers;
 * @d_comp must stay readable up to the 4-byte boundary after the last
 * compressed byte.  Each frame writes only its own [d_off, d_off+d_size).
 * Returns 0 if the launch was queued, -1 otherwise.
 *
 * Scratch: the call has no reader to own scratch and takes a set from a pool
 * of at most four per device, for the time the call itself runs on the host
 * (not for the time its kernels run).  Sets are reused in stream order: the
 * set the same stream used last is taken as it is, one whose work has
 * completed by any stream, and otherwise @stream is made to wait
 * (hipStreamWaitEvent) for the least recently used set's last call.  Any
 * number of calls may be queued; with four calls of this entry point (or of
 * zsk_lz4_decode_frames_ex) in progress on a device at once, in other threads,
 * a fifth gets -1 with nothing queued and @d_status and @d_out untouched.
 */
ZSEEK_EXPORT int zsk_lz4_decode_frames(const zsk_frame_desc_t *d_desc,
    uint32_t nframes, const void *d_comp, void *d_out, int32_t *d_status,
    void *stream);

/*
 * Decode @nframes independent zstd frames (each seek-table entry: the zstd
 * frames and skippable frames it holds, as ZSTD_decompressDCtx decodes them)
 * on the GPU, on @stream.  Same descriptors and per-frame status as
 * zsk_lz4_decode_frames; a failed frame's status is ZSK_STATUS_ZSTD | the
 * ZSTD_ErrorCode libzstd 1.4.9 reports for it.  The call synchronizes
 * @stream once, after the planning kernel (a frame's sequence count sizes its
 * scratch), and returns with the decode queued.  Returns 0 or -1.
 *
 * Scratch: pooled as zsk_lz4_decode_frames' (a pool of its own, shared with
 * zsk_zstd_decode_frames_async): at most four sets per device, reused in
 * stream order, held while the call runs on the host -- here that includes
 * the wait for the planning kernel.  A fifth call in progress at once on a
 * device gets -1 with nothing queued and nothing written.
 */
ZSEEK_EXPORT int zsk_zstd_decode_frames(const zsk_frame_desc_t *d_desc,
    uint32_t nframes, const void *d_comp, void *d_out, int32_t *d_status,
    void *stream);
#define ZSK_STATUS_ZSTD 0x4000000 /* zstd frame failure: low bits = ZSTD_ErrorCode */

/*
 * zsk_zstd_decode_frames, stream-ordered.  The descriptors, per-frame statuses
 * and decoded bytes are zsk_zstd_decode_frames'.  Everything is queued on
 * @stream, ordered after what the stream already holds and before what is
 * queued later; the call returns 0 once everything is queued and never waits
 * for the planning kernel.  Instead the caller states @bounds, the host sizes
 * the scratch and the Huffman grids from them before anything is queued, and
 * the device checks its own plan against them behind the planning kernel.
 *
 * A batch that does not fit -- more block headers than max_blocks, more item
 * slots than max_blocks and max_sequences provide, or a frame reaching past
 * out_bytes -- is refused on the device: every d_status[f] of the call becomes
 * ZSK_ERR_SCRATCH, no byte of @d_out is written, and the next call decodes as
 * if nothing had happened.  The remedy is zsk_zstd_decode_frames, which sizes
 * exactly.  (A refused call's statuses read ZSK_ERR_SCRATCH only once the
 * stream has passed the call's last kernel.)
 *
 * zsk_zstd_bounds_default fills @b for @nframes entries decoding into
 * @out_bytes: max_sequences = out_bytes / 3 (a zstd match is at least 3 bytes,
 * so no entry that decodes within out_bytes has more), max_blocks = 2 *
 * nframes + out_bytes / 16384 (libzstd and this project's compressor write
 * 128 KiB blocks: 8x their rate plus two per entry).  A policy, not a
 * guarantee: an entry of many tiny blocks exceeds it and is refused as above.
 * Memory: items are 8 bytes each, two per sequence plus padding -- about 5.4
 * bytes per output byte at the defaults -- a block costs about 11 KiB (table
 * slot, Huffman jobs, ops), and the literal scratch is out_bytes + 64.  A
 * caller who knows its files states tighter bounds.
 *
 * Host waits: only growing the pooled scratch, at first use or after a call
 * with larger bounds (freeing device memory waits for the device) -- the wait
 * zsk_preadv_device_async lists as its (1).  The scratch comes from the pool
 * zsk_zstd_decode_frames uses (at most four sets per device, reused in stream
 * order: see zsk_lz4_decode_frames).  -1 and nothing queued for: a fifth call
 * of the two entry points in progress at once on the device (four other
 * threads inside theirs); NULL @bounds; a stream that is capturing
 * (pooled scratch sized per call: it must never end up in a graph); bounds no
 * device could hold (max_blocks >= 2^29); an allocation or launch failure.
 * nframes == 0 returns 0 and queues nothing.
 */
#define ZSK_ERR_SCRATCH 105   /* the batch did not fit the call's bounds: nothing of the call was decoded */
typedef struct {
    uint64_t out_bytes;      /* every frame's [d_off, d_off + d_size) lies inside d_out[0, out_bytes) */
    uint64_t max_blocks;     /* zstd block headers in all entries of the call together */
    uint64_t max_sequences;  /* sequences (as declared in the sequence sections) in all of them together */
} zsk_zstd_bounds_t;
ZSEEK_EXPORT void zsk_zstd_bounds_default(uint32_t nframes, uint64_t out_bytes, zsk_zstd_bounds_t *b);
ZSEEK_EXPORT int zsk_zstd_decode_frames_async(const zsk_frame_desc_t *d_desc, uint32_t nframes,
    const void *d_comp, void *d_out, int32_t *d_status, const zsk_zstd_bounds_t *bounds, void *stream);

/* Human-readable name of a frame status (LZ4F-style "ERROR_..." names for
 * LZ4 frames, ZSTD_getErrorName strings for zstd frames). */
ZSEEK_EXPORT const char *zsk_status_string(int32_t status);

/*
 * zsk_lz4_decode_frames with one of the library's production decoders forced
 * for every frame (testing, tooling): ZSK_DECODER_AUTO is the library's own
 * choice (= zsk_lz4_decode_frames); WAVE the wave-per-frame decoder; LEAN,
 * SCAN and CHUNK the two-phase decoder with that parse kernel for every frame;
 * BLOCK the two-phase decoder's block route (one parse lane per LZ4 block of
 * each multi-block frame, the chunk parse for the rest) at any batch size.
 * Returns -1 for an unknown decoder.  Scratch and its bound of four calls in
 * progress per device: zsk_lz4_decode_frames' pool (WAVE uses no scratch).
 */
#define ZSK_DECODER_AUTO 0
#define ZSK_DECODER_WAVE 1
#define ZSK_DECODER_LEAN 2
#define ZSK_DECODER_SCAN 3
#define ZSK_DECODER_CHUNK 4
#define ZSK_DECODER_BLOCK 5
/* the one-frame route (every frame through the chunk parse reading it staged
 * in LDS), the library's own choice for batches of <= 64 frames, forced at
 * any size */
#define ZSK_DECODER_ONE 6
ZSEEK_EXPORT int zsk_lz4_decode_frames_ex(const zsk_frame_desc_t *d_desc,
    uint32_t nframes, const void *d_comp, void *d_out, int32_t *d_status,
    void *stream, int decoder);

/* Name of the dominant HIP kernel zsk_lz4_decode_frames launches for a
 * batch of nframes frames (as it appears in a rocprofv3 kernel trace,
 * without namespace), for tooling: the two-phase decoder's execute,
 * seq_exec_kernel, unless the environment forces the
 * wave-per-frame decoder (env ZSEEK_HIP_KERNEL=wave forces it). */
ZSEEK_EXPORT const char *zsk_lz4_kernel_name(uint32_t nframes);

/* Name of the parse kernel the two-phase decoder runs for a frame of
 * @c_size compressed bytes in a batch of @nframes frames (lz4_lean_pair_kernel,
 * lz4_lean_kernel on the block route, lz4_scan_kernel or lz4_chunk_kernel;
 * lz4_wave_kernel for small batches):
 * the library's routing, exposed so tools attribute time and traffic to the
 * kernel that actually runs. */
ZSEEK_EXPORT const char *zsk_lz4_parse_kernel_name(uint32_t nframes, uint32_t c_size);

/* Measurement hook: while on, every two-phase decode launch records HIP
 * events between its stages (plan, parse, execute, hand-off) on its stream,
 * and a zstd launch also around each chunk's kernels on the streams they run
 * on.  zsk_kernel_timing(on) switches it and clears the records;
 * zsk_kernel_times(ms, cap) waits for the recorded launches and writes, per
 * slot, the MEDIAN milliseconds over them into ms[0..min(cap,8)): [0..3] the
 * stages; [4..7] (zstd launches, summed over the launch's chunks)
 * zstd_frame_kernel, zstd_seq_kernel, zstd_huf_kernel and seq_exec_kernel
 * (the zstd literal-source execute).  Returns the
 * number of launches recorded.  Not on any decode path's critical path. */
ZSEEK_EXPORT int zsk_kernel_timing(int on);
ZSEEK_EXPORT int zsk_kernel_times(double *ms, int cap);

/* Number of frames of an open reader and its seek table as prefix sums:
 * c_off/d_off receive n+1 entries each (either may be NULL). */
ZSEEK_EXPORT ssize_t zsk_reader_frames(zseek_reader_t *reader,
    uint64_t *c_off, uint64_t *d_off);

/* Codec of an open reader (ZSEEK_LZ4 / ZSEEK_ZSTD), -1 for NULL. */
ZSEEK_EXPORT int zsk_reader_type(zseek_reader_t *reader);

/*
 * zseek_pread into device memory @d_buf (on the reader's device): decoded
 * bytes [offset, offset+count) are produced on the GPU and never cross PCIe.
 * Same return convention as zseek_pread.  Synchronous.
 */
ZSEEK_EXPORT ssize_t zsk_pread_device(zseek_reader_t *reader, void *d_buf,
    size_t count, size_t offset, void *call_data,
    char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * Vectored read: @nranges ranges of the decoded file in one call.  Every
 * frame the ranges touch is read (one pread callback per run of adjacent
 * touched frames; an untouched frame is never read), decoded once, whole, in
 * batches of at most zsk_reader_set_batch_bytes decoded bytes, and each
 * range's bytes are moved to @buf + dst_off by one segmented copy per batch
 * (zsk_gather_segments).  zsk_preadv: @buf is host memory; zsk_preadv_device:
 * device memory on the reader's device.  Synchronous.
 *
 * Per range, `result` is what looping zseek_pread over it on a reader opened
 * WITH a cache (cache_size >= 1) delivers in total: the bytes before the
 * range's first failed frame (a frame with a non-zero status), short at EOF,
 * 0 for a zero-length range or one at / past EOF, -1 when its first frame
 * fails.  The no-cache partial-read rules of zseek_pread do not apply: frames
 * are decoded whole, whatever the reader's cache_size.
 *
 * Returns the number of ranges delivered in full (result == min(count,
 * size - offset), empty ranges included).  When some range failed, @errbuf
 * holds the text zseek_pread on a cached reader gives for the first failed
 * frame of the LOWEST-INDEX failed range ("decompress frame: ...").  Returns
 * -1 with every result -1 when the whole call fails: NULL reader ("invalid
 * reader"), NULL @ranges with nranges > 0, a pread callback failure ("read
 * file failed" / "unexpected EOF"), a HIP failure, no device.  nranges == 0
 * returns 0.
 *
 * Ranges may be unsorted, share frames, overlap in the source or repeat.
 * Their destination regions [dst_off, dst_off + count) must be DISJOINT
 * (the caller's contract: overlapping destinations are written in no defined
 * order).  Bytes of a range's destination past `result` are unspecified;
 * nothing outside a range's own destination region is written.
 *
 * The call neither consults nor fills the reader's frame cache
 * (zseek_reader_stats' cached_frames is unchanged); it takes the reader's
 * exclusive lock like any decoding read, updates the GPU counters, honours
 * zsk_reader_set_verify_checksums, and runs on the reader's FIRST lane only
 * (zsk_reader_set_devices: the first device; a vectored read is not split
 * over devices).
 */
typedef struct {
    uint64_t offset;   /* decoded offset of the range                         */
    uint64_t count;    /* bytes wanted                                        */
    uint64_t dst_off;  /* the range's bytes go to buf + dst_off               */
    int64_t  result;   /* out: bytes delivered (short at EOF or before a bad  */
                       /* frame), 0 at/after EOF, -1 if its first frame fails */
} zsk_range_t;

ZSEEK_EXPORT ssize_t zsk_preadv(zseek_reader_t *reader, void *buf,
    zsk_range_t *ranges, size_t nranges, void *call_data,
    char errbuf[ZSEEK_ERRBUF_SIZE]);
ZSEEK_EXPORT ssize_t zsk_preadv_device(zseek_reader_t *reader, void *d_buf,
    zsk_range_t *ranges, size_t nranges, void *call_data,
    char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * zsk_preadv_device, stream-ordered: the same read queued on @stream (a
 * hipStream_t of the reader's first lane's device; NULL: HIP's null stream).
 * Everything the call does on the GPU is ordered after what @stream already
 * holds and before what is queued on it afterwards; the call does not wait on
 * the host for its own work and returns 0 once everything is queued, -1 +
 * errbuf otherwise.  A consumer kernel queued on @stream behind the call sees
 * the bytes and the results.
 *
 * @ranges is a host array, read during the call (it may be reused on return);
 * its `result` fields are not written.  The results go to @d_result, device
 * memory of nranges + 1 int64_t: when the stream reaches the end of the
 * call's work, d_result[i] holds exactly what zsk_preadv_device would have put
 * in ranges[i].result (the full count when every touched frame decoded, short
 * at EOF, 0 for an empty range or one at / past EOF, the bytes before the
 * first failed frame, -1 when the first frame fails) and d_result[nranges]
 * what it would have returned: the number of ranges delivered in full.  The
 * bytes in @d_buf follow zsk_preadv_device's rules: disjoint destinations,
 * nothing outside a range's destination written, bytes past `result`
 * unspecified.  No error text can be deferred: errbuf is written only for
 * failures the call itself sees.  For the "decompress frame: ..." text of a
 * failed range, repeat that range with zsk_preadv_device.
 *
 * Honours zsk_reader_set_verify_checksums and zsk_reader_set_batch_bytes like
 * the synchronous call; neither consults nor fills the frame cache; holds the
 * reader's exclusive lock for the duration of the call (the enqueue) only;
 * the GPU counters (batches, frames_decoded, bytes_decoded, bytes_uploaded)
 * advance at enqueue.
 *
 * LZ4 readers, over a host image or a device image (zsk_reader_open_device).
 * A zstd reader: -1, "asynchronous read: zstd is not supported", unless
 * zsk_reader_set_zstd_async has turned it on (below).  On a host image the pread callbacks run on the calling
 * thread during the call, one per run of adjacent touched frames; only the
 * GPU work is deferred.
 *
 * -1 and nothing queued for: a NULL reader ("invalid reader"); a stream that
 * is capturing ("asynchronous read: stream is capturing" -- the call reuses
 * pinned staging, so it must never end up in a graph); a zstd reader without
 * zsk_reader_set_zstd_async; NULL
 * @ranges or NULL @d_result with nranges > 0; NULL @d_buf when some range has
 * bytes ("invalid buffer"); no device.  nranges == 0 returns 0 and queues only
 * d_result[0] = 0 (nothing for a NULL @d_result).  The call may also fail
 * after some batches were queued -- a pread callback failure, "unexpected
 * EOF", a batch spanning 2 GiB of a device image, a HIP error: it then still
 * queues a fill of d_result[0 .. nranges] with -1, so a stream-ordered
 * consumer sees the failure, and returns -1 + the usual text; @d_buf is then
 * unspecified inside the ranges' destinations and untouched outside them.
 *
 * Host waits the call may make: (1) growing a batch slot's buffers, the LZ4
 * parse scratch or the per-call table -- at first use and after a larger call
 * (freeing device memory waits for the device); (2) reusing a batch slot or a
 * per-call table whose previous asynchronous batch has not finished: a reader
 * has three of each per device, taken in turn across calls, so this happens
 * to a call of more than three batches and to a fourth batch (or call) in
 * flight.
 *
 * Every synchronous read on the same reader (zseek_pread, zseek_read,
 * zsk_pread_device, zsk_preadv, zsk_preadv_device) stays correct while
 * asynchronous work is in flight: each first waits for what it needs.
 * zseek_reader_close waits for all of the reader's queued work before it
 * frees anything; @d_buf, @d_result and, for a device-image reader, the image
 * must stay valid until the work has run.
 */
ZSEEK_EXPORT ssize_t zsk_preadv_device_async(zseek_reader_t *reader, void *d_buf,
    const zsk_range_t *ranges, size_t nranges, int64_t *d_result, void *stream,
    void *call_data, char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * zsk_preadv_device_async on a zstd reader.  Off by default (@seq_bytes 0:
 * the refusal above).  @seq_bytes >= 3 turns it on; 1 and 2 return false, as
 * does a NULL reader.  Env ZSEEK_ZSTD_ASYNC=<n> at open does the same.
 *
 * When on, each batch of the call is decoded by zsk_zstd_decode_frames_async's
 * machinery on the batch slot's own scratch -- no host plan, no wait -- with
 * bounds taken from the seek table: out_bytes the batch's decoded span,
 * max_sequences = span / seq_bytes, max_blocks the sum over its frames of
 * 2 + d_size / 16384.  With 3, no file that decodes overflows the sequence
 * bound; larger values save memory (16 / seq_bytes bytes of items per decoded
 * byte) and give that guarantee up.  A batch that does not fit its bounds
 * is refused whole on the device: its frames carry ZSK_ERR_SCRATCH, its ranges
 * come out short or -1 like any failed frame's, and d_result[nranges] counts
 * the rest.  The remedy is the usual one: repeat those ranges with
 * zsk_preadv_device, which sizes exactly.  Everything else is the LZ4
 * contract above; growing a slot's zstd scratch is one of its waits (1).
 * zsk_preadv_device_indirect does not use this setting: on a zstd reader it
 * is bounded by zsk_reader_zstd_census (below).
 */
ZSEEK_EXPORT bool zsk_reader_set_zstd_async(zseek_reader_t *reader, unsigned seq_bytes);

/*
 * zsk_preadv_device_async for a range list that is itself in DEVICE memory,
 * on a reader over a device image (zsk_reader_open_device; LZ4, or zstd after
 * zsk_reader_zstd_census, below): the plan --
 * which frames the ranges touch, their descriptors, the (range, frame)
 * segments -- is computed by kernels on @stream from the seek table the
 * reader keeps on the device, so ranges produced on the GPU (a sampler, an
 * index lookup, an earlier read) never visit the host.  Nothing but the
 * call's arguments goes host -> device, no pinned staging is rewritten, and
 * the host waits only as listed below.
 *
 * @d_ranges: @nranges zsk_range_t in device memory, read on @stream: work
 * queued on @stream before the call may have written them; they must stay
 * valid until the stream has passed the call's work; their `result` fields
 * are never written.  @d_result: nranges + 1 int64_t in device memory.
 * @d_buf[0, buf_size): the destination.
 *
 * When the stream reaches the end of the call's work, d_result[i],
 * d_result[nranges] and the bytes in @d_buf are exactly what
 * zsk_preadv_device_async leaves for the same ranges on the same reader (the
 * full count; short at EOF; 0 for an empty range or one at / past EOF; the
 * bytes before the first failed frame; -1 when the first frame fails; in
 * d_result[nranges] the ranges delivered in full).  Ranges may be unsorted,
 * overlap in the source, share frames or repeat; destinations must be
 * disjoint.  offset + count may wrap: the range ends at EOF.
 *
 * The list is data, not trusted input: a range whose destination [dst_off,
 * dst_off + count) is not inside [0, buf_size) gets -1, moves no byte and is
 * not counted as delivered.  A garbage list can produce wrong results; it can
 * never make the call write outside d_buf[0, buf_size).
 *
 * @max_frames is the caller's bound on the distinct frames one call touches.
 * The call is ONE batch: it reserves max_frames x (the file's largest frame
 * dSize) of decoded staging and is refused up front when that exceeds the
 * reader's batch size (zsk_reader_set_batch_bytes): -1, "device-planned
 * read: max_frames frames exceed the batch size" (and, a segment's length
 * being 32 bits, when it reaches 4 GiB: "... exceed 4 GiB").
 *
 * Segments: a host-planned read moves one segment per (range, frame)
 * overlap, which nranges + max_frames slots hold for ranges that are disjoint
 * in the source (sorted by offset, two neighbours share at most one frame and
 * every other frame belongs to one range: at most touched frames + nranges -
 * 1) but not for ranges that overlap or repeat.  This call needs no such
 * bound: the frames a range touches lie back to back in the decoded staging,
 * so a range is ONE segment, nranges in all, moved when the range's first
 * frame decoded.  The bytes before the first failed frame are delivered as
 * always; what is moved behind them stays inside the range's own destination,
 * past its result, where bytes are unspecified.  No list of @nranges ranges
 * can run out of segments.
 *
 * When the ranges touch more than max_frames frames, nothing is decoded or
 * moved: @d_buf is untouched, every d_result[i] is -1 and d_result[nranges]
 * is ZSK_PLAN_OVERFLOW.  When the
 * compressed bytes from the first touched frame's start to the last one's end
 * are 2 GiB (less 256 bytes) or more -- the parse kernels address a batch
 * through 32-bit offsets -- the outcome is the same with ZSK_PLAN_SPAN; the
 * check is made on the device per call, so a larger image works for every read
 * that stays within 2 GiB.
 *
 * Honours zsk_reader_set_verify_checksums (the touched frames' words come
 * from the resident table); neither consults nor fills the frame cache; holds
 * the reader's exclusive lock for the enqueue only.  Counters: `batches`
 * advances by 1 at enqueue; frames_decoded and bytes_decoded do NOT advance
 * (the host never learns what the ranges touched); bytes_uploaded stays 0.
 *
 * -1 + errbuf and nothing queued for: a NULL reader ("invalid reader"); a
 * reader not opened with zsk_reader_open_device ("device-planned read: needs
 * a device image"); a zstd reader whose census has not been taken
 * ("device-planned read: zstd is not supported"); a capturing stream ("device-planned read: stream is
 * capturing"); nranges > 0 with NULL @d_ranges, NULL @d_result or max_frames
 * == 0; nranges > 0, buf_size > 0 and NULL @d_buf ("invalid buffer"); the
 * staging refusal above; a seek table that reaches past the image
 * ("unexpected EOF").  nranges == 0 returns 0 and queues only d_result[0] = 0
 * (nothing for a NULL @d_result).  A HIP failure after something was queued
 * still queues a fill of d_result[0 .. nranges] with -1 and returns -1.
 *
 * Host waits the call may make: growing its buffers (first use, a larger
 * call), and reusing one of the reader's three batch slots or call tables
 * while an earlier asynchronous call still runs on it -- the slots and tables
 * are taken in turn, as zsk_preadv_device_async takes them.  Synchronous
 * reads on the same reader stay correct while such a call is in flight, and
 * zseek_reader_close waits for it.  Not for a capturing stream; not for host
 * images; a read of more than one batch is the caller's loop.
 *
 * A zstd reader.  The host never sees which frames a call touches, so it
 * cannot size the zstd scratch from them; it sizes it from the file's census:
 * accepted once zsk_reader_zstd_census has succeeded on the reader (before
 * that: the refusal above), whatever zsk_reader_set_zstd_async says.  The
 * batch is decoded by zsk_zstd_decode_frames_async's machinery with out_bytes
 * = max_frames x the file's largest dSize, max_blocks = max_frames x the
 * census' max_blocks and max_sequences = max_frames x its max_sequences, which
 * no max_frames entries of the file exceed: no read of an unmodified image is
 * ever refused for scratch, a file of many tiny blocks included.  -1,
 * "device-planned read: max_frames frames exceed the zstd block bound" and
 * nothing queued when max_frames x max_blocks reaches 2^29.  Growing the
 * slot's zstd scratch to those bounds is one of the host waits.  Everything
 * else is the contract above.
 *
 * The device still checks its own plan against the bounds: an image whose
 * bytes were rewritten after the census (against zsk_reader_open_device's
 * contract) so that a batch exceeds them is refused whole on the device, as in
 * zsk_preadv_device_async -- every touched frame carries ZSK_ERR_SCRATCH, the
 * ranges come out -1 or short, d_result[nranges] counts the rest, nothing
 * outside the ranges' destinations is written, and the next call decodes
 * normally.
 */
#define ZSK_PLAN_OVERFLOW (-2)  /* more touched frames than the call reserved */
#define ZSK_PLAN_SPAN     (-3)  /* the touched frames span 2 GiB or more of the image */
ZSEEK_EXPORT ssize_t zsk_preadv_device_indirect(zseek_reader_t *reader,
    void *d_buf, size_t buf_size,
    const zsk_range_t *d_ranges, size_t nranges, size_t max_frames,
    int64_t *d_result, void *stream, char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * Whole frames by INDEX, the indices in DEVICE memory, each frame decoded in
 * place: the read side of zsk_lz4_build_image_pieces / zsk_zstd_build_image_
 * pieces, where the frame index is the record index.  On a reader over a
 * device image (zsk_reader_open_device; LZ4, or zstd after
 * zsk_reader_zstd_census, below).  Slot i of the list (i < @nidx) asks for
 * seek-table frame d_idx[i], whole.  Kernels on @stream turn the list into
 * frame descriptors from the seek table the reader keeps on the device --
 * sizes, a scan of them, destinations -- and the decode kernels write every
 * frame straight into @d_buf at its slot's offset: no staging, no gather, no
 * seek-table download, no max_frames to guess, and each decoded byte is
 * written once.  Nothing but the call's arguments goes host -> device, no
 * pinned staging is rewritten, and the host waits only as listed below.
 *
 * @d_idx: @nidx int64_t in device memory, read on @stream: work queued on
 * @stream before the call may have written them; they must stay valid and
 * unchanged until the stream has passed the call's work; they are never
 * written.  @d_result: nidx + 1 int64_t in device memory.  @d_buf[0,
 * buf_size): the destination, 16-byte aligned.  The call returns 0 once
 * everything is queued.
 *
 * Layout.  @stride == 0, packed: slot i goes to d_buf + d_offsets[i], where
 * d_offsets[i] is the sum of the decoded sizes of the valid slots before i (a
 * slot whose index is invalid counts 0) and d_offsets[nidx] the total.  The
 * total is written whatever @buf_size is, so a caller whose buffer was too
 * small learns the size it needs.  @d_offsets: nidx + 1 uint64_t in device
 * memory, required.  @stride > 0, padded rows: slot i goes to d_buf + i *
 * stride; @d_offsets may be NULL, and when given receives i * stride, and nidx
 * * stride in its last entry.
 *
 * When the stream reaches the end of the call's work, d_result[i] is
 *   - the frame's decoded size when the frame was decoded and its status is
 *     ZSK_OK (with zsk_reader_set_verify_checksums on: and its seek-table
 *     checksum matched; the words come from the resident table);
 *   - 0 for a frame of decoded size 0: delivered, nothing decoded, wherever
 *     its offset lies;
 *   - -1 when the index is no frame of the file (negative, or >= frames), when
 *     the slot's region [off, off + size) is not inside [0, buf_size), when
 *     in rows mode size > stride (a frame is never truncated to its row), or
 *     when the frame failed;
 * and d_result[nidx] is the number of delivered slots (those with d_result[i]
 * >= 0).
 *
 * The list is data, not trusted input: a garbage list gives -1 slots; it can
 * never make the call write outside d_buf[0, buf_size).  Nothing outside the
 * slots' own regions is ever written -- in rows mode the bytes between a
 * frame's end and the next row are untouched -- and the bytes of a failed
 * slot's region are unspecified.
 *
 * Duplicates.  A repeated index is decoded once per occurrence, each into its
 * own region: two slots, two decodes.  Removing duplicates would need the
 * touched-frame bitmap, a staging buffer and a copy per slot, which is what
 * this call exists to avoid; a caller whose lists repeat heavily uses
 * zsk_preadv_device_indirect.
 *
 * Span.  When the compressed bytes from the lowest touched frame's start to
 * the highest one's end (over the slots with a valid index and a non-empty
 * frame, fitting or not) are 2 GiB (less 256 bytes) or more -- the parse
 * kernels address a wave's frames through one 32-bit buffer resource --
 * nothing is decoded: @d_buf is untouched, every d_result[i] is -1 and
 * d_result[nidx] is ZSK_PLAN_SPAN.  d_offsets is written as always.  The check
 * is made on the device per call, as in zsk_preadv_device_indirect.
 *
 * The call is ONE batch.  Its parse scratch and, for zstd, its literal scratch
 * are bounded by nidx x (stride ? stride : the file's largest frame dSize); it
 * is refused up front when that exceeds the reader's batch size
 * (zsk_reader_set_batch_bytes): -1, "frame-list read: the list exceeds the
 * batch size" (and when it reaches 4 GiB: "... exceeds 4 GiB").  A longer
 * list is the caller's loop.
 *
 * Neither consults nor fills the frame cache; holds the reader's exclusive
 * lock for the enqueue only.  Counters: `batches` advances by 1 at enqueue;
 * frames_decoded and bytes_decoded do NOT advance (the host never learns what
 * the list asked for); bytes_uploaded stays 0.
 *
 * -1 + errbuf and nothing queued for: a NULL reader ("invalid reader"); a
 * reader not opened with zsk_reader_open_device ("frame-list read: needs a
 * device image"); a zstd reader whose census has not been taken ("frame-list
 * read: zstd is not supported"); a capturing stream ("frame-list read: stream
 * is capturing"); nidx > 0 with NULL @d_idx ("invalid index list") or NULL
 * @d_result ("invalid result buffer"); stride == 0 with NULL @d_offsets
 * ("frame-list read: the packed layout needs d_offsets"); buf_size > 0 and
 * NULL @d_buf ("invalid buffer"); a @d_buf that is not 16-byte aligned; a
 * @d_idx, @d_offsets or @d_result that is not 8-byte aligned; the batch
 * refusals above; on a zstd reader nidx x the census' max_blocks at 2^29
 * ("frame-list read: the list exceeds the zstd block bound"); a seek table
 * that reaches past the image ("unexpected EOF").  nidx == 0 returns 0 and
 * queues only d_result[0] = 0 and, when @d_offsets is given, d_offsets[0] = 0.
 * A HIP failure after something was queued still queues a fill of d_result[0
 * .. nidx] with -1 and returns -1.
 *
 * Host waits the call may make: growing its buffers (first use, a longer
 * list), and reusing one of the reader's three batch slots or call tables
 * while an earlier asynchronous call still runs on it -- taken in turn, as
 * zsk_preadv_device_async and zsk_preadv_device_indirect take them.
 * Synchronous reads on the same reader stay correct while such a call is in
 * flight, and zseek_reader_close waits for it.  Not for a capturing stream;
 * not for host images.
 *
 * A zstd reader.  Accepted once zsk_reader_zstd_census has succeeded on the
 * reader, whatever zsk_reader_set_zstd_async says.  The batch is decoded by
 * zsk_zstd_decode_frames_async's machinery.  Its literal scratch is laid out
 * like the output -- slot i's literals at its destination offset -- so
 * out_bytes covers the destination span and not the frames' sizes: out_bytes
 * = min(buf_size, nidx x (stride ? stride : the file's largest dSize)),
 * max_blocks = nidx x the census' max_blocks, max_sequences = nidx x its
 * max_sequences, which no nidx entries of the file exceed.  A wide stride
 * therefore costs literal scratch (and batch size) although the rows are
 * mostly padding.  The device still checks its own plan against the bounds: an
 * image rewritten after the census so that a batch exceeds them is refused
 * whole on the device -- every non-empty slot gets -1, nothing outside the
 * slots' regions is written, and the next call decodes normally.
 */
ZSEEK_EXPORT ssize_t zsk_read_frames_indirect(zseek_reader_t *reader,
    const int64_t *d_idx, size_t nidx, size_t stride,
    void *d_buf, size_t buf_size,
    uint64_t *d_offsets, int64_t *d_result,
    void *stream, char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * The census of a zstd reader over a device image: one kernel, a lane per
 * seek-table entry of the WHOLE file, walks every entry's frame, block and
 * literals headers and sequence counts (the walk the decoder's planning kernel
 * makes per batch) and keeps the maxima over the entries.  The image is
 * immutable for the life of the reader, so the walk runs once: the first call
 * takes the reader's exclusive lock, runs the kernel on the reader's own
 * stream (its first batch slot's; the kernel reads only the image and the
 * resident table), waits once for the three words to come back and stores
 * them in the reader; every later call
 * returns the stored numbers with no GPU work.  The reader keeps no device
 * memory for it.
 *
 * What it is for: @max_frames x (max_blocks, max_sequences, max_dsize) bound
 * any max_frames entries of the file, which is how zsk_preadv_device_indirect
 * sizes its zstd scratch (above).  The same products are valid
 * zsk_zstd_bounds_t for a caller of zsk_zstd_decode_frames_async over any
 * max_frames entries of this file (out_bytes: wherever the caller's
 * descriptors put them).  max_items is the largest single entry's item-slot
 * need, for information: the scratch is sized from the other two.
 * zsk_preadv_device_async does not use the census.
 *
 * 0 and *@census filled; a file with no frames gives all zeros.  -1 + errbuf
 * for: a NULL reader ("invalid reader"); a NULL @census ("invalid census
 * pointer"); a reader not opened with zsk_reader_open_device ("zstd census:
 * needs a device image"); an LZ4 reader ("zstd census: not a zstd reader"); a
 * seek table that reaches past the image ("unexpected EOF"); a HIP failure.
 */
typedef struct {
    uint64_t frames;         /* seek-table entries walked                               */
    uint64_t max_items;      /* most 8-byte item slots one entry's plan asks for        */
    uint64_t max_blocks;     /* most zstd block headers in one entry                    */
    uint64_t max_sequences;  /* most sequences one entry's sequence sections declare    */
    uint32_t max_dsize;      /* the file's largest frame, decoded ...                   */
    uint32_t max_csize;      /* ... and compressed                                      */
} zsk_zstd_census_t;
ZSEEK_EXPORT int zsk_reader_zstd_census(zseek_reader_t *reader, zsk_zstd_census_t *census,
    char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * The device-side building block, for callers of zsk_*_decode_frames: copy
 * d_src[src_off, src_off + len) to d_dst[dst_off, dst_off + len) for each of
 * the @nseg segments in @d_seg (device memory) whose d_status[frame] is
 * ZSK_OK; a NULL @d_status copies every segment.  Any byte alignment on both
 * sides, len 0 .. 4 GiB - 1, one to hundreds of thousands of segments per
 * call; the work is balanced by bytes, not by segment.  The kernel never
 * writes a byte outside [dst_off, dst_off + len), and reads nothing outside
 * the aligned 4-byte words that contain bytes of [src_off, src_off + len)
 * (so @d_src must be readable up to the next 4-byte boundary on both ends,
 * which holds for any allocation).  Source and destination bytes must not
 * overlap, and destinations must be disjoint.  Asynchronous on @stream (the
 * segments are read on the stream too: keep @d_seg alive until it has
 * passed).  Returns 0 if queued (nseg == 0: nothing to do, 0), -1 otherwise.
 * The segments' prefix sum goes into pooled scratch (a pool of this entry
 * point's own; see zsk_lz4_decode_frames): at most four sets per device,
 * reused in stream order, held while the call runs on the host; a fifth call
 * in progress at once on a device gets -1 with nothing queued.
 */
typedef struct {
    uint64_t src_off;  /* into d_src                                        */
    uint64_t dst_off;  /* into d_dst                                          */
    uint32_t len;      /* bytes                                               */
    uint32_t frame;    /* index into d_status                                 */
} zsk_segment_t;

ZSEEK_EXPORT int zsk_gather_segments(const zsk_segment_t *d_seg,
    uint32_t nseg, const void *d_src, void *d_dst, const int32_t *d_status,
    void *stream);

/* GPU-side counters of a reader.  zsk_reader_gpu_stats fills the fields
 * through `device` (the struct's layout before copy_threads / io_parts were
 * added, so a caller built against that header is never written past its
 * struct); zsk_reader_gpu_stats_ex(reader, stats, sizeof *stats) fills the
 * first @size bytes of the current layout (at most its size). */
typedef struct {
    uint64_t batches;          /* decode grids launched                 */
    uint64_t frames_decoded;   /* frames decoded on the GPU             */
    uint64_t bytes_decoded;    /* decoded bytes produced on the GPU     */
    uint64_t bytes_uploaded;   /* compressed bytes copied host->device  */
    uint64_t device_memory;    /* device bytes held by the reader       */
    int device;                /* HIP device ordinal, -1 before first use */
    int copy_threads;          /* host copy / pread pool threads (usable CPUs - 2, 2..16) */
    int io_parts;              /* concurrent pread callbacks a batch uses: min(io_threads, copy_threads / 2) */
} zsk_gpu_stats_t;

ZSEEK_EXPORT bool zsk_reader_gpu_stats(zseek_reader_t *reader,
    zsk_gpu_stats_t *stats);
ZSEEK_EXPORT bool zsk_reader_gpu_stats_ex(zseek_reader_t *reader,
    zsk_gpu_stats_t *stats, size_t size);

/* Largest decoded span one batch grid covers (bytes, default 64 MiB; env
 * ZSEEK_HIP_BATCH_BYTES overrides at open).  A read runs as a pipeline of
 * such batches (the user pread of one, the upload / decode / download of
 * the next and the copy into the caller's buffer of a third overlap); its
 * first batch is at most 4 MiB. */
ZSEEK_EXPORT bool zsk_reader_set_batch_bytes(zseek_reader_t *reader,
    size_t bytes);

/*
 * Seek-table frame checksums.  The seekable format's optional per-frame
 * checksum (descriptor bit 7; 12-byte entries cSize, dSize, checksum,
 * seek_table.c:95-97 / writer :392-396) is the low 32 bits of XXH64(seed 0)
 * of the frame's decoded bytes; the reference parses it and never checks it.
 *
 * zsk_verify_frame_checksums: for every frame whose d_status is ZSK_OK, hash
 * d_out[d_off, d_off + d_size) on the GPU and set its status to
 * ZSK_ERR_SEEK_CHECKSUM when the low 32 bits differ from d_checksums[f]
 * (device array, one u32 per frame).  Asynchronous on @stream; 0 or -1.
 */
#define ZSK_ERR_SEEK_CHECKSUM 104
ZSEEK_EXPORT int zsk_verify_frame_checksums(const zsk_frame_desc_t *d_desc,
    uint32_t nframes, const void *d_out, const uint32_t *d_checksums,
    int32_t *d_status, void *stream);

/* The compute form of the same hash:
 * d_checksums[f] = low 32 bits of XXH64(seed 0) of d_data[d_off, d_off + d_size)
 * for each of the nframes descriptors (c_off / c_size ignored).  d_size 0 is
 * valid (0x51D8E999).  Reads nothing outside a frame's bytes; writes exactly
 * d_checksums[0, nframes).  Asynchronous on stream; 0 or -1; nframes == 0: 0. */
ZSEEK_EXPORT int zsk_frame_checksums(const zsk_frame_desc_t *d_desc, uint32_t nframes,
    const void *d_data, uint32_t *d_checksums, void *stream);

/* Make a reader check the seek-table checksum of every frame it decodes
 * (files whose seek table carries them).  Default off, as the reference; env
 * ZSEEK_VERIFY_CHECKSUMS=1 at open turns it on.  A mismatching frame fails
 * like a corrupt one: a short read, then -1 and "...: frame checksum
 * mismatch".  false for a NULL reader. */
ZSEEK_EXPORT bool zsk_reader_set_verify_checksums(zseek_reader_t *reader,
    bool on);

/*
 * Allow up to @n concurrent calls of the reader's pread callback (on
 * disjoint ranges of >= 4 MiB of one batch's compressed span).  Default 1,
 * the reference's contract: it calls pread under the reader's lock, one call
 * at a time, and its default FILE* callback is not safe to call concurrently.
 * Only for callbacks that are (an in-memory image, pread(2) on a descriptor).
 * The calls run on the library's host pool, at most half of it at once (the
 * rest keeps copying decoded batches out): zsk_gpu_stats_t.io_parts.
 * Env ZSEEK_IO_THREADS at open.  false for a NULL reader or n outside 1..64.
 */
ZSEEK_EXPORT bool zsk_reader_set_io_threads(zseek_reader_t *reader, int n);

/*
 * The devices a reader decodes on: one decode pipeline ("lane") per entry; a
 * multi-frame read is split into contiguous frame ranges by decoded bytes,
 * one per lane, decoded concurrently (host destinations: each lane copies its
 * part into the caller's buffer; zsk_pread_device: each lane copies its part
 * into the destination, peer-to-peer from another device).  A device may
 * repeat (several pipelines on one GPU).  Default: env ZSEEK_HIP_DEVICES
 * ("0,1,2,3") at the first read, else ZSEEK_HIP_DEVICE, else the calling
 * thread's current device.  false for a NULL reader or an invalid device.
 * zsk_reader_devices writes up to @cap entries and returns the count (0
 * before the first read has picked the default).
 */
ZSEEK_EXPORT bool zsk_reader_set_devices(zseek_reader_t *reader,
    const int *devices, int n);
ZSEEK_EXPORT int zsk_reader_devices(zseek_reader_t *reader, int *devices,
    int cap);

/*
 * LZ4 frame compression, byte-identical to the reference
 * writer's frames: LZ4F_compressFrame(level, autoFlush = 1, 64 KiB blocks) of
 * liblz4 1.9.3, as compress.c:737-786 / :463-518 call it.  One frame per
 * descriptor, src_size <= ZSK_LZ4_COMPRESS_MAX_FRAME (one independent block
 * up to 64 KiB, linked 64 KiB blocks above; larger frames are refused with
 * c_size 0).  ZSK_COMPRESS_CONTENT_SIZE = the writer's contentSize != 0 case
 * (a buffered frame flushed by end_frame_lz4, compress.c:472): the header
 * then carries the frame's size.
 */
typedef struct {
    uint64_t src_off;   /* frame input start in d_src                        */
    uint64_t dst_off;   /* output slot start in d_dst: 16-byte aligned, at    */
                        /* least ZSK_LZ4_COMPRESS_BOUND(src_size) bytes       */
    uint32_t src_size;  /* <= ZSK_LZ4_COMPRESS_MAX_FRAME                      */
    uint32_t flags;     /* ZSK_COMPRESS_CONTENT_SIZE                          */
} zsk_compress_desc_t;
#define ZSK_COMPRESS_CONTENT_SIZE 1u
#define ZSK_LZ4_COMPRESS_MAX_FRAME (1u << 22)
#define ZSK_LZ4_COMPRESS_BOUND(n) \
    ((((uint64_t)(n)) + 4 * (((uint64_t)(n)) >> 16) + 24 + 15) & ~(uint64_t)15)

/* Device scratch bytes zsk_lz4_compress_frames needs for @nframes frames
 * (a 64 KiB table of position + input-word entries per frame); size scratch
 * with this call, not from the comment. */
ZSEEK_EXPORT size_t zsk_lz4_compress_scratch_size(uint32_t nframes);

/*
 * Compress @nframes frames on the GPU, asynchronously on @stream: frame f's
 * bytes d_src[src_off, src_off + src_size) become one LZ4 frame written at
 * d_dst + dst_off, its size in d_csize[f] (0 for a refused descriptor).
 * @level is the writer's compressionLevel (< 3: liblz4's fast encoder,
 * acceleration 1 - level for negative levels; HC levels return -1).
 * @d_scratch holds zsk_lz4_compress_scratch_size(nframes) bytes.  All
 * pointers are device pointers.  Returns 0 if queued, -1 otherwise.
 */
ZSEEK_EXPORT int zsk_lz4_compress_frames(const zsk_compress_desc_t *d_desc,
    uint32_t nframes, const void *d_src, void *d_dst, uint32_t *d_csize,
    int level, void *d_scratch, void *stream);

/*
 * zstd frame compression on the GPU.  Each descriptor becomes one valid zstd
 * frame (RFC 8878) that libzstd decodes to the input; the bytes are NOT
 * libzstd's at any level, there is one effort level and no level parameter.
 * The format subset (csrc/zstd_enc_dev.h): a single-segment header with the
 * content size always present (ZSK_COMPRESS_CONTENT_SIZE is ignored) and no
 * dictionary id; blocks of 128 KiB of input, each encoded on its own --
 * Compressed when that is smaller, RLE for one repeated byte, Raw otherwise;
 * literals Raw, RLE or Huffman (code lengths <= 11, the tree as direct 4-bit
 * weights, so literals that hold a byte above 128 are stored Raw:
 * FSE-compressed weight descriptions are not written); sequences over the
 * predefined LL / OF / ML tables with every offset coded as offset + 3 (no
 * repeat offsets, no repeated or custom tables).  A 0-byte frame is the header
 * and one empty last Raw block (9 bytes).  ZSK_COMPRESS_CONTENT_CHECKSUM in a
 * descriptor's flags ends its frame with the low 32 bits of XXH64 (seed 0) of
 * its content.  src_size <= ZSK_ZSTD_COMPRESS_MAX_FRAME; a larger frame is
 * refused with c_size 0 and its slot is left untouched.
 *
 * zsk_zstd_compress_frames follows zsk_lz4_compress_frames' contract:
 * asynchronous on @stream, dst_off 16-byte aligned, every slot at least
 * ZSK_ZSTD_COMPRESS_BOUND(src_size) bytes (all blocks Raw) and nothing written
 * outside it, no source byte read outside the frame, nframes == 0 returns 0,
 * a @d_scratch smaller than zsk_zstd_compress_scratch_size(nframes, total
 * source bytes) returns -1.  The same input gives the same bytes on every run.
 */
#define ZSK_ZSTD_COMPRESS_MAX_FRAME (1u << 22)
#define ZSK_COMPRESS_CONTENT_CHECKSUM 2u
#define ZSK_ZSTD_COMPRESS_BOUND(n) \
    ((9 + 3 * ((uint64_t)(n) ? (((uint64_t)(n)) + 131071) >> 17 : 1) + ((uint64_t)(n)) + 4 + 15) & ~(uint64_t)15)
ZSEEK_EXPORT size_t zsk_zstd_compress_scratch_size(uint32_t nframes, uint64_t src_bytes);
ZSEEK_EXPORT int zsk_zstd_compress_frames(const zsk_compress_desc_t *d_desc,
    uint32_t nframes, const void *d_src, void *d_dst, uint32_t *d_csize,
    void *d_scratch, size_t scratch_size, void *stream);

/*
 * The same call with the format as an argument.  ZSK_ZSTD_FORMAT_SUBSET is
 * zsk_zstd_compress_frames, byte for byte.  ZSK_ZSTD_FORMAT_FULL
 * (csrc/zstd_enc_full_dev.h) keeps the subset's frame header, 128 KiB blocks,
 * block-type rule (Compressed only when smaller than the block's input),
 * stream count and match search, and changes four things:
 *   literals  Huffman over all 256 byte values (code lengths <= 11).  The tree
 *             is described by direct 4-bit weights (legal when at most 128 are
 *             listed) or by FSE-compressed weights (header byte < 128,
 *             accuracy log <= 6, two interleaved states), whichever is
 *             smaller, direct on a tie.  Where neither is legal (all listed
 *             weights equal; 128 bytes or more) or Huffman is not smaller, the
 *             literals are Raw, or RLE for one repeated byte.
 *   tables    LL, OF and ML are each Predefined, RLE (every sequence of the
 *             block has the same code) or FSE_Compressed, per block.  A block
 *             of fewer than 8 sequences uses the predefined tables.  Otherwise
 *             the accuracy log is highbit(nseq - 1) - 2, at least
 *             min(highbit(nseq) + 1, highbit(largest code) + 2) and 5, at most
 *             9 (LL, ML) or 8 (OF); a count below one table cell is "less than
 *             one", the others round half up, the difference to the table
 *             size goes to (or comes one at a time from) the largest share;
 *             and the mode with the lowest cost in 1/256 bit wins, Predefined
 *             on a tie: description bits + accuracy log + per sequence
 *             (accuracy log - log2 of the code's share) in 8-bit fixed point.
 *   offsets   repeat codes: an offset equal to one of the three last offsets
 *             is coded 1..3 by RFC 8878 3.1.1.5 (without literals before the
 *             match: the second, the third, the first minus one; the first
 *             itself is then coded plain).  The history starts at 1, 4, 8 in
 *             every frame, passes from block to block, and only a block that
 *             is written Compressed moves it on.
 * Still not written: matches into earlier blocks, Repeat_Mode or treeless
 * tables, dictionaries, frames above ZSK_ZSTD_COMPRESS_MAX_FRAME, levels.
 * The contract is zsk_zstd_compress_frames' whole: asynchronous on @stream,
 * one compress kernel per call, the same slots and bound, nothing written
 * outside them, no source byte read outside the frame, a frame above the cap
 * refused with c_size 0 and its slot untouched, the same bytes on every run,
 * ZSK_COMPRESS_CONTENT_CHECKSUM honoured.  An unknown @format returns -1 (0
 * from the scratch size) and queues nothing.
 *
 * ZSK_ZSTD_FORMAT_FULL_WIDE (csrc/zstd_enc_wide_dev.h; ZSK_ZSTD_FORMAT_FULL | 4,
 * bit 2 selecting the search) is the full format over a wider match search;
 * the format layer -- header, blocks, block-type rule, literals, table modes,
 * repeat offsets, checksum -- is the full format's, only the sequences handed
 * to it differ:
 *   n <= 16384  the full format's search (hash log 12, a table per block): the
 *               frame is ZSK_ZSTD_FORMAT_FULL's frame byte for byte.
 *   n >  16384  h = (v * 2654435761u) >> (32 - 14) over the 4 bytes v at a
 *               position; one table of 2^14 entries holding position + 1
 *               relative to the frame's start (0: empty), zeroed once, at the
 *               frame's start.  Block b's search is the full format's -- 64
 *               positions a step; the lowest position whose candidate's 4
 *               bytes match wins; the match extends to at most the block's own
 *               end; the step's positions below the next step's start enter
 *               the table, the highest one on a clash -- over the table as the
 *               earlier blocks' searches left it.  A candidate may lie in any
 *               earlier block and an offset may reach n - 1; a match never
 *               passes the end of its own block, its source may run across a
 *               block boundary.  A searched block's positions enter the table
 *               whether it is written Compressed or Raw; an empty block or a
 *               block of one repeated byte is not searched and inserts
 *               nothing.  The repeat-offset history rule is unchanged.
 * The contract is the full format's whole.  The scratch grows by the tables,
 * 64 KiB per resident workgroup (at most 1,792): 576 KiB instead of 512 KiB
 * per frame of a batch, at most 1,008 MiB instead of 896 MiB; a @d_scratch
 * below zsk_zstd_compress_scratch_size_ex(.., ZSK_ZSTD_FORMAT_FULL_WIDE), or
 * one that is not 16-byte aligned, returns -1.  The subset's and the full
 * format's sizes are what they were.  Formats 2, 3 and 4 stay unknown.
 */
#define ZSK_ZSTD_FORMAT_SUBSET 0   /* zsk_zstd_compress_frames' frames, byte for byte */
#define ZSK_ZSTD_FORMAT_FULL   1
#define ZSK_ZSTD_FORMAT_FULL_WIDE 5   /* the full format over the frame-wide match search */
ZSEEK_EXPORT size_t zsk_zstd_compress_scratch_size_ex(uint32_t nframes, uint64_t src_bytes, int format);
ZSEEK_EXPORT int zsk_zstd_compress_frames_ex(const zsk_compress_desc_t *d_desc,
    uint32_t nframes, const void *d_src, void *d_dst, uint32_t *d_csize,
    void *d_scratch, size_t scratch_size, void *stream, int format);

/*
 * Writer GPU mode: an LZ4 writer's frames of <= 4 MiB are compressed on the
 * GPU (zsk_lz4_compress_frames, on the calling thread's current device) in
 * batches of @batch_bytes input bytes (0: 1 GiB; (size_t)-1: GPU mode off,
 * after writing what is queued).  The file is byte-identical to host
 * compression.  Frames are written and logged when their batch is compressed:
 * when it fills, when a frame the GPU does not take (> 4 MiB) arrives, at
 * zseek_writer_stats and at zseek_writer_close; each write callback gets the
 * call_data of the zseek_write that produced the frame.  Deferred writes:
 * zseek_write returns true once its frame is QUEUED, so a compression or
 * write-callback failure of a queued frame is reported by the later call
 * that flushes (zseek_write, zseek_writer_stats or zseek_writer_close), not
 * by the zseek_write that queued it, and the writer then stays failed: every
 * later call, close included, returns false.  Staging is allocated at the
 * first queued frame and grows with the queue; frames per batch are capped
 * so the compressor's scratch (64 KiB per frame) stays within @batch_bytes.
 * Env ZSEEK_GPU_COMPRESS=1
 * (or a batch size in bytes) at open turns it on.  false for NULL, a zstd
 * writer, an HC level (>= 3) or no HIP device.
 */
ZSEEK_EXPORT bool zsk_writer_set_gpu_compress(zseek_writer_t *writer, size_t batch_bytes);

/* Make the file's seek table carry per-frame checksums (descriptor bit 7,
 * 12-byte entries cSize, dSize, checksum: seek_table.c:374-407 of the
 * reference).  Only before anything has been written: false once a frame
 * has been logged or queued or bytes are buffered (and for NULL).  Setting
 * the value it already has returns true.  Env ZSEEK_WRITE_CHECKSUMS=1 at
 * open.  Default off: files are then byte for byte what they are without
 * this call.  Frames compressed on the host are hashed there; a GPU-mode
 * batch is hashed on the GPU, on the compression's stream.  With checksums
 * on, zseek_writer_stats counts 12 bytes per frame in seek_table_size and
 * compressed_size (the reference's stats always assume 8). */
ZSEEK_EXPORT bool zsk_writer_set_checksums(zseek_writer_t *writer, bool on);

/* The bytes d_buf[0, len) (device memory of the writer's GPU-mode device, or
 * of the calling thread's current device when GPU mode is off) written as if
 * they were host memory and the caller had run
 *     for (o = 0; o < len; o += write_size)
 *         if (!zseek_write(w, host + o, min(write_size, len - o), call_data, errbuf)) return false;
 * (write_size 0: one write of len; len 0: one empty write).  The file, the
 * frames, each write callback's bytes and call_data, and the stats afterwards
 * are exactly that loop's.  Synchronous: the call returns with nothing queued
 * (it flushes what earlier zseek_write calls queued, in order, then its own
 * frames), so a compression or callback failure of its frames is reported by
 * this call; d_buf may be reused on return.  The bytes must be complete when
 * the call is made (the work that produced them synchronized).
 * In GPU mode, with nothing buffered and min_frame_size <= write_size <=
 * 4 MiB, the pieces are compressed (and hashed) where they are and only
 * compressed frames cross to the host; every other case (zstd, GPU mode off,
 * other piece sizes, bytes already buffered) downloads the pieces and takes
 * zseek_write's path.
 * false + errbuf for a NULL writer ("invalid writer"), a pointer that is not
 * device memory of that device ("write from device: not device memory of the
 * writer's device"), and everything zseek_write fails on. */
ZSEEK_EXPORT bool zsk_write_device(zseek_writer_t *writer, const void *d_buf, size_t len,
    size_t write_size, void *call_data, char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * A reader over a complete seekable file (LZ4 or zstd frames plus seek
 * table) that is already in device memory: @d_image[0, size), any alignment.
 * The reader does not own the image; it must stay valid and unmodified until
 * zseek_reader_close.  The reader's device is the one the pointer belongs to.
 *
 * Open downloads the file's tail, parses it with the same code as
 * zseek_reader_open_full (a bad file gives the same NULL and errbuf text as
 * a host copy of the bytes) and uploads the seek table once (prefix sums and,
 * when the file carries them, checksums; counted in
 * zsk_gpu_stats_t.device_memory).  NULL + errbuf also for no HIP device ("no
 * HIP device available") and a pointer that is not device memory ("open
 * device image: not device memory").
 *
 * Every read call (zseek_pread, zseek_read, zsk_pread_device, zsk_preadv,
 * zsk_preadv_device) behaves as on a reader opened over a host copy of the
 * image -- return values, bytes, errbuf, cache, partial-read rules,
 * zsk_reader_set_verify_checksums -- but no compressed byte is staged or
 * uploaded: the decode kernels read the frames in place, and
 * zsk_gpu_stats_t.bytes_uploaded stays 0.  A contiguous read's descriptors
 * are written on the device from the resident table; a vectored batch uploads
 * only its descriptors, segments and their prefix sum.  zstd reads of <= 64
 * frames plan on the device (one stream synchronization more than on a host
 * image).  A vectored batch is also cut where the compressed distance between
 * its first and last touched frame would pass 4 x zsk_reader_set_batch_bytes
 * (256 MiB by default): the LZ4 parse scratch of a batch decoded in place
 * grows with that distance, and the parse kernels address a wave's frames
 * through one 32-bit buffer resource (with batch_bytes of 512 MiB or more a
 * batch spanning 2 GiB fails the call: "vectored read: a batch spans 2 GiB of
 * the device image").
 *
 * What must be readable around the image: the kernels load whole aligned
 * words, so they may read the bytes between the 32-byte boundary below
 * @d_image and @d_image, and up to the 4-byte boundary past a frame's end --
 * for the last frame that lies inside the seek table (>= 17 bytes) that
 * follows it.  Nothing at or past @d_image + size is read by a kernel: any
 * allocation's own rounding covers the low end, the file itself the high.
 * Open only sums the seek table's entries, so a corrupt table can put frames
 * past the end of the file: a read whose compressed span is not inside
 * [0, size) fails with "unexpected EOF" before any kernel runs, where the
 * pread callback of a host copy comes back short (a span that ends exactly at
 * @size may be read up to the 4-byte boundary after it).
 *
 * One lane: zsk_reader_set_devices returns true only for exactly that one
 * device (and changes nothing), zsk_reader_devices reports it from open on,
 * zsk_reader_set_io_threads is accepted and has no effect.
 */
ZSEEK_EXPORT zseek_reader_t *zsk_reader_open_device(const void *d_image, size_t size,
    size_t cache_size, char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * A complete seekable LZ4 file built in device memory.  The call leaves in
 * @d_image[0, returned size) the bytes this sequence writes: a writer opened
 * with {ZSEEK_LZ4, @level} and min_frame_size = @frame_size,
 * zsk_writer_set_checksums(@flags & ZSK_IMAGE_CHECKSUMS),
 * zsk_write_device(w, d_src, len, frame_size, ...), zseek_writer_close --
 * direct frames of @frame_size bytes, a shorter last piece as the buffered
 * frame with its content-size header, then the seek table (8-byte entries, 12
 * with checksums); len == 0 gives the empty table alone.  No frame byte, slot
 * or per-frame size crosses to the host: frames are compressed from @d_src in
 * batches of at most @batch_bytes input bytes (0: 256 MiB, 1 GiB for frames
 * above 64 KiB, as zsk_write_device; at least one frame) into pooled slots,
 * packed into the image by zsk_gather_segments' kernel at offsets scanned on
 * the device, and the table is written there too.  Synchronous (one host
 * synchronization, at the end); @d_src and @d_image (any alignment) are
 * memory of one device and must not overlap.  The bytes of @d_src must be
 * complete when the call is made (their producer synchronized), as for
 * zsk_write_device.  The scratch (a batch's slots at their bound, 64 KiB of
 * compressor tables per batch frame, 12 bytes per frame of the file) is
 * sized by the largest call so far and stays allocated for the life of the
 * process, one set per device (up to four under concurrent calls): about
 * 0.5 GiB after a default call on 64 KiB frames, 1.1 GiB on frames above;
 * pass a smaller @batch_bytes to hold less.
 *
 * zsk_lz4_image_bound(len, frame_size, flags): the capacity the call asks
 * for -- every frame at its ZSK_LZ4_COMPRESS_BOUND, plus the table
 * (17 + 8 or 12 bytes per frame); 0 for frame_size == 0.
 *
 * Returns the file's size, or -1 + errbuf for frame_size == 0 or above
 * ZSK_LZ4_COMPRESS_MAX_FRAME, level >= 3, more frames than a seek table
 * holds, pointers that are not device memory of one device, @capacity below
 * the bound ("build image: buffer too small", checked before anything is
 * written) and a HIP failure.  Nothing at or past @d_image + @capacity is ever
 * written; bytes between the returned size and @capacity are unspecified.
 *
 * Concurrent calls: the scratch is a pool of at most four sets per device,
 * one pool for this entry point and zsk_zstd_build_image, a set held from the
 * call's start to its end and reused in stream order (see
 * zsk_lz4_decode_frames).  A fifth call in progress at once on a device gets
 * -1 + "build image: scratch allocation failed" with nothing queued and
 * @d_image untouched.
 */
#define ZSK_IMAGE_CHECKSUMS 1u
ZSEEK_EXPORT size_t zsk_lz4_image_bound(size_t len, size_t frame_size, unsigned flags);
ZSEEK_EXPORT ssize_t zsk_lz4_build_image(const void *d_src, size_t len, size_t frame_size,
    int level, unsigned flags, size_t batch_bytes, void *d_image, size_t capacity,
    char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * zsk_lz4_build_image for zstd: a complete seekable zstd file built in device
 * memory from zsk_zstd_compress_frames' frames (the subset described there) by
 * the same machinery -- pooled slots at ZSK_ZSTD_COMPRESS_BOUND, sizes scanned
 * and frames packed on the device, the table written there, one host
 * synchronization at the end.  Frames hold @frame_size bytes (at most
 * ZSK_ZSTD_COMPRESS_MAX_FRAME), the last one the rest; len == 0 gives the
 * empty table alone.  ZSK_IMAGE_CHECKSUMS: 12-byte table entries;
 * ZSK_IMAGE_CONTENT_CHECKSUMS: the same XXH64 word (computed once) also ends
 * each frame.  ZSK_IMAGE_ZSTD_FULL: the frames in ZSK_ZSTD_FORMAT_FULL (the
 * bounds and the scratch are the same; zsk_lz4_build_image ignores the bit).
 * ZSK_IMAGE_ZSTD_WIDE: the frames in ZSK_ZSTD_FORMAT_FULL_WIDE, with or
 * without ZSK_IMAGE_ZSTD_FULL, which it implies (the bounds are the same, the
 * scratch grows by the search's tables; zsk_lz4_build_image ignores the bit).
 * @batch_bytes 0: 256 MiB.  zsk_zstd_image_bound: every frame at
 * its bound plus the table; 0 for frame_size == 0.  Errors are
 * zsk_lz4_build_image's, under the same conditions (there is no level).  The
 * result is read as zstd by the reference reader and zsk_reader_open_device.
 * The pooled scratch is zsk_lz4_build_image's with the zstd compressor's in
 * place of the LZ4 tables: 512 KiB per frame of a batch, at most 896 MiB;
 * with ZSK_IMAGE_ZSTD_WIDE 576 KiB per frame of a batch, at most 1,008 MiB.
 * Its bound is zsk_lz4_build_image's too: four calls of the two entry points
 * in progress at once per device, a fifth gets -1 with nothing queued.
 */
#define ZSK_IMAGE_CONTENT_CHECKSUMS 2u
#define ZSK_IMAGE_ZSTD_FULL 4u     /* zsk_zstd_build_image: frames in the full format */
#define ZSK_IMAGE_ZSTD_WIDE 8u     /* zsk_zstd_build_image: the full format over the wide match search */
ZSEEK_EXPORT size_t zsk_zstd_image_bound(size_t len, size_t frame_size, unsigned flags);
ZSEEK_EXPORT ssize_t zsk_zstd_build_image(const void *d_src, size_t len, size_t frame_size,
    unsigned flags, size_t batch_bytes, void *d_image, size_t capacity,
    char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * zsk_lz4_build_image / zsk_zstd_build_image queued on the caller's stream,
 * optionally with one frame per PIECE of a list that is in device memory.
 *
 * Stream order: everything is queued on @stream (a hipStream_t of the image's
 * device; NULL = HIP's null stream, as in zsk_preadv_device_async), after what
 * the stream already holds and before what is queued later -- work already on
 * the stream may have written @d_src and @d_sizes.  The call returns 0 once
 * everything is queued and makes no host wait for its own work.  The one thing
 * that can make it wait: growing the pooled scratch (the first call, or a call
 * that needs more than any before: hipFree waits for the device; the scratch
 * is the synchronous builders', sized by @max_piece as they size it by
 * frame_size).
 *
 * @d_result: three int64_t of device memory, written when the stream reaches
 * the end of the call's work: [0] the file's size, or ZSK_IMAGE_FAILED (a frame
 * was refused by the compressor, or a HIP failure after something was queued)
 * or ZSK_IMAGE_BAD_PIECES; [1] the frames in the table; [2] the source bytes
 * consumed.  Whatever is queued behind the call -- a copy of the result, a
 * kernel that reads the table -- sees all three and the image.
 *
 * @d_sizes != NULL, a build from pieces: piece i is d_sizes[i] bytes of @d_src
 * right after piece i - 1, and becomes frame i; frame index = piece index.
 * LZ4: the image is byte for byte the file of a host writer opened with
 * {ZSEEK_LZ4, @level} and min_frame_size = 1,
 * zsk_writer_set_checksums(@flags & ZSK_IMAGE_CHECKSUMS), one zseek_write per
 * piece, zseek_writer_close: every frame a direct frame without a content-size
 * field, pieces above 64 KiB as linked 64 KiB blocks.  zstd: frame i is the
 * frame zsk_zstd_compress_frames_ex writes for the piece's bytes in the format
 * the flags select (the subset, ZSK_IMAGE_ZSTD_FULL, ZSK_IMAGE_ZSTD_WIDE);
 * ZSK_IMAGE_CONTENT_CHECKSUMS as in zsk_zstd_build_image.  npieces == 0 gives
 * the empty table alone (17 bytes).
 * The list is data, not trusted input.  It is invalid when some size is 0,
 * some size exceeds @max_piece, or the sizes sum to more than @src_len:
 * d_result[0] is then ZSK_IMAGE_BAD_PIECES, no byte outside
 * d_src[0, src_len) is read and none outside d_image[0, capacity) written
 * (bytes inside the capacity are unspecified, [1] and [2] too), and the next
 * call builds normally.  A sum below @src_len is valid: the rest of the source
 * is ignored, and [2] says how much was used.
 *
 * @d_sizes == NULL, the fixed-frame build: pieces of @max_piece bytes, the
 * last one the rest of @src_len; @npieces must be ceil(src_len / max_piece)
 * ("build image: invalid piece count").  The image is exactly
 * zsk_lz4_build_image's / zsk_zstd_build_image's for frame_size = max_piece,
 * LZ4's content-size header on a short tail included.
 *
 * Batches hold min(@batch_bytes / @max_piece, the synchronous builders' frame
 * caps, @npieces) pieces (at least one; @batch_bytes 0: their defaults), in
 * slots of the bound of @max_piece; a batch of a build from pieces costs one
 * more one-workgroup kernel (the scan and check of its sizes).
 *
 * zsk_lz4_pieces_bound / zsk_zstd_pieces_bound(src_len, npieces, flags): the
 * capacity the call asks for, computable on the host without the sizes: at
 * least the sum of ZSK_*_COMPRESS_BOUND over ANY npieces sizes that sum to at
 * most src_len, plus the table --
 *   LZ4   src_len + 4 * (src_len >> 16) + 39 * npieces + 17 + (8 | 12) * npieces
 *   zstd  src_len + 3 * (src_len >> 17) + 31 * npieces + 17 + (8 | 12) * npieces
 * (csrc/image_pieces.h derives them).  On a fixed-frame list it exceeds
 * zsk_*_image_bound by at most 19 (LZ4) or 18 (zstd) bytes per piece.
 *
 * -1 + errbuf with nothing queued and @d_image untouched: a capturing stream
 * ("build image: stream is capturing" -- pooled scratch must never end up in a
 * graph); NULL @d_result ("build image: NULL result"); @max_piece 0 or above
 * the codec's cap of 4 MiB ("build image: invalid piece size"); level >= 3;
 * more pieces than a seek table holds; no HIP device ("no HIP device
 * available"); @d_image, @d_result, @d_sizes when not NULL and @d_src when
 * src_len > 0 not device memory of one device ("build image: not device memory
 * of one device"), or @d_sizes / @d_result not aligned to their words;
 * @capacity below the bound ("build image: buffer too small"); a fifth call of
 * the four builder entry points in progress at once on a device (one pool, see
 * zsk_lz4_build_image).  A HIP failure after something was queued queues a fill
 * of d_result[0..2] with -1 and returns -1.
 * Left out: graph capture, zero-length pieces, sources in host memory, pieces
 * on another device than the image.
 */
#define ZSK_IMAGE_FAILED     (-1)
#define ZSK_IMAGE_BAD_PIECES (-2)
ZSEEK_EXPORT size_t zsk_lz4_pieces_bound(size_t src_len, size_t npieces, unsigned flags);
ZSEEK_EXPORT size_t zsk_zstd_pieces_bound(size_t src_len, size_t npieces, unsigned flags);
ZSEEK_EXPORT int zsk_lz4_build_image_pieces(const void *d_src, size_t src_len,
    const uint32_t *d_sizes, size_t npieces, size_t max_piece, int level, unsigned flags,
    size_t batch_bytes, void *d_image, size_t capacity, int64_t *d_result, void *stream,
    char errbuf[ZSEEK_ERRBUF_SIZE]);
ZSEEK_EXPORT int zsk_zstd_build_image_pieces(const void *d_src, size_t src_len,
    const uint32_t *d_sizes, size_t npieces, size_t max_piece, unsigned flags,
    size_t batch_bytes, void *d_image, size_t capacity, int64_t *d_result, void *stream,
    char errbuf[ZSEEK_ERRBUF_SIZE]);

/*
 * Appending frames to a seekable file that is in device memory: a build from
 * pieces behind the file's last frame, queued on the caller's stream.
 *
 * @d_src, @src_len, @d_sizes, @npieces, @max_piece, @level, @flags,
 * @batch_bytes, @d_result, @stream: as in zsk_*_build_image_pieces -- the list
 * is data, an invalid one answers ZSK_IMAGE_BAD_PIECES, the zstd format flags
 * and the checksum flags mean the same, nothing waits on the host -- except
 * that @d_sizes is required (a fixed-frame caller passes a list of equal
 * sizes; "append image: needs a piece list") and @npieces == 0 is valid.
 * @d_image[0, capacity): holds a seekable file of the same codec, at any byte
 * alignment.  @d_prev: two int64_t of device memory, 8-byte aligned, read ON
 * THE STREAM: [0] the existing file's size, [1] its frame count -- the layout
 * of a builder's d_result, so that an append can be queued directly behind the
 * build or the append that produced the image, without the host looking.
 * @d_prev == @d_result is allowed: the words are read before anything of the
 * call writes them.  @prev_frames: the host's statement of the frame count
 * (always known to it: every builder takes npieces from the host); it sizes
 * the scratch that holds the table's entries, 8 or 12 bytes per frame.
 *
 * Success, when the stream reaches the end of the call's work:
 * d_image[0, new size) holds the old frames' bytes untouched, the new frames
 * packed behind them from the old table's position on, and a seek table over
 * @prev_frames + @npieces entries; d_result = {new size, prev_frames + npieces,
 * source bytes consumed}.  Frames are independent and the table is a function
 * of the frames' sizes, so the file is byte for byte the one that a single
 * zsk_*_build_image_pieces call over the old pieces followed by the new ones
 * writes (LZ4: the host writer's file for one zseek_write per piece).
 * @npieces == 0 rewrites the same table and answers the old size.
 *
 * @d_prev and the image are data, not trusted input, and no byte at or past
 * d_image + capacity is read or written whatever they hold.  The file is
 * accepted when d_prev[1] == prev_frames; table bytes of prev_frames entries
 * <= d_prev[0] <= capacity (checked first, before any read of the table); the
 * table's footer has the seek magic, no reserved descriptor bit, the frame
 * count prev_frames and a checksum bit equal to @flags & ZSK_IMAGE_CHECKSUMS;
 * the skippable header's magic and size field match; the entries' compressed
 * sizes sum to the table's offset; and, when prev_frames > 0, the file starts
 * with the codec's frame magic (what zseek_reader_open tells the codecs apart
 * by).  Otherwise d_result[0] = ZSK_IMAGE_BAD_IMAGE and no byte of @d_image is
 * written.  An accepted file for which zsk_*_append_bound(its size, ...)
 * exceeds @capacity answers ZSK_IMAGE_NO_ROOM, nothing written either.
 *
 * A failure found after the old table was overwritten -- an invalid piece list
 * in any batch (ZSK_IMAGE_BAD_PIECES), a frame the compressor refused
 * (ZSK_IMAGE_FAILED) -- ends with the old table written back, so
 * d_image[0, old size) is again the old file byte for byte; what lies between
 * that and @capacity is unspecified, and the next call works normally.  When
 * several apply the answer is, in this order, BAD_IMAGE, NO_ROOM, BAD_PIECES,
 * FAILED.  A failure code used as the next append's d_prev[0] fails that
 * call's size check: along a chain queued without looking, every call after a
 * failed one answers ZSK_IMAGE_BAD_IMAGE and touches nothing.
 *
 * zsk_lz4_append_bound / zsk_zstd_append_bound(prev_size, prev_frames, src_len,
 * npieces, flags): prev_size - table bytes(prev_frames) + the frames' part of
 * zsk_*_pieces_bound(src_len, npieces) + table bytes(prev_frames + npieces);
 * 0 when prev_size is below the table bytes of prev_frames.  Monotone in
 * prev_size: a caller who knows only a bound on the old size allocates by it.
 *
 * -1 + errbuf with nothing queued and @d_image untouched, every argument check
 * before the device is asked for: a capturing stream ("append image: stream is
 * capturing"); NULL @d_result, @d_prev or @d_sizes; @max_piece 0 or above the
 * codec's cap; level >= 3; prev_frames + npieces above the seek table's 2^27
 * frames; @d_result or @d_prev not 8-byte, @d_sizes not 4-byte aligned;
 * @capacity below zsk_*_append_bound(table bytes(prev_frames), prev_frames,
 * ...), the smallest file that could be there ("append image: buffer too
 * small"); no HIP device; a pointer that is not device memory of the image's
 * device; a fifth builder or append call in progress at once on the device
 * (the builders' pool).  A HIP failure after something was queued queues a fill
 * of d_result[0..2] with -1 and returns -1; the old frames' bytes are then
 * intact and what lies behind them is unspecified.
 *
 * A reader's contract is that its image does not change while it is open:
 * close the readers on an image before appending to it and open a new reader
 * afterwards.
 * Left out: removing or replacing frames, selecting frames into a new image,
 * an image on another device than the source, graph capture, refreshing an
 * open reader, a fixed-frame mode without a list.
 */
#define ZSK_IMAGE_BAD_IMAGE (-3)  /* d_prev / prev_frames do not describe a valid file in d_image */
#define ZSK_IMAGE_NO_ROOM   (-4)  /* the appended file might not fit capacity */
ZSEEK_EXPORT size_t zsk_lz4_append_bound(size_t prev_size, size_t prev_frames, size_t src_len,
    size_t npieces, unsigned flags);
ZSEEK_EXPORT size_t zsk_zstd_append_bound(size_t prev_size, size_t prev_frames, size_t src_len,
    size_t npieces, unsigned flags);
ZSEEK_EXPORT int zsk_lz4_append_image_pieces(const void *d_src, size_t src_len,
    const uint32_t *d_sizes, size_t npieces, size_t max_piece, int level, unsigned flags,
    size_t batch_bytes, void *d_image, size_t capacity, const int64_t *d_prev, size_t prev_frames,
    int64_t *d_result, void *stream, char errbuf[ZSEEK_ERRBUF_SIZE]);
ZSEEK_EXPORT int zsk_zstd_append_image_pieces(const void *d_src, size_t src_len,
    const uint32_t *d_sizes, size_t npieces, size_t max_piece, unsigned flags,
    size_t batch_bytes, void *d_image, size_t capacity, const int64_t *d_prev, size_t prev_frames,
    int64_t *d_result, void *stream, char errbuf[ZSEEK_ERRBUF_SIZE]);

#ifdef __cplusplus
}
#endif

#endif /* ZSEEK_HIP_H */
