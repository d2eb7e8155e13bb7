// zstd_internal.h — the zstd decoder's stages as launch_zstd_decode
// (zstd_decode.hip) strings them together: one launcher per kernel, each in
// the file that holds its kernel.  A launcher enqueues on the stream it is
// given and reports nothing: launch_zstd_decode reads hipGetLastError once.
#pragma once

#include <stdlib.h>
#include <string.h>

#include "zsk_internal.h"

namespace zsk {

// one decode call's device arrays (launch_zstd_decode's arguments)
struct ZstdCall {
    const FrameDesc *desc;
    const uint8_t *comp;
    int32_t *status;
    uint32_t *fail_at;   // optional
    // the asynchronous decode (zstd_decode_frames_async): the device word that
    // is nonzero when the batch did not fit the call's bounds -- every stage
    // then returns at its top.  Null: the host sized the scratch from the plan
    const uint64_t *fit = nullptr;
};

// a chunk of the call: frames [f0, f1) and their block slots [b0, b1)
struct ZstdChunk {
    uint32_t c;   // its index (events, diagnostics)
    uint32_t f0, f1;
    uint64_t b0, b1;
    // the asynchronous decode: the host has no plan totals, [b0, b1) is [0,
    // the call's block capacity) and sizes the Huffman grids; the kernels take
    // the chunk's true range from these two device words (d_total[4 + c])
    const uint64_t *dev = nullptr;
};

// chunks a decode of n frames runs in (zstd_decode.hip)
uint32_t zstd_chunks(uint32_t n);

// true when the environment switch `name` is set to "0" (the switches that
// are on by default and "=0" turns off)
inline bool env_is_zero(const char *name)
{
    const char *v = getenv(name);
    return v && !strcmp(v, "0");
}

// zstd_frame.hip.  help: the one-frame route's shape, a workgroup per frame
// whose second wave decodes the Huffman descriptions (env ZSEEK_FRAME_HELP=0:
// off)
void launch_zstd_frame(const ZstdCall &C, ZstdScratch *s, const ZstdChunk &c, bool help, hipStream_t stream);
// zstd_huf_seq.hip.  The chunk's Huffman streams (b1 > b0; one: a workgroup
// per stream)
void launch_zstd_huf(const ZstdCall &C, ZstdScratch *s, const ZstdChunk &c, bool one, hipStream_t stream);
// ... the sequence replay (one: a wave per frame); the one-frame route's
// replay, Huffman streams and literal fix-up in one launch; the
// literal fix-up that joins the Huffman and sequence kernels
void launch_zstd_seq(const ZstdCall &C, ZstdScratch *s, const ZstdChunk &c, bool one, hipStream_t stream);
void launch_zstd_one(const ZstdCall &C, ZstdScratch *s, const ZstdChunk &c, hipStream_t stream);
void launch_zstd_lit_fix(const ZstdCall &C, ZstdScratch *s, const ZstdChunk &c, hipStream_t stream);
// tuning builds, ZSEEK_SEQ_TIMERS: the one-frame replay's cycle counters (else nothing)
void zstd_seq_timers(hipStream_t stream);

}   // namespace zsk
