// zstd_enc_wide_dev.h — the wide match search of the GPU zstd compressor
// (ZSK_ZSTD_FORMAT_FULL_WIDE), beside zstd_enc_dev.h and zstd_enc_full_dev.h,
// which it includes and leaves as they are.  Host and device compile the same
// functions: the wide kernel of zstd_compress.hip calls them from lanes, and
// tests/native/zstd_enc_wide_shim.cpp restates the search serially on the CPU.
// Integer arithmetic only, so both give the same bytes.
//
// A wide frame is a full frame (zstd_enc_full_dev.h) in everything but the
// sequences handed to the format layer: header, 128 KiB blocks, block-type
// rule, literals, table modes, repeat offsets and their history, checksum are
// the full format's.
//   n <= kWideMinFrame (16384)
//           the full format's search, unchanged: kHashLog (12), a table
//           cleared for every block.  The frame is the full format's frame
//           byte for byte.
//   n >  kWideMinFrame
//           one table of 1 << kWideHashLog (2^14) entries for the whole frame,
//           position + 1 relative to the frame's start by wide_hash, 0: empty.
//           It is zeroed once, at the frame's start.  Block b's search is the
//           full format's -- 64 positions a step, the lowest lane whose
//           candidate's 4 bytes match wins, the match extends to the block's
//           own end at most, the step's positions below the next step's start
//           enter the table and the highest position wins a clash -- over the
//           table as the earlier blocks' searches left it.  So a candidate may
//           lie in any earlier block and an offset may reach n - 1; a match
//           never passes its own block's end, its source may cross a block
//           boundary.  A searched block's positions enter the table whether
//           the block is then written Compressed or Raw; an empty block and a
//           block of one repeated byte (written RLE without a search) insert
//           nothing.
// A candidate is a position entered earlier, so it lies below the current
// position and inside the frame: the table must hold nothing of another
// frame, which the clear at the frame's start sees to.
#pragma once

#include "zstd_enc_dev.h"
#include "zstd_enc_full_dev.h"

namespace zsk {
namespace zenc {

constexpr uint32_t kWideHashLog = 14;            // the frame-long table: 2^14 positions by 4-byte hash
constexpr uint32_t kWideMinFrame = 1u << 14;     // frames above this many bytes take the wide search
constexpr size_t kWideTableBytes = sizeof(uint32_t) << kWideHashLog;

static_assert(kMaxFrame + 1 != 0 && kWideHashLog > kHashLog, "positions + 1 fit a table entry");

// Whether a frame of n bytes is searched with the frame-long table.
ZENC_HD bool wide_frame(uint32_t n)
{
    return n > kWideMinFrame;
}

// The table index of the 4 bytes v: below 1 << kWideHashLog by construction.
ZENC_HD uint32_t wide_hash(uint32_t v)
{
    return (v * 2654435761u) >> (32 - kWideHashLog);
}

}   // namespace zenc
}   // namespace zsk
