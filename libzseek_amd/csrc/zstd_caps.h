// zstd_caps.h — the scratch capacities of the asynchronous zstd decode
// (zsk_zstd_decode_frames_async): the host cannot wait for the plan's totals
// there, so it sizes the scratch from bounds the caller states and the device
// checks its own plan against them (zstd_fit_kernel, zstd_plan.hip); and the
// bounds a device-planned read takes from a file's census.  No HIP types:
// tests/native/zstd_caps_shim.cpp and zstd_census_shim.cpp drive it.
//
// What the default bounds (zstd_bounds_default) cost in device memory: 2 items
// of 8 bytes per sequence at out_bytes / 3 sequences, plus their padding, is
// about 5.4 bytes of items per output byte; a block slot, its four Huffman
// jobs and its four ops are about 11 KiB (kZSlot + 4 * 32 + 4 * 32 + 16), at
// one block per 16 KiB of output plus two per entry; the literal scratch is
// out_bytes + 64.  A caller who knows its files states tighter bounds.
#pragma once

#include <stdint.h>

namespace zsk {

// Item slots that cover the sum of zstd_frame_plan().bound over any batch of
// nframes entries with at most max_blocks block headers and max_sequences
// sequences together.  Per entry (zstd_plan.h): 8, rounded up to 4 at the end
// (<= 3 more, everything else being even or a multiple of 4 does not matter:
// 11 covers it); 4 per block; per block with n sequences 2 n + ceil(2 n / 63)
// <= 2 n + 2 n / 63 + 1, and only blocks with a sequence pay the + 1: over
// the batch 2 S + floor(2 S / 63) + min(B, S).
inline uint64_t zstd_item_capacity(uint32_t nframes, uint64_t max_blocks, uint64_t max_sequences)
{
    constexpr uint64_t kHuge = 1ull << 58;   // past any device's memory: no wrap below
    if (max_blocks >= kHuge || max_sequences >= kHuge)
        return ~0ull;
    const uint64_t pads = 2 * max_sequences / 63 + (max_blocks < max_sequences ? max_blocks : max_sequences);
    return 11ull * nframes + 4 * max_blocks + 2 * max_sequences + pads;
}

// The default bounds of a call that decodes nframes entries into out_bytes: a
// policy, not a guarantee.  A zstd match is at least 3 bytes, so no entry that
// decodes within out_bytes declares more than out_bytes / 3 sequences that
// all execute; libzstd and this project's compressor write 128 KiB blocks, so
// one block per 16 KiB is 8x their rate, plus two per entry (a short last
// block, an empty frame's).
inline void zstd_bounds_default(uint32_t nframes, uint64_t out_bytes, uint64_t *max_blocks, uint64_t *max_sequences)
{
    *max_sequences = out_bytes / 3;
    *max_blocks = 2ull * nframes + out_bytes / 16384;
}

// The bounds of a call that decodes any max_frames entries of one file, from
// the file's census (zsk_reader_zstd_census: the most block headers and the
// most declared sequences any one entry has, the largest decoded size): a
// guarantee while the file's bytes stay what the census walked.  Every entry
// has at most census_blocks blocks and census_sequences sequences, so
// max_frames of them have at most the products, and zstd_item_capacity
// (max_frames, products) covers the sum of their plan bounds; an entry of no
// bytes (a padding descriptor) walks to a bound of 8 with no block and no
// sequence, inside the 11 per entry.  A product past 64 bits saturates (no
// device holds such a scratch: the caller refuses it).
inline void zstd_census_bounds(uint64_t max_frames, uint64_t census_blocks, uint64_t census_sequences,
                               uint32_t max_dsize, uint64_t *out_bytes, uint64_t *max_blocks,
                               uint64_t *max_sequences)
{
    const auto times = [](uint64_t a, uint64_t b) { return a && b > ~0ull / a ? ~0ull : a * b; };
    *out_bytes = times(max_frames, max_dsize);
    *max_blocks = times(max_frames, census_blocks);
    *max_sequences = times(max_frames, census_sequences);
}

}   // namespace zsk
