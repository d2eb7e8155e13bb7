// Where the pieces of a batch's pinned upload lie: one buffer, one upload.
// No HIP and no reader state, so tests/native/batch_layout_shim.cpp checks the
// arithmetic on the CPU; reader.cpp's submit, reader_vec.cpp's submit_gather
// and the pre-growing of an asynchronous call's slots use exactly this.
//
//   [0, doff)     the compressed frames, back to back, and 256 bytes of slack
//                 that the parse kernels may read past the last frame; nothing
//                 for a file in device memory, whose frames stay where they are
//   [doff, poff)  one descriptor per frame (256-aligned)
//   [poff, goff)  the zstd host plan of a request's few frames, 2 (n + 1) u64
//   [goff, coff)  a vectored batch's gather segments
//   [coff, up)    ... and the nseg + 1 prefix sums of their lengths
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace zsk {

constexpr uint64_t kDescBytes = 24;   // sizeof(FrameDesc)
constexpr uint64_t kSegBytes = 24;    // sizeof(GatherSeg)

struct BatchLayout {
    uint64_t doff, poff, goff, coff, up;
};

// A contiguous batch (submit): no segment regions, up = the end of the plan.
inline BatchLayout contiguous_layout(uint64_t csz, size_t n, bool image, bool plan)
{
    BatchLayout L;
    L.doff = image ? 0 : (csz + 256 + 255) & ~255ull;
    L.poff = L.doff + n * kDescBytes;
    L.goff = L.coff = L.up = L.poff + (plan ? 16 * (uint64_t)(n + 1) : 0);
    return L;
}

// A vectored batch (submit_gather) of nseg segments.
inline BatchLayout vectored_layout(uint64_t csz, size_t n, size_t nseg, bool image, bool plan)
{
    BatchLayout L = contiguous_layout(csz, n, image, plan);
    L.coff = L.goff + nseg * kSegBytes;
    L.up = L.coff + (uint64_t)(nseg + 1) * sizeof(uint64_t);
    return L;
}

// A vectored batch's decoded staging (d_out): behind the d_bytes of its frames,
// 256-aligned, the segments compacted for a host destination.
inline uint64_t gather_pack_at(uint64_t d_bytes)
{
    return (d_bytes + 255) & ~255ull;
}

}   // namespace zsk
