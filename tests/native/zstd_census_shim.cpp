// Test-only C shim over the census arithmetic of libzseek_amd/csrc/zstd_caps.h
// (zstd_census_bounds, with the item capacity and the default policy it is
// compared to: pure, no HIP) and the plan walk of zstd_plan.h, the one walk
// the census kernel runs per entry: tests/zstd_census_util.py builds it with
// g++ and calls it via ctypes.
#include "../../libzseek_amd/csrc/zstd_caps.h"
#include "../../libzseek_amd/csrc/zstd_plan.h"

extern "C" {

// out: out_bytes, max_blocks, max_sequences
void zcensus_bounds(uint64_t max_frames, uint64_t census_blocks, uint64_t census_sequences, uint32_t max_dsize,
                    uint64_t *out)
{
    zsk::zstd_census_bounds(max_frames, census_blocks, census_sequences, max_dsize, &out[0], &out[1], &out[2]);
}

uint64_t zcensus_item_capacity(uint32_t nframes, uint64_t max_blocks, uint64_t max_sequences)
{
    return zsk::zstd_item_capacity(nframes, max_blocks, max_sequences);
}

// out: max_blocks, max_sequences
void zcensus_bounds_default(uint32_t nframes, uint64_t out_bytes, uint64_t *out)
{
    zsk::zstd_bounds_default(nframes, out_bytes, &out[0], &out[1]);
}

// out: bound, blocks, sequences
void zcensus_frame_plan(const uint8_t *p, uint32_t len, uint64_t *out)
{
    const zsk::ZstdFramePlan P =
        zsk::zstd_frame_plan([=](uint32_t i) -> uint32_t { return i < len ? (uint32_t)p[i] : 0u; }, len);
    out[0] = P.bound;
    out[1] = P.blocks;
    out[2] = P.sequences;
}
}
