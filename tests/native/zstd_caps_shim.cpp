// Test-only C shim over libzseek_amd/csrc/zstd_caps.h (the asynchronous zstd
// decode's capacity arithmetic and default bounds: pure, no HIP) and the plan
// walk of zstd_plan.h with its sequence count: tests/test_zstd_caps.py builds
// it with g++ and calls it via ctypes.
#include "../../libzseek_amd/csrc/zstd_caps.h"
#include "../../libzseek_amd/csrc/zstd_plan.h"

extern "C" {

uint64_t zcaps_item_capacity(uint32_t nframes, uint64_t max_blocks, uint64_t max_sequences)
{
    return zsk::zstd_item_capacity(nframes, max_blocks, max_sequences);
}

// out: max_blocks, max_sequences
void zcaps_bounds_default(uint32_t nframes, uint64_t out_bytes, uint64_t *out)
{
    zsk::zstd_bounds_default(nframes, out_bytes, &out[0], &out[1]);
}

// out: bound, blocks, cks, sequences
void zcaps_frame_plan(const uint8_t *p, uint32_t len, uint64_t *out)
{
    const zsk::ZstdFramePlan P =
        zsk::zstd_frame_plan([=](uint32_t i) -> uint32_t { return i < len ? (uint32_t)p[i] : 0u; }, len);
    out[0] = P.bound;
    out[1] = P.blocks;
    out[2] = P.cks ? 1u : 0u;
    out[3] = P.sequences;
}
}
