// Test-only C shim over libzseek_amd/csrc/batch_layout.h (pure arithmetic, no
// HIP): tests/test_batch_layout.py builds it with g++ and calls it via ctypes.
#include "../../libzseek_amd/csrc/batch_layout.h"

using namespace zsk;

extern "C" {

// out: doff, poff, goff, coff, up
void bl_contiguous(uint64_t csz, size_t n, int image, int plan, uint64_t *out)
{
    const BatchLayout L = contiguous_layout(csz, n, image != 0, plan != 0);
    const uint64_t v[5] = {L.doff, L.poff, L.goff, L.coff, L.up};
    for (int i = 0; i < 5; i++)
        out[i] = v[i];
}

uint64_t bl_pack_at(uint64_t d_bytes) { return gather_pack_at(d_bytes); }

void bl_vectored(uint64_t csz, size_t n, size_t nseg, int image, int plan, uint64_t *out)
{
    const BatchLayout L = vectored_layout(csz, n, nseg, image != 0, plan != 0);
    const uint64_t v[5] = {L.doff, L.poff, L.goff, L.coff, L.up};
    for (int i = 0; i < 5; i++)
        out[i] = v[i];
}
}
