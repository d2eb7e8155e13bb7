// Test-only C shim over libzseek_amd/csrc/zstd_plan.h (the zstd decoder's
// plan walk: pure, no HIP): tests/test_zstd_plan.py builds it with g++ and
// calls it via ctypes.  With -DZSTD_PLAN_MAIN it is a stand-alone program
// (built with -fsanitize=address,undefined) that walks a dump of entries, each
// from a heap buffer of exactly its length, whole and cut short.
#include "../../libzseek_amd/csrc/zstd_plan.h"

extern "C" {

// out: bound, blocks, cks
void zp_frame_plan(const uint8_t *p, uint32_t len, uint32_t *out)
{
    const zsk::ZstdFramePlan P =
        zsk::zstd_frame_plan([=](uint32_t i) -> uint32_t { return i < len ? (uint32_t)p[i] : 0u; }, len);
    out[0] = P.bound;
    out[1] = P.blocks;
    out[2] = P.cks ? 1u : 0u;
}
}

#ifdef ZSTD_PLAN_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

// argv[1]: a dump of entries, each a little-endian u32 length and its bytes.
// Prints "bound blocks cks" per entry (the whole entry only).
int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    std::vector<uint8_t> all;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;)
        all.insert(all.end(), buf, buf + n);
    fclose(f);
    for (size_t at = 0; at + 4 <= all.size();) {
        uint32_t len;
        memcpy(&len, &all[at], 4);
        at += 4;
        if (at + len > all.size())
            return 3;
        const uint32_t cuts[] = {len, 0, 1, 8, 9, len ? len - 1 : 0};
        for (size_t k = 0; k < sizeof(cuts) / sizeof(cuts[0]); k++) {
            const uint32_t n = cuts[k] < len ? cuts[k] : len;
            uint8_t *p = (uint8_t *)malloc(n ? n : 1);   // exactly the cut: a read past it is a heap overflow
            if (n)
                memcpy(p, &all[at], n);
            uint32_t out[3];
            zp_frame_plan(n ? p : p + 1, n, out);        // (n == 0: not even p[0] may be read)
            if (k == 0)
                printf("%u %u %u\n", out[0], out[1], out[2]);
            free(p);
        }
        at += len;
    }
    return 0;
}
#endif
