// C entry points over libzseek_amd/csrc/xxh64_host.h for tests/test_xxh64_host.py.
#include "../../libzseek_amd/csrc/xxh64_host.h"

extern "C" {

uint64_t xs_oneshot(const void *p, size_t n)
{
    return zsk::xxh64(p, n);
}

// the digest of p[0, n) fed as updates of cuts[0], cuts[1], ... bytes (the
// rest in one last update)
uint64_t xs_stream(const uint8_t *p, size_t n, const size_t *cuts, size_t ncuts)
{
    zsk::Xxh64 s;
    s.init();
    size_t at = 0;
    for (size_t i = 0; i < ncuts && at < n; i++) {
        const size_t k = cuts[i] < n - at ? cuts[i] : n - at;
        s.update(p + at, k);
        at += k;
    }
    s.update(p + at, n - at);
    return s.digest();
}
}
