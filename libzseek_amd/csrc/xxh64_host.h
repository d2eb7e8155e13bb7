// xxh64_host.h — XXH64 on the host, written from the XXH64 specification
// (xxHash fast digest algorithm, "XXH64 algorithm description"): the writer's
// seek-table frame checksums (low 32 bits, seed 0) for the frames it
// compresses on the host.  One-shot xxh64() and a streaming state
// (init / update / digest) for frames whose bytes arrive over several writes.
// Neither liblz4 nor libzstd exports XXH64, and the product does not link the
// test oracle, so the library carries its own.  Little-endian hosts only, as
// the rest of the library.
#ifndef ZSK_XXH64_HOST_H
#define ZSK_XXH64_HOST_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace zsk {

struct Xxh64 {
    static constexpr uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull,
                              P4 = 0x85EBCA77C2B2AE63ull, P5 = 0x27D4EB2F165667C5ull;
    uint64_t acc[4];
    uint64_t total;     // bytes seen
    uint8_t buf[32];    // a partial stripe
    uint32_t held;      // bytes in buf

    static uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
    static uint64_t rd64(const uint8_t *p)
    {
        uint64_t v;
        memcpy(&v, p, 8);
        return v;
    }
    static uint32_t rd32(const uint8_t *p)
    {
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    }
    static uint64_t round(uint64_t a, uint64_t v) { return rotl(a + v * P2, 31) * P1; }
    static uint64_t merge(uint64_t h, uint64_t v) { return (h ^ round(0, v)) * P1 + P4; }

    void init(uint64_t seed = 0)
    {
        acc[0] = seed + P1 + P2;
        acc[1] = seed + P2;
        acc[2] = seed;
        acc[3] = seed - P1;
        total = 0;
        held = 0;
    }
    void stripe(const uint8_t *p)
    {
        for (int k = 0; k < 4; k++)
            acc[k] = round(acc[k], rd64(p + 8 * k));
    }
    void update(const void *data, size_t len)
    {
        const uint8_t *p = static_cast<const uint8_t *>(data);
        total += len;
        if (held) {
            const size_t take = len < 32 - held ? len : 32 - held;
            memcpy(buf + held, p, take);
            held += (uint32_t)take;
            p += take;
            len -= take;
            if (held < 32)
                return;
            stripe(buf);
            held = 0;
        }
        for (; len >= 32; p += 32, len -= 32)
            stripe(p);
        if (len) {
            memcpy(buf, p, len);
            held = (uint32_t)len;
        }
    }
    // (acc[2] - seed recovers the seed for inputs under one stripe)
    uint64_t digest() const
    {
        uint64_t h;
        if (total >= 32) {
            h = rotl(acc[0], 1) + rotl(acc[1], 7) + rotl(acc[2], 12) + rotl(acc[3], 18);
            for (int k = 0; k < 4; k++)
                h = merge(h, acc[k]);
        } else {
            h = acc[2] + P5;
        }
        h += total;
        const uint8_t *p = buf;
        uint32_t n = held;
        for (; n >= 8; p += 8, n -= 8)
            h = rotl(h ^ round(0, rd64(p)), 27) * P1 + P4;
        if (n >= 4) {
            h = rotl(h ^ rd32(p) * P1, 23) * P2 + P3;
            p += 4;
            n -= 4;
        }
        for (; n; p++, n--)
            h = rotl(h ^ *p * P5, 11) * P1;
        h ^= h >> 33;
        h *= P2;
        h ^= h >> 29;
        h *= P3;
        h ^= h >> 32;
        return h;
    }
};

inline uint64_t xxh64(const void *data, size_t len, uint64_t seed = 0)
{
    Xxh64 s;
    s.init(seed);
    s.update(data, len);
    return s.digest();
}

}   // namespace zsk

#endif
