// Test-only C shim over libzseek_amd/csrc/lean_ring.h (constexpr functions, no
// HIP): tests/test_lean_ring.py builds it with g++ and calls it via ctypes.
// Every check runs here, against a plain byte array and `%`; a failing check
// returns its line number and the values in out[0..3], 0 means all held.
#include "../../libzseek_amd/csrc/lean_ring.h"

#include <string.h>

#include <vector>

namespace {

#define CHECK(cond, a, b, c, d)                                                                     \
    do {                                                                                            \
        if (!(cond)) {                                                                              \
            out[0] = (uint32_t)(a), out[1] = (uint32_t)(b), out[2] = (uint32_t)(c), out[3] = (uint32_t)(d); \
            return __LINE__;                                                                        \
        }                                                                                           \
    } while (0)

// the byte the stream holds at coordinate x
inline uint8_t stream(uint32_t x) { return (uint8_t)((x * 2654435761u) >> 13); }

inline uint32_t le32(const uint8_t *p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

template <uint32_t R>
int run(uint32_t *out)
{
    using Ring = zsk::LeanRing<R>;
    // ---- advancing: every start, the lazy slack included, every advance ----
    for (uint32_t pos = 0; pos < R + Ring::kSlack; pos++)
        for (uint32_t n = 0; n <= Ring::kMaxAdv; n++) {
            CHECK(Ring::adv(pos, n) == (pos + n) % R, R, pos, n, Ring::adv(pos, n));
            if (pos < R && n <= Ring::kSlack)
                CHECK(Ring::adv_lazy(pos, n) == pos + n && pos + n < R + Ring::kSlack, R, pos, n, 0);
        }
    // ---- a coordinate's position, by division --------------------------------
    for (uint32_t x = 0; x < 3 * R + 64; x++)
        CHECK(Ring::of(x) == x % R, R, x, Ring::of(x), 0);
    CHECK(Ring::of(0x7FFFFFE0u) == 0x7FFFFFE0u % R, R, 0, 0, 0);
    // ---- 4-byte reads against a plain ring -----------------------------------
    // area: the ring [0, R) and its mirror.  The ring holds the stream's
    // coordinates [lo, lo + R), byte x at position x % R; a read of 4 bytes
    // inside that window goes through position x % R, and also through the
    // unwrapped position R + x % R where adv_lazy can leave it (< R + kSlack)
    std::vector<uint8_t> area(R + Ring::kMirrorLen);
    for (uint32_t lo = 0; lo < 2 * R; lo++) {
        for (uint32_t x = lo; x < lo + R; x++)
            area[x % R] = stream(x);
        memcpy(&area[Ring::kMirror], &area[0], Ring::kMirrorLen);
        for (uint32_t x = lo; x + 4 <= lo + R; x++) {
            uint8_t want[4];
            for (int i = 0; i < 4; i++)
                want[i] = stream(x + i);
            for (uint32_t pos = x % R; pos < R + Ring::kSlack; pos += R) {
                const uint32_t a = Ring::read4_at(pos);
                CHECK(a % 4 == 0 && a + 8 <= R + Ring::kMirrorLen, R, pos, a, lo);
                const uint32_t got = Ring::read4_pick(le32(&area[a]), le32(&area[a + 4]), pos);
                CHECK(got == le32(want), R, pos, got, le32(want));
            }
        }
    }
    // ---- slot placement: every 32-aligned coordinate over three laps ---------
    // carried positions (a jump, then pieces advancing) against x % R, the
    // bytes against a plain ring, the mirror after the piece at position 0
    for (uint32_t pieces = 2; pieces <= 4; pieces++)
        for (uint32_t jump = 0; jump < 3 * R; jump += 32) {
            std::vector<uint8_t> plain(R), ring(R + 16, 0xEE);
            uint32_t pos = Ring::of(jump);
            CHECK(pos == jump % R, R, jump, pos, 0);
            for (uint32_t x = jump; x < jump + 3 * R;) {
                const uint32_t n = 1 + (x / 32 + jump / 32) % pieces;   // a slot of 1..pieces pieces
                for (uint32_t i = 0; i < n; i++) {
                    const uint32_t at = Ring::piece_at(pos, i), c = x + 32 * i;
                    CHECK(at == c % R && at % 32 == 0 && at + 32 <= R, R, c, at, i);
                    for (uint32_t b = 0; b < 32; b++)
                        ring[at + b] = plain[c % R + b] = stream(c + b);
                    CHECK(Ring::piece_mirrored(at) == (c % R == 0), R, c, at, 1);
                    if (Ring::piece_mirrored(at))
                        memcpy(&ring[Ring::kMirror], &ring[0], Ring::kMirrorLen);
                }
                pos = Ring::adv(pos, 32 * n);
                x += 32 * n;
                CHECK(pos == x % R, R, x, pos, 2);
            }
            CHECK(memcmp(ring.data(), plain.data(), R) == 0, R, jump, 0, 3);
            CHECK(memcmp(&ring[Ring::kMirror], plain.data(), Ring::kMirrorLen) == 0, R, jump, 0, 4);
        }
    return 0;
}

}   // namespace

extern "C" int lean_ring_check(uint32_t R, uint32_t *out)
{
    switch (R) {
    case 256: return run<256>(out);
    case 288: return run<288>(out);
    case 320: return run<320>(out);
    }
    return -1;
}
