// lean_ring.h — wrap arithmetic of the lean LZ4 parse's per-lane byte ring
// (lz4_lean.hip).  Plain C++17, constexpr throughout: the kernels and the CPU
// shim tests/native/lean_ring_shim.cpp compile the same text.
//
// The ring holds R bytes (a multiple of 32, not necessarily a power of two)
// at positions [0, R); ring bytes [0, 16) are mirrored at [R, R + 16), so a
// read that starts below R + 12 never wraps.  A stream coordinate x lives at
// position x % R, but the parse chain never divides: it carries the position
// of its read pointer and advances it with one add and one conditional
// subtract.  Coordinates themselves (what has arrived, what is needed, the
// fill's limit) stay absolute and are compared as such.
#pragma once
#include <stdint.h>

namespace zsk {

template <uint32_t R>
struct LeanRing {
    static_assert(R % 32 == 0 && R >= 256, "32-byte pieces; the head fill is 128 bytes");
    static constexpr bool kPow2 = (R & (R - 1)) == 0;
    // the fast step's longest advance from a read pointer that is itself up
    // to kSlack past the wrap: a token, one extension byte, 270 literals,
    // then the offset word and a match extension byte
    static constexpr uint32_t kMaxAdv = 273 + 3, kSlack = 3;
    static_assert(kPow2 || R + kSlack + kMaxAdv <= 2 * R, "one conditional subtract must cover the longest advance");
    static constexpr uint32_t kMirror = R, kMirrorLen = 16;

    // position of coordinate x (the mover after a jump, the exact step)
    static constexpr uint32_t of(uint32_t x) { return x % R; }

    // position (in [0, R)) n bytes after pos; pos < R + kSlack, n <= kMaxAdv
    static constexpr uint32_t adv(uint32_t pos, uint32_t n)
    {
        const uint32_t x = pos + n;
        if (kPow2)
            return x & (R - 1);
        return x - R < x ? x - R : x;   // unsigned min: x - R wraps high when x < R
    }

    // the read pointer after the sequence's last 2 or 3 bytes: not wrapped,
    // below R + kSlack -- the mirror serves the next read (pos in [0, R))
    static constexpr uint32_t adv_lazy(uint32_t pos, uint32_t n) { return pos + n; }

    // 4 bytes from pos (< R + 12) are bytes [pos & 3, (pos & 3) + 4) of the
    // two dwords at read4_at(pos) and read4_at(pos) + 4, both below R + 16
    static constexpr uint32_t read4_at(uint32_t pos) { return pos & ~3u; }
    static constexpr uint32_t read4_pick(uint32_t lo, uint32_t hi, uint32_t pos)
    {
        const uint32_t s = 8 * (pos & 3);
        return s ? (lo >> s) | (hi << (32 - s)) : lo;
    }

    // a slot's 32-byte piece i goes to piece_at(position of piece 0, i); the
    // piece at position 0 is written to the mirror too (its first 16 bytes)
    static constexpr uint32_t piece_at(uint32_t pos0, uint32_t i) { return adv(pos0, 32 * i); }
    static constexpr bool piece_mirrored(uint32_t pos) { return pos == 0; }
};

}   // namespace zsk
