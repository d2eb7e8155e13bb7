// image_pieces.h — the per-piece rule of the builds from device-listed pieces
// (zsk_lz4_build_image_pieces / zsk_zstd_build_image_pieces, image_build.hip):
// when a piece of the list is valid, how the running source offset advances,
// what a refused piece becomes, and the capacity bound.  No HIP types and no
// runtime calls: image_pieces_kernel uses exactly these functions, and
// tests/native/image_pieces_shim.cpp drives them on the CPU.
//
// The list is data, not trusted input.  Piece i is `size` bytes of the source
// at `off`, the sum of the sizes before it.  It is valid when
//     1 <= size <= max_piece   and   off + size <= src_len;
// the first piece that is not makes the list invalid, and from there on every
// piece is refused: an empty piece at source offset 0, which reads no source
// byte and whose frame fits any slot.  The offset stops at the first invalid
// piece.  (Sizes are u32 and a batch holds at most 65,536 pieces on top of an
// offset <= src_len, so no 64-bit sum here wraps.)
#pragma once

#include <stdint.h>

#ifdef __HIP__
#define ZSK_IP_HD __host__ __device__
#else
#define ZSK_IP_HD
#endif

namespace zsk {

constexpr int64_t kImageFailed = -1;      // ZSK_IMAGE_FAILED
constexpr int64_t kImageBadPieces = -2;   // ZSK_IMAGE_BAD_PIECES
constexpr uint32_t kNoBadPiece = 0xFFFFFFFFu;

// bits of the chained state's flag word
constexpr uint64_t kStateRefused = 1;     // the compressor refused a frame (c_size 0)
constexpr uint64_t kStateBadPieces = 2;   // the list is invalid: sticky, later pieces become nothing

ZSK_IP_HD inline bool piece_valid(uint32_t size, uint64_t off, uint64_t max_piece, uint64_t src_len)
{
    return size != 0 && size <= max_piece && off <= src_len && size <= src_len - off;
}

// the offset of the piece after one of `size` bytes at `off`
ZSK_IP_HD inline uint64_t piece_advance(uint64_t off, uint32_t size)
{
    return off + size;
}

// What the compressor is handed for a piece.
struct PieceSpan {
    uint64_t src_off;
    uint32_t size;
};

// Piece i of a batch at `off`, with the batch's first invalid index (kNoBadPiece:
// none) known: itself, or the refused piece.
ZSK_IP_HD inline PieceSpan piece_span(uint32_t i, uint32_t size, uint64_t off, uint32_t first_bad)
{
    PieceSpan s;
    const bool keep = i < first_bad;
    s.src_off = keep ? off : 0;
    s.size = keep ? size : 0;
    return s;
}

// The capacity bounds.  For sizes s_i >= 1 that sum to at most src_len:
//   LZ4   ZSK_LZ4_COMPRESS_BOUND(s) = (s + 4 * (s >> 16) + 24 + 15) & ~15
//                                  <= s + 4 * (s >> 16) + 39,
//         and sum floor(s_i / 65536) <= floor(sum s_i / 65536), so the frames
//         take at most src_len + 4 * (src_len >> 16) + 39 * npieces;
//   zstd  ZSK_ZSTD_COMPRESS_BOUND(s) = (9 + 3 * ceil(s / 131072) + s + 4 + 15) & ~15
//                                   <= s + 3 * ceil(s / 131072) + 28,
//         ceil(s / 131072) <= (s >> 17) + 1 and sum (s_i >> 17) <= src_len >> 17,
//         so the frames take at most src_len + 3 * (src_len >> 17) + 31 * npieces.
// The table is 17 bytes and 8 (12 with checksums) per piece.  Against the sum
// of the exact macros (the fixed-frame zsk_*_image_bound) the slack is the
// rounding, under 16 bytes a piece, and one block word a piece: at most
// 19 * npieces (LZ4) and 18 * npieces (zstd).
ZSK_IP_HD inline uint64_t pieces_table_bytes(uint64_t npieces, bool checksums)
{
    return 8 + (checksums ? 12u : 8u) * npieces + 9;
}

ZSK_IP_HD inline uint64_t lz4_pieces_bound(uint64_t src_len, uint64_t npieces, bool checksums)
{
    return src_len + 4 * (src_len >> 16) + 39 * npieces + pieces_table_bytes(npieces, checksums);
}

ZSK_IP_HD inline uint64_t zstd_pieces_bound(uint64_t src_len, uint64_t npieces, bool checksums)
{
    return src_len + 3 * (src_len >> 17) + 31 * npieces + pieces_table_bytes(npieces, checksums);
}

// One batch of the list, the kernel's work spelled out as a loop (the CPU
// form; image_pieces_kernel does the same with a workgroup scan): spans[i]
// and the first invalid index.  *off is the running source offset and *bad
// the sticky flag, both advanced.
inline uint32_t pieces_batch(const uint32_t *sizes, uint32_t n, uint64_t max_piece, uint64_t src_len, uint64_t *off,
                             bool *bad, PieceSpan *spans)
{
    uint32_t first_bad = *bad ? 0 : kNoBadPiece;
    uint64_t at = *off;
    for (uint32_t i = 0; i < n && first_bad == kNoBadPiece; i++) {
        if (!piece_valid(sizes[i], at, max_piece, src_len))
            first_bad = i;
        else
            at = piece_advance(at, sizes[i]);
    }
    uint64_t o = *off;
    for (uint32_t i = 0; i < n; i++) {
        spans[i] = piece_span(i, sizes[i], o, first_bad);
        o = piece_advance(o, spans[i].size);
    }
    *off = at;
    if (first_bad != kNoBadPiece)
        *bad = true;
    return first_bad;
}

}   // namespace zsk
