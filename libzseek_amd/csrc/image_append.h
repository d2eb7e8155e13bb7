// image_append.h — the rules of an append to a seekable image in device memory
// (zsk_lz4_append_image_pieces / zsk_zstd_append_image_pieces, image_build.hip):
// where an existing file's seek table lies, when the file is accepted, when
// the appended file is sure to fit, and the capacity bounds.  No HIP types and
// no runtime calls: image_stash_kernel and image_append_check_kernel use
// exactly these functions, and tests/native/image_append_shim.cpp drives them
// on the CPU.
//
// The existing file is data, not trusted input: its size and frame count come
// from device memory (d_prev) and its table from the image.  The host states
// the frame count (prev_frames), which fixes the table's length, so the one
// window
//     table_bytes(prev_frames) <= size <= capacity
// bounds every later read: the table is the file's last table_bytes bytes.
// Only a file that passes the window is looked at; only a file that passes
// append_accept is written to.
#pragma once

#include <stdint.h>

#include "image_pieces.h"

namespace zsk {

constexpr int64_t kImageBadImage = -3;   // ZSK_IMAGE_BAD_IMAGE
constexpr int64_t kImageNoRoom = -4;     // ZSK_IMAGE_NO_ROOM

// further bits of the chained state's flag word (image_pieces.h): both sticky,
// both turn every piece into nothing as kStateBadPieces does
constexpr uint64_t kStateBadImage = 4;   // d_prev / the image are not a valid file
constexpr uint64_t kStateNoRoom = 8;     // the appended file might not fit
constexpr uint64_t kStateDrop = kStateBadPieces | kStateBadImage | kStateNoRoom;

constexpr uint32_t kSkippableMagic = 0x184D2A5Eu, kSeekMagic = 0x8F92EAB1u;   // ref seek_table.c
constexpr uint32_t kLz4FrameMagic = 0x184D2204u, kZstdFrameMagic = 0xFD2FB528u;
constexpr uint32_t kTableHeader = 8, kTableFooter = 9;   // skippable header; count, descriptor, magic
constexpr uint32_t kTableEnds = kTableHeader + kTableFooter;

// the table of a file of `frames` frames: header, entries, footer
ZSK_IP_HD inline uint64_t append_table_bytes(uint64_t frames, bool checksums)
{
    return pieces_table_bytes(frames, checksums);
}

// The size window.  Checked first, before any read of the image.
ZSK_IP_HD inline bool append_window(int64_t size, uint64_t capacity, uint64_t prev_frames, bool checksums)
{
    return size >= 0 && (uint64_t)size >= append_table_bytes(prev_frames, checksums) && (uint64_t)size <= capacity;
}

// where the table of a file in the window starts: the end of its frames
ZSK_IP_HD inline uint64_t append_table_at(int64_t size, uint64_t prev_frames, bool checksums)
{
    return (uint64_t)size - append_table_bytes(prev_frames, checksums);
}

ZSK_IP_HD inline uint32_t append_le32(const uint8_t *p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// The acceptance rule (read_seek_table's, host_support.cpp, plus what the
// host stated).  @size, @count: d_prev[0], d_prev[1].  @ends: the table's 8
// header bytes and 9 footer bytes (read only when the window holds; anything
// otherwise).  @csize_sum: the sum of the entries' cSize.  @first_magic: the
// file's first four bytes when prev_frames > 0 (else ignored): what
// zseek_reader_open sniffs the codec by.  @checksums: flags & ZSK_IMAGE_CHECKSUMS.
ZSK_IP_HD inline bool append_accept(int64_t size, int64_t count, uint64_t capacity, uint64_t prev_frames,
                                    bool checksums, bool zstd, const uint8_t ends[kTableEnds], uint64_t csize_sum,
                                    uint32_t first_magic)
{
    if (count < 0 || (uint64_t)count != prev_frames)
        return false;
    if (!append_window(size, capacity, prev_frames, checksums))
        return false;
    const uint8_t *foot = ends + kTableHeader;
    const uint8_t desc = foot[4];
    if (append_le32(foot + 5) != kSeekMagic || (desc & 0x7c) != 0)
        return false;
    if (append_le32(foot) != prev_frames || ((desc & 0x80) != 0) != checksums)
        return false;
    const uint64_t table = append_table_bytes(prev_frames, checksums);
    if (append_le32(ends) != kSkippableMagic || append_le32(ends + 4) != table - kTableHeader)
        return false;
    if (csize_sum != append_table_at(size, prev_frames, checksums))
        return false;
    if (prev_frames > 0 && first_magic != (zstd ? kZstdFrameMagic : kLz4FrameMagic))
        return false;
    return true;
}

// The bounds: the old frames stay, the new frames take at most the frames
// part of zsk_*_pieces_bound(src_len, npieces), the table covers all frames.
// 0 when prev_size cannot hold a table of prev_frames entries.  Monotone in
// prev_size.
ZSK_IP_HD inline uint64_t append_bound_of(uint64_t new_frames_bound, uint64_t prev_size, uint64_t prev_frames,
                                          uint64_t npieces, bool checksums)
{
    const uint64_t old_table = append_table_bytes(prev_frames, checksums);
    if (prev_size < old_table)
        return 0;
    return prev_size - old_table + new_frames_bound + append_table_bytes(prev_frames + npieces, checksums);
}

ZSK_IP_HD inline uint64_t lz4_append_bound(uint64_t prev_size, uint64_t prev_frames, uint64_t src_len,
                                           uint64_t npieces, bool checksums)
{
    return append_bound_of(lz4_pieces_bound(src_len, npieces, checksums) - pieces_table_bytes(npieces, checksums),
                           prev_size, prev_frames, npieces, checksums);
}

ZSK_IP_HD inline uint64_t zstd_append_bound(uint64_t prev_size, uint64_t prev_frames, uint64_t src_len,
                                            uint64_t npieces, bool checksums)
{
    return append_bound_of(zstd_pieces_bound(src_len, npieces, checksums) - pieces_table_bytes(npieces, checksums),
                           prev_size, prev_frames, npieces, checksums);
}

// The room rule, for an accepted file of @size bytes: everything the call may
// write lies below the bound.
ZSK_IP_HD inline bool append_room(bool zstd, int64_t size, uint64_t prev_frames, uint64_t src_len, uint64_t npieces,
                                  bool checksums, uint64_t capacity)
{
    const uint64_t need = zstd ? zstd_append_bound((uint64_t)size, prev_frames, src_len, npieces, checksums)
                               : lz4_append_bound((uint64_t)size, prev_frames, src_len, npieces, checksums);
    return need != 0 && need <= capacity;
}

// What the check leaves in the state's flag word: 0, kStateBadImage or
// kStateNoRoom (in that precedence).
ZSK_IP_HD inline uint64_t append_verdict(int64_t size, int64_t count, uint64_t capacity, uint64_t prev_frames,
                                         bool checksums, bool zstd, const uint8_t ends[kTableEnds],
                                         uint64_t csize_sum, uint32_t first_magic, uint64_t src_len,
                                         uint64_t npieces)
{
    if (!append_accept(size, count, capacity, prev_frames, checksums, zstd, ends, csize_sum, first_magic))
        return kStateBadImage;
    if (!append_room(zstd, size, prev_frames, src_len, npieces, checksums, capacity))
        return kStateNoRoom;
    return 0;
}

}   // namespace zsk
