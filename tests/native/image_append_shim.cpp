// Test-only C shim over libzseek_amd/csrc/image_append.h (the rules of
// zsk_lz4_append_image_pieces / zsk_zstd_append_image_pieces: the size window,
// the acceptance of an existing file, the room, the capacity bounds; pure, no
// HIP): tests/test_image_append.py builds it with g++ and calls it via ctypes.
#include "../../libzseek_amd/csrc/image_append.h"

extern "C" {

int iappend_window(int64_t size, uint64_t capacity, uint64_t prev_frames, int checksums)
{
    return zsk::append_window(size, capacity, prev_frames, checksums != 0) ? 1 : 0;
}

// The kernels' work on a file in host memory: the window, then (inside it
// only) the 17 header and footer bytes, the cSize sum and the first word read
// from image[0, capacity), then the verdict.  Returns 0 (accepted, room), or
// the result code the call answers.  *table_at: where the new frames start.
int64_t iappend_check(const uint8_t *image, uint64_t capacity, int64_t size, int64_t count, uint64_t prev_frames,
                      int checksums, int zstd, uint64_t src_len, uint64_t npieces, uint64_t *table_at)
{
    const bool ck = checksums != 0;
    uint8_t ends[zsk::kTableEnds] = {0};
    uint64_t sum = 0;
    uint32_t first = 0;
    if (zsk::append_window(size, capacity, prev_frames, ck)) {
        const uint64_t at = zsk::append_table_at(size, prev_frames, ck);
        const uint32_t ew = ck ? 3 : 2;
        for (uint32_t i = 0; i < zsk::kTableHeader; i++)
            ends[i] = image[at + i];
        for (uint32_t i = 0; i < zsk::kTableFooter; i++)
            ends[zsk::kTableHeader + i] = image[(uint64_t)size - zsk::kTableFooter + i];
        for (uint64_t f = 0; f < prev_frames; f++)
            sum += zsk::append_le32(image + at + zsk::kTableHeader + 4 * ew * f);
        if (prev_frames > 0)
            first = zsk::append_le32(image);
        *table_at = at;
    }
    const uint64_t v = zsk::append_verdict(size, count, capacity, prev_frames, ck, zstd != 0, ends, sum, first, src_len,
                                           npieces);
    return v == 0 ? 0 : v == zsk::kStateBadImage ? zsk::kImageBadImage : zsk::kImageNoRoom;
}

uint64_t iappend_lz4_bound(uint64_t prev_size, uint64_t prev_frames, uint64_t src_len, uint64_t npieces, int checksums)
{
    return zsk::lz4_append_bound(prev_size, prev_frames, src_len, npieces, checksums != 0);
}

uint64_t iappend_zstd_bound(uint64_t prev_size, uint64_t prev_frames, uint64_t src_len, uint64_t npieces, int checksums)
{
    return zsk::zstd_append_bound(prev_size, prev_frames, src_len, npieces, checksums != 0);
}

uint64_t iappend_table_bytes(uint64_t frames, int checksums)
{
    return zsk::append_table_bytes(frames, checksums != 0);
}

// bits: the flags that refuse every piece
uint64_t iappend_drop_mask(void)
{
    return zsk::kStateDrop;
}
}
