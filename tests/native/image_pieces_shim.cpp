// Test-only C shim over libzseek_amd/csrc/image_pieces.h (the per-piece rule of
// zsk_lz4_build_image_pieces / zsk_zstd_build_image_pieces: validity, the
// running source offset, the refused piece, the capacity bounds; pure, no
// HIP): tests/test_image_pieces.py builds it with g++ and calls it via ctypes.
#include "../../libzseek_amd/csrc/image_pieces.h"

#include <vector>

extern "C" {

int ipieces_valid(uint32_t size, uint64_t off, uint64_t max_piece, uint64_t src_len)
{
    return zsk::piece_valid(size, off, max_piece, src_len) ? 1 : 0;
}

// The list in batches of `per` pieces, chained through the running offset and
// the sticky flag as the builder chains its kernels.  src_off[n], size[n]: what
// the compressor is handed per piece; first_bad[batches]: each batch's first
// invalid index (0xFFFFFFFF: none).  Returns the final running offset; *bad_out
// the final flag.
uint64_t ipieces_plan(const uint32_t *sizes, uint32_t n, uint32_t per, uint64_t max_piece, uint64_t src_len,
                      uint64_t *src_off, uint32_t *size, uint32_t *first_bad, int *bad_out)
{
    uint64_t off = 0;
    bool bad = false;
    std::vector<zsk::PieceSpan> spans(per ? per : 1);
    for (uint32_t f = 0, b = 0; per && f < n; f += per, b++) {
        const uint32_t m = n - f < per ? n - f : per;
        first_bad[b] = zsk::pieces_batch(sizes + f, m, max_piece, src_len, &off, &bad, spans.data());
        for (uint32_t i = 0; i < m; i++) {
            src_off[f + i] = spans[i].src_off;
            size[f + i] = spans[i].size;
        }
    }
    *bad_out = bad ? 1 : 0;
    return off;
}

uint64_t ipieces_lz4_bound(uint64_t src_len, uint64_t npieces, int checksums)
{
    return zsk::lz4_pieces_bound(src_len, npieces, checksums != 0);
}

uint64_t ipieces_zstd_bound(uint64_t src_len, uint64_t npieces, int checksums)
{
    return zsk::zstd_pieces_bound(src_len, npieces, checksums != 0);
}

int64_t ipieces_code(int which)
{
    return which ? zsk::kImageBadPieces : zsk::kImageFailed;
}
}
