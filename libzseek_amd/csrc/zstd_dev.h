// zstd_dev.h -- what the zstd decoder's stages share: format constants, error
// codes, LDS access by byte address, the frame kernel's hand-off records
// (block slots, HufJob, the op list) and buffer spans of the compressed bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_dev.h"
#include "zsk_internal.h"

namespace zsk {
namespace {

using namespace lz4d;

constexpr uint32_t kZMagic = 0xFD2FB528u;
constexpr uint32_t kZBlockMax = 128u << 10;
constexpr uint32_t kItemExt = 0x80000000u;

enum : uint32_t {
    ZE_GENERIC = 1,
    ZE_PREFIX = 10,
    ZE_FRAMEPARAM = 14,
    ZE_WINDOW = 16,
    ZE_CORRUPT = 20,
    ZE_CHECKSUM = 22,
    ZE_DICT_CORRUPT = 30,
    ZE_DICT_WRONG = 32,
    ZE_DST_SMALL = 70,
    ZE_SRC_WRONG = 72,
};

__device__ __forceinline__ int32_t zerr(uint32_t e)
{
    return (int32_t)(ST_ZSTD_FLAG | e);
}

// LDS access by byte address (pointers into LDS converted to their offset)
template <typename T>
__device__ __forceinline__ __attribute__((address_space(3))) T *lp(const void *a)
{
    return (__attribute__((address_space(3))) T *)(uintptr_t)(uint32_t)(uintptr_t)a;
}

typedef u32x4 u32x4_a4 __attribute__((aligned(4)));

template <typename T>
__device__ __forceinline__ __attribute__((address_space(3))) T *la(uint32_t a)
{
    return (__attribute__((address_space(3))) T *)(uintptr_t)a;
}

__device__ __forceinline__ uint32_t ldsaddr(const void *p)
{
    return (uint32_t)(uintptr_t)p;
}

__device__ __forceinline__ uint32_t lane_id()
{
    return threadIdx.x & 63;
}

__device__ __forceinline__ int32_t hibit(uint32_t v)
{
    return 31 - __builtin_clz(v);
}

// ---- phase hand-off records (frame kernel -> Huffman / sequence kernels) --------------
// Per-block decoding tables, in HBM: the block's Huffman cells and its three
// FSE tables, so the lane-parallel kernels need no table building of their own.
constexpr uint32_t kZSlot = 10752;               // bytes per block slot
constexpr uint32_t kSlotFse = 8192;              // byte offset of the FSE cells (u16)
constexpr uint32_t kFseOff[3] = {0, 512, 768};   // LL / OF / ML, in u16 cells

// One Huffman stream (4 per block; len == 0: no stream).  32 bytes.
struct HufJob {
    uint64_t src;   // comp coordinate of the stream's first byte
    uint64_t dst;   // literal-scratch coordinate of its first symbol
    uint32_t len;   // stream bytes
    uint32_t cnt;   // symbols to decode
    uint32_t lim;   // symbols that may be stored (the frame's capacity)
    uint32_t tab;   // slot holding the Huffman cells | X2 decoder << 27 | table log << 28
};
constexpr uint32_t kHufSlotMask = (1u << 27) - 1;
static_assert(sizeof(HufJob) == 32, "HufJob");

// Per-frame op list, in decode order.  The frame kernel stops at its first
// error (OP_ERR); the sequence kernel replays the list and reports the first
// failure in libzstd's order, interleaving the Huffman kernel's stream
// results (OP_LIT) with the frame kernel's header checks.
enum : uint32_t {
    OP_LIT = 1,   // a: block -> the block's Huffman streams must have decoded cleanly
    OP_SEQ,       // a: nseq, b: stream (frame offset), c: stream bytes, d: literal start,
                  // e: literal count, f: block, g: table logs LL | OF << 4 | ML << 8
    OP_RUN,       // a: literal start, b: bytes (raw / RLE block)
    OP_FBEGIN,    // zstd frame starts: repeat offsets reset
    OP_FEND,      // a: 1 = content size present, 2 = checksum (4: the replay's request to check it,
                  // e/f: the frame's start and length); b/c: size lo/hi; d: checksum
    OP_ERR,       // a: status
    OP_DONE,
};
struct ZOp {
    uint32_t k, a, b, c, d, e, f, g;
};
static_assert(sizeof(ZOp) == 32, "ZOp");

__device__ __forceinline__ uint64_t op_base(const uint64_t *blk_base, uint32_t f)
{
    return 4 * blk_base[f] + 4ull * f;
}

constexpr uint32_t kOOR = 0x80000000u;   // out-of-range buffer offset: loads 0
constexpr uint64_t kMaxSpan = 0x7FFFFF00ull;   // largest span one resource covers

// mask of the bits of the dword at bit coordinate p that lie at or above xs
__device__ __forceinline__ uint32_t above(int32_t xs, int32_t p)
{
    const int32_t sh = xs - p;
    return sh <= 0 ? ~0u : sh >= 32 ? 0u : ~0u << sh;
}

// A span [base, base + len) of comp as a buffer resource (len < 2^31 - 256;
// rounded up to whole dwords: the hardware range-checks each dword).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_rsrc(const uint8_t *comp, uint64_t base, uint64_t len)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)(comp + base), 0, (int)(uint32_t)((len + 3) & ~3ull),
                                             kRsrcDw3);
}

}   // namespace
}   // namespace zsk
