// zstd_plan.h — the per-entry plan of the zstd decoder: the 8-byte item slots
// and block slots (tables, op list) a seek-table entry needs, from its frame,
// block and literals section headers and sequence counts.  One walk for
// zstd_plan_kernel and zstd_census_kernel (bytes through a buffer resource)
// and zstd_host_plan (bytes from host memory).  No HIP types: tests/native/zstd_plan_shim.cpp drives it.
#pragma once

#include <stdint.h>

#ifdef __HIP__
#define ZSK_HD __host__ __device__ __forceinline__
#else
#define ZSK_HD inline
#endif

namespace zsk {

struct ZstdFramePlan {
    uint32_t bound;    // item slots: 8 + 4 per block + 2 per sequence + the pairs' padding, rounded up to 4
    uint32_t blocks;   // block headers met
    bool cks;          // some frame carries a content checksum (the check kernel runs)
    uint64_t sequences;   // sequences the sequence sections declare (zstd_caps.h's bound counts them)
};

// B(p): byte p of the entry's clen bytes, 0 for p >= clen.  Walks skippable
// and concatenated frames, to the first thing that is not a frame, the entry's
// end, or a bound past 2^30 (the frame kernel refuses such an entry).
template <class ByteAt>
ZSK_HD ZstdFramePlan zstd_frame_plan(ByteAt B, uint32_t clen)
{
    constexpr uint32_t kMagic = 0xFD2FB528u, kSkippable = 0x184D2A50u;
    uint64_t items = 8, sequences = 0;
    uint32_t ip = 0, blocks = 0;
    bool cks = false;
    while (clen - ip >= 9 && items < (1u << 30)) {
        const uint32_t magic = B(ip) | B(ip + 1) << 8 | B(ip + 2) << 16 | B(ip + 3) << 24;
        if ((magic & 0xFFFFFFF0u) == kSkippable) {
            ip += 8 + (B(ip + 4) | B(ip + 5) << 8 | B(ip + 6) << 16 | B(ip + 7) << 24);
            continue;
        }
        if (magic != kMagic)
            break;
        const uint32_t fhd = B(ip + 4);
        const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, did = fhd & 3;
        ip += 5 + !single + (did == 3 ? 4 : did) + (fcs_flag == 0 ? single : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8);
        for (;;) {
            if (clen < ip + 3)
                break;
            const uint32_t bh = B(ip) | B(ip + 1) << 8 | B(ip + 2) << 16;
            const uint32_t type = (bh >> 1) & 3, bsize = bh >> 3;
            ip += 3;
            items += 4;
            blocks++;
            if (type == 2 && bsize >= 3) {
                const uint32_t b0 = B(ip), lt = b0 & 3, sf = (b0 >> 2) & 3;
                uint32_t sec;
                if (lt <= 1) {
                    const uint32_t lh = sf == 1 ? 2 : sf == 3 ? 3 : 1;
                    const uint32_t sz = sf == 1 ? (b0 | B(ip + 1) << 8) >> 4
                                      : sf == 3 ? (b0 | B(ip + 1) << 8 | B(ip + 2) << 16) >> 4
                                                : b0 >> 3;
                    sec = lt == 0 ? lh + sz : lh + 1;
                } else {
                    const uint32_t lhc = b0 | B(ip + 1) << 8 | B(ip + 2) << 16 | B(ip + 3) << 24;
                    sec = sf <= 1 ? 3 + ((lhc >> 14) & 0x3FF) : sf == 2 ? 4 + (lhc >> 18)
                                                                      : 5 + (lhc >> 22) + (B(ip + 4) << 10);
                }
                if (sec < bsize) {
                    const uint32_t q = ip + sec, s0 = B(q);
                    const uint32_t nseq = s0 < 128 ? s0 : s0 < 255 ? ((s0 - 128) << 8) + B(q + 1)
                                                                   : (B(q + 1) | B(q + 2) << 8) + 0x7F00;
                    items += 2ull * nseq + (2ull * nseq + 62) / 63;
                    sequences += nseq;
                }
            }
            ip += type == 1 ? 1 : bsize;
            if ((bh & 1) || ip > clen)
                break;
        }
        if (ip > clen)
            break;
        if ((fhd >> 2) & 1) {
            ip += 4;
            cks = true;
        }
    }
    return ZstdFramePlan{(uint32_t)((items + 3) & ~3ull), blocks, cks, sequences};
}

}   // namespace zsk
