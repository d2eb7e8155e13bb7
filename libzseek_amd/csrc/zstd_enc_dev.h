// zstd_enc_dev.h — the format layer of the GPU zstd compressor
// (zstd_compress.hip): everything that decides a frame's bytes once the
// matches are known.  Host and device compile the same functions (the way
// range_plan_dev.h is shared): the kernels call them from lanes, and
// tests/native/zstd_enc_shim.cpp drives them serially on the CPU, where the
// frames are judged by libzstd 1.4.9 and oracle/zstd_oracle.c.
//
// The format subset (RFC 8878; the in-tree decoders are the specification):
//   frame     magic, Single_Segment header without dictionary id,
//             Frame_Content_Size in its smallest field, blocks of at most
//             kZBlock input bytes, optionally the low 32 bits of XXH64
//   block     Compressed when that is smaller than the block's input, RLE for
//             one repeated byte, Raw otherwise; nothing crosses a block
//             boundary but match offsets (never before the frame's start)
//   literals  Raw, RLE, or Huffman with code lengths <= 11 whose tree is
//             described by direct 4-bit weights; that form lists at most 128
//             weights, so literals holding a byte above 128 are stored Raw
//             (FSE-compressed weights are not written); one stream below 256
//             literals, four above
//   sequences predefined LL / OF / ML tables (mode byte 0), every offset
//             coded as offset + 3 (no repeat codes), one backward bitstream
// Not written: repeat or treeless tables, custom FSE tables, repeat offsets,
// dictionaries, windows (frames are single-segment, <= 4 MiB).
//
// This file is ZSK_ZSTD_FORMAT_SUBSET and stays as it is: its frames are pinned
// byte for byte (tests/golden/zstd_enc_subset.json).  ZSK_ZSTD_FORMAT_FULL --
// Huffman over all 256 byte values with FSE-compressed weights, a mode per
// sequence table, repeat offsets -- is zstd_enc_full_dev.h, which adds its
// layer beside these functions and uses them.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIP__
#define ZENC_HD __host__ __device__ inline
#else
#define ZENC_HD inline
#endif

namespace zsk {
namespace zenc {

constexpr uint32_t kZBlock = 1u << 17;   // input bytes per block: the format's largest, so a 64 KiB or
                                         // 128 KiB frame is one block and every length code can occur
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kHashLog = 12;         // the match search's table: positions by 4-byte hash
constexpr uint32_t kHufMaxBits = 11;
constexpr uint32_t kHufSyms = 129;       // bytes 0..128: what direct weights describe
constexpr uint32_t kMaxFrame = 1u << 22;   // ZSK_ZSTD_COMPRESS_MAX_FRAME
constexpr uint32_t kFrameHeaderMax = 9;    // magic, descriptor, 4-byte content size

struct Seq {
    uint32_t ll, ml, off;   // literals before the match, match length (>= 3), offset (>= 1)
};

ZENC_HD uint32_t highbit(uint32_t v)
{
    return 31u - (uint32_t)__builtin_clz(v);
}

// ---------------------------------------------------------------- bit writer
// Bits are added low first and bytes leave in memory order: zstd's backward
// bitstreams, which the decoder reads from the last byte down.  Writes stop at
// `end` (ovf is set and kept).
struct BitW {
    uint8_t *p, *end;
    uint64_t acc;
    uint32_t n;
    bool ovf;
};

ZENC_HD void bw_init(BitW &b, uint8_t *p, uint8_t *end)
{
    b.p = p;
    b.end = end;
    b.acc = 0;
    b.n = 0;
    b.ovf = false;
}

// nb <= 32 low bits of v
ZENC_HD void bw_add(BitW &b, uint32_t v, uint32_t nb)
{
    b.acc |= ((uint64_t)v & ((1ull << nb) - 1)) << b.n;
    b.n += nb;
    if (b.n >= 32) {
        if (b.end - b.p < 4) {
            b.ovf = true;
        } else {
            b.p[0] = (uint8_t)b.acc;
            b.p[1] = (uint8_t)(b.acc >> 8);
            b.p[2] = (uint8_t)(b.acc >> 16);
            b.p[3] = (uint8_t)(b.acc >> 24);
            b.p += 4;
        }
        b.acc >>= 32;
        b.n -= 32;
    }
}

// The final-bit marker and the last bytes; the stream's end, or nullptr.
ZENC_HD uint8_t *bw_close(BitW &b)
{
    bw_add(b, 1, 1);
    while (b.n > 0) {
        if (b.p >= b.end) {
            b.ovf = true;
            break;
        }
        *b.p++ = (uint8_t)b.acc;
        b.acc >>= 8;
        b.n = b.n > 8 ? b.n - 8 : 0;
    }
    return b.ovf ? nullptr : b.p;
}

// ------------------------------------------------------------------- Huffman
struct HufCode {
    uint8_t len[kHufSyms];     // 0: absent
    uint16_t code[kHufSyms];
    uint32_t max_sym;          // largest byte value present
    uint32_t max_bits;         // 0: fewer than 2 symbols (no code)
};

constexpr uint32_t kHufWorkWords = 2 * kHufSyms + kHufSyms + kHufSyms;   // huf_lengths' ws

// Code lengths <= kHufMaxBits for count[0..kHufSyms): a Huffman tree over the
// symbols sorted by (count, value), then the lengths above the limit are cut
// to it and the Kraft sum is brought back to exactly 1 -- over: the rarest
// symbol of the longest length below the limit grows by one; under: the most
// frequent symbol whose step still fits shrinks by one.  Every tie is broken
// by symbol value, so the lengths are a function of the counts alone.
ZENC_HD void huf_lengths(const uint32_t *count, HufCode &h, uint32_t *ws)
{
    uint32_t *w = ws;                                    // node weights, 2n
    uint16_t *par = reinterpret_cast<uint16_t *>(ws + 2 * kHufSyms);   // 2n
    uint8_t *order = reinterpret_cast<uint8_t *>(ws + 3 * kHufSyms);   // n: sorted symbols
    uint8_t *depth = order + kHufSyms;                   // 2n
    uint32_t n = 0;
    h.max_sym = 0;
    h.max_bits = 0;
    for (uint32_t s = 0; s < kHufSyms; s++) {
        h.len[s] = 0;
        h.code[s] = 0;
        if (count[s] == 0)
            continue;
        h.max_sym = s;
        uint32_t i = n++;   // insertion by (count, value): values arrive ascending
        while (i > 0 && count[order[i - 1]] > count[s]) {
            order[i] = order[i - 1];
            i--;
        }
        order[i] = (uint8_t)s;
    }
    if (n < 2)
        return;
    for (uint32_t i = 0; i < n; i++)
        w[i] = count[order[i]];
    // two queues: leaves [li, n) and internal nodes [ni, nn), both ascending
    uint32_t li = 0, ni = n, nn = n;
    while (nn < 2 * n - 1) {
        uint32_t pick[2];
        for (int k = 0; k < 2; k++) {
            if (li < n && (ni >= nn || w[li] <= w[ni]))
                pick[k] = li++;
            else
                pick[k] = ni++;
        }
        w[nn] = w[pick[0]] + w[pick[1]];
        par[pick[0]] = (uint16_t)nn;
        par[pick[1]] = (uint16_t)nn;
        nn++;
    }
    depth[nn - 1] = 0;
    for (uint32_t i = nn - 1; i-- > 0;)
        depth[i] = (uint8_t)(depth[par[i]] + 1);
    // the limit; K = the Kraft sum in units of 2^-kHufMaxBits
    uint32_t K = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (depth[i] > kHufMaxBits)
            depth[i] = (uint8_t)kHufMaxBits;
        K += 1u << (kHufMaxBits - depth[i]);
    }
    const uint32_t full = 1u << kHufMaxBits;
    while (K > full) {
        // lengths fall along the sorted order: the first one below the limit
        // is the longest such length's rarest symbol
        uint32_t i = 0;
        while (i < n && depth[i] >= kHufMaxBits)
            i++;
        if (i == n)   // (n <= 129 < 2^kHufMaxBits symbols: never)
            break;
        K -= 1u << (kHufMaxBits - depth[i] - 1);
        depth[i]++;
    }
    while (K < full) {
        const uint32_t d = full - K;
        uint32_t i = n;
        while (i-- > 0)
            if (depth[i] > 1 && (1u << (kHufMaxBits - depth[i])) <= d)
                break;
        if (i >= n)   // (K is a multiple of the longest code's step: never)
            break;
        K += 1u << (kHufMaxBits - depth[i]);
        depth[i]--;
    }
    uint32_t mb = 0;
    for (uint32_t i = 0; i < n; i++) {
        h.len[order[i]] = depth[i];
        mb = depth[i] > mb ? depth[i] : mb;
    }
    h.max_bits = mb;
    // canonical codes by zstd's weight rule: the decoding table is filled by
    // ascending weight (= descending length), then by symbol value; a code is
    // its first cell's index without the bits the symbol does not use
    uint32_t pos = 0;
    for (uint32_t l = mb; l >= 1; l--)
        for (uint32_t s = 0; s <= h.max_sym; s++)
            if (h.len[s] == l) {
                h.code[s] = (uint16_t)(pos >> (mb - l));
                pos += 1u << (mb - l);
            }
}

// The tree description by direct weights: 127 + the number of weights listed
// (symbols 0 .. max_sym - 1; the last symbol's weight is what completes the
// sum), then two weights per byte, the first in the high nibble.
ZENC_HD uint32_t huf_desc_size(const HufCode &h)
{
    return 1 + (h.max_sym + 1) / 2;
}

ZENC_HD uint32_t huf_write_desc(const HufCode &h, uint8_t *dst)
{
    dst[0] = (uint8_t)(127 + h.max_sym);
    for (uint32_t s = 0; s < h.max_sym; s += 2) {
        const uint32_t a = h.len[s] ? h.max_bits + 1 - h.len[s] : 0;
        const uint32_t b = (s + 1 < h.max_sym && h.len[s + 1]) ? h.max_bits + 1 - h.len[s + 1] : 0;
        dst[1 + s / 2] = (uint8_t)(a << 4 | b);
    }
    return huf_desc_size(h);
}

// Bytes of the stream that encodes symbols of `bits` code bits in all.
ZENC_HD uint32_t huf_stream_size(uint64_t bits)
{
    return (uint32_t)((bits + 1 + 7) / 8);
}

// One stream: lit[0..n) encoded last symbol first into dst (huf_stream_size
// bytes, which the caller has made room for).
ZENC_HD uint32_t huf_encode_stream(const HufCode &h, const uint8_t *lit, uint32_t n, uint8_t *dst, uint8_t *end)
{
    BitW b;
    bw_init(b, dst, end);
    for (uint32_t i = n; i-- > 0;) {
        const uint32_t s = lit[i];
        bw_add(b, h.code[s], h.len[s]);
    }
    const uint8_t *e = bw_close(b);
    return e ? (uint32_t)(e - dst) : 0;
}

// Four streams from 256 literals up (libzstd's threshold); a stream holds
// (n + 3) / 4 symbols, the last one the rest.
ZENC_HD uint32_t huf_streams(uint32_t n)
{
    return n >= 256 ? 4 : 1;
}

ZENC_HD uint32_t huf_segment(uint32_t n)
{
    return (n + 3) / 4;
}

// Literals_Section_Header of a Raw (type 0) or RLE (type 1) section of n bytes.
ZENC_HD uint32_t lit_header_plain(uint8_t *dst, uint32_t type, uint32_t n)
{
    if (n < 32) {
        dst[0] = (uint8_t)(type | n << 3);
        return 1;
    }
    if (n < 4096) {
        const uint32_t v = type | 1u << 2 | n << 4;
        dst[0] = (uint8_t)v;
        dst[1] = (uint8_t)(v >> 8);
        return 2;
    }
    const uint32_t v = type | 3u << 2 | n << 4;
    dst[0] = (uint8_t)v;
    dst[1] = (uint8_t)(v >> 8);
    dst[2] = (uint8_t)(v >> 16);
    return 3;
}

ZENC_HD uint32_t lit_header_plain_size(uint32_t n)
{
    return n < 32 ? 1 : n < 4096 ? 2 : 3;
}

// ... of a Huffman-compressed section: n literals in `comp` bytes (tree
// description, jump table and streams).  One stream only exists in the
// 10-bit form, which n < 256 always fits (comp < n is the caller's condition).
ZENC_HD uint32_t lit_header_huf_size(uint32_t n, uint32_t comp)
{
    return (n < 1024 && comp < 1024) ? 3 : (n < 16384 && comp < 16384) ? 4 : 5;
}

ZENC_HD uint32_t lit_header_huf(uint8_t *dst, uint32_t n, uint32_t comp)
{
    const uint32_t hs = lit_header_huf_size(n, comp);
    if (hs == 3) {
        const uint32_t v = 2u | (huf_streams(n) == 4 ? 1u : 0u) << 2 | n << 4 | comp << 14;
        dst[0] = (uint8_t)v;
        dst[1] = (uint8_t)(v >> 8);
        dst[2] = (uint8_t)(v >> 16);
    } else if (hs == 4) {
        const uint32_t v = 2u | 2u << 2 | n << 4 | comp << 18;
        dst[0] = (uint8_t)v;
        dst[1] = (uint8_t)(v >> 8);
        dst[2] = (uint8_t)(v >> 16);
        dst[3] = (uint8_t)(v >> 24);
    } else {
        const uint64_t v = 2u | 3u << 2 | (uint64_t)n << 4 | (uint64_t)comp << 22;
        for (int i = 0; i < 5; i++)
            dst[i] = (uint8_t)(v >> (8 * i));
    }
    return hs;
}

// How a block's literals are stored, from their histogram (count[0..kHufSyms),
// `high` = literals above 128) and, for a Huffman code, its streams' sizes.
enum LitMode { kLitRaw = 0, kLitRle = 1, kLitHuf = 2 };

struct LitPlan {
    uint32_t mode;
    uint32_t n;
    uint32_t stream[4];   // Huffman: bytes per stream
    uint32_t comp;        // Huffman: description + jump table + streams
    uint32_t size;        // the whole section, header included
};

// Step 1, from the histogram: RLE, Raw for certain, or "try Huffman" (h is
// then built and the caller counts each stream's code bits).
ZENC_HD bool lit_wants_huf(const uint32_t *count, uint32_t high, uint32_t n, HufCode &h, uint32_t *ws, LitPlan &p)
{
    p.n = n;
    p.comp = 0;
    p.mode = kLitRaw;
    p.size = lit_header_plain_size(n) + n;
    if (n == 0)
        return false;
    if (high != 0)   // a byte the direct weights cannot describe
        return false;
    uint32_t distinct = 0;
    for (uint32_t s = 0; s < kHufSyms && distinct < 2; s++)
        distinct += count[s] != 0;
    if (distinct == 1) {
        p.mode = kLitRle;
        p.size = lit_header_plain_size(n) + 1;
        return false;
    }
    if (n < 8)   // a description alone is 2 bytes or more and a stream 1: never smaller
        return false;
    huf_lengths(count, h, ws);
    return h.max_bits != 0;
}

// Step 2, from the streams' code bits: Huffman only when smaller than Raw.
ZENC_HD void lit_plan_huf(const HufCode &h, const uint64_t *bits, LitPlan &p)
{
    const uint32_t ns = huf_streams(p.n);
    uint32_t comp = huf_desc_size(h) + (ns == 4 ? 6 : 0);
    for (uint32_t k = 0; k < ns; k++) {
        p.stream[k] = huf_stream_size(bits[k]);
        comp += p.stream[k];
    }
    const uint32_t size = lit_header_huf_size(p.n, comp) + comp;
    if (size < p.size) {
        p.mode = kLitHuf;
        p.comp = comp;
        p.size = size;
    }
}

// The section's bytes before its payload: header (and for Huffman the
// description and the jump table).  Returns their length; the payload (raw
// bytes, the RLE byte, or the streams back to back) follows.
ZENC_HD uint32_t lit_write_head(const LitPlan &p, const HufCode &h, uint8_t *dst)
{
    if (p.mode != kLitHuf)
        return lit_header_plain(dst, p.mode, p.n);
    uint32_t at = lit_header_huf(dst, p.n, p.comp);
    at += huf_write_desc(h, dst + at);
    if (huf_streams(p.n) == 4)
        for (int k = 0; k < 3; k++) {
            dst[at++] = (uint8_t)p.stream[k];
            dst[at++] = (uint8_t)(p.stream[k] >> 8);
        }
    return at;
}

// ------------------------------------------------------------ sequence codes
// base | extra bits << 24, as the decoders' tables
ZENC_HD uint32_t ll_code_info(uint32_t c)
{
    const uint32_t t[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,
                            16 | 1u << 24, 18 | 1u << 24, 20 | 1u << 24, 22 | 1u << 24, 24 | 2u << 24,
                            28 | 2u << 24, 32 | 3u << 24, 40 | 3u << 24, 48 | 4u << 24, 64 | 6u << 24,
                            128 | 7u << 24, 256 | 8u << 24, 512 | 9u << 24, 1024 | 10u << 24, 2048 | 11u << 24,
                            4096 | 12u << 24, 8192 | 13u << 24, 16384 | 14u << 24, 32768 | 15u << 24,
                            65536 | 16u << 24};
    return t[c];
}

ZENC_HD uint32_t ml_code_info(uint32_t c)
{
    const uint32_t t[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25,
                            26, 27, 28, 29, 30, 31, 32, 33, 34, 35 | 1u << 24, 37 | 1u << 24, 39 | 1u << 24,
                            41 | 1u << 24, 43 | 2u << 24, 47 | 2u << 24, 51 | 3u << 24, 59 | 3u << 24,
                            67 | 4u << 24, 83 | 4u << 24, 99 | 5u << 24, 131 | 7u << 24, 259 | 8u << 24,
                            515 | 9u << 24, 1027 | 10u << 24, 2051 | 11u << 24, 4099 | 12u << 24,
                            8195 | 13u << 24, 16387 | 14u << 24, 32771 | 15u << 24, 65539 | 16u << 24};
    return t[c];
}

ZENC_HD uint32_t ll_code(uint32_t ll)
{
    if (ll < 16)
        return ll;
    if (ll >= 64)
        return highbit(ll) + 19;
    uint32_t c = 16;
    while (c < 24 && (ll_code_info(c + 1) & 0xFFFFFF) <= ll)
        c++;
    return c;
}

ZENC_HD uint32_t ml_code(uint32_t ml)   // ml >= 3
{
    if (ml < 35)
        return ml - 3;
    if (ml - 3 >= 128)
        return highbit(ml - 3) + 36;
    uint32_t c = 32;
    while (c < 42 && (ml_code_info(c + 1) & 0xFFFFFF) <= ml)
        c++;
    return c;
}

// ---------------------------------------------------------------------- FSE
// Encoding table of one predefined distribution (libzstd's
// FSE_buildCTable_wksp restated): state[] by symbol-sorted cell, and per
// symbol the two deltas of the state step.
struct FseCT {
    uint16_t state[64];
    int32_t dnb[53];   // deltaNbBits
    int32_t dfs[53];   // deltaFindState
    uint32_t log;
};

struct SeqTables {
    FseCT ll, of, ml;
};

ZENC_HD void fse_build(const int8_t *norm, uint32_t nsym, uint32_t log, FseCT &t)
{
    const uint32_t size = 1u << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint8_t sym[64];
    uint32_t cumul[54];
    uint32_t high = size - 1;
    cumul[0] = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        if (norm[s] == -1) {
            cumul[s + 1] = cumul[s] + 1;
            sym[high--] = (uint8_t)s;
        } else {
            cumul[s + 1] = cumul[s] + (uint32_t)norm[s];
        }
    }
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; s++)
        for (int i = 0; i < norm[s]; i++) {
            sym[pos] = (uint8_t)s;
            pos = (pos + step) & mask;
            while (pos > high)
                pos = (pos + step) & mask;
        }
    for (uint32_t u = 0; u < size; u++)
        t.state[cumul[sym[u]]++] = (uint16_t)(size + u);
    uint32_t total = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        if (norm[s] == 0) {
            t.dnb[s] = (int32_t)(((log + 1) << 16) - size);
            t.dfs[s] = 0;
        } else if (norm[s] == -1 || norm[s] == 1) {
            t.dnb[s] = (int32_t)((log << 16) - size);
            t.dfs[s] = (int32_t)total - 1;
            total++;
        } else {
            const uint32_t c = (uint32_t)norm[s];
            const uint32_t max_out = log - highbit(c - 1);
            t.dnb[s] = (int32_t)((max_out << 16) - (c << max_out));
            t.dfs[s] = (int32_t)total - (int32_t)c;
            total += c;
        }
    }
    t.log = log;
}

ZENC_HD void seq_tables_build(SeqTables &T)
{
    const int8_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                           2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    const int8_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                           1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    const int8_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    fse_build(ll, 36, 6, T.ll);
    fse_build(of, 29, 5, T.of);
    fse_build(ml, 53, 6, T.ml);
}

ZENC_HD uint32_t fse_init(const FseCT &t, uint32_t s)
{
    const uint32_t nb = (uint32_t)(t.dnb[s] + (1 << 15)) >> 16;
    const uint32_t v = (nb << 16) - (uint32_t)t.dnb[s];
    return t.state[(int32_t)(v >> nb) + t.dfs[s]];
}

ZENC_HD uint32_t fse_step(const FseCT &t, BitW &b, uint32_t st, uint32_t s)
{
    const uint32_t nb = (uint32_t)((int32_t)st + t.dnb[s]) >> 16;
    bw_add(b, st, nb);
    return t.state[(int32_t)(st >> nb) + t.dfs[s]];
}

// Sequences_Section_Header: the count in its 1 / 2 / 3-byte form and, when
// there are sequences, the modes byte 0 (three predefined tables).
ZENC_HD uint32_t seq_header(uint8_t *dst, uint32_t nseq)
{
    uint32_t at = 0;
    if (nseq < 128) {
        dst[at++] = (uint8_t)nseq;
        if (nseq == 0)
            return at;
    } else if (nseq < 0x7F00) {
        dst[at++] = (uint8_t)((nseq >> 8) + 0x80);
        dst[at++] = (uint8_t)nseq;
    } else {
        dst[at++] = 0xFF;
        dst[at++] = (uint8_t)(nseq - 0x7F00);
        dst[at++] = (uint8_t)((nseq - 0x7F00) >> 8);
    }
    dst[at++] = 0;
    return at;
}

// The whole section into [dst, end): header and the bitstream, sequences
// taken last first (libzstd's ZSTD_encodeSequences order: the decoder reads
// LL, OF, ML states, then per sequence OF / ML / LL extra bits and the LL, ML,
// OF state updates).  Returns its size, or 0 when it does not fit.
ZENC_HD uint32_t seq_section(const SeqTables &T, const Seq *seq, uint32_t nseq, uint8_t *dst, uint8_t *end)
{
    if (end - dst < 4)
        return 0;
    const uint32_t hs = seq_header(dst, nseq);
    if (nseq == 0)
        return hs;
    BitW b;
    bw_init(b, dst + hs, end);
    uint32_t sll = 0, sof = 0, sml = 0;
    for (uint32_t i = nseq; i-- > 0;) {
        const Seq q = seq[i];
        const uint32_t lc = ll_code(q.ll), mc = ml_code(q.ml), ov = q.off + 3, oc = highbit(ov);
        const uint32_t li = ll_code_info(lc), mi = ml_code_info(mc);
        if (i == nseq - 1) {
            sml = fse_init(T.ml, mc);
            sof = fse_init(T.of, oc);
            sll = fse_init(T.ll, lc);
        } else {
            sof = fse_step(T.of, b, sof, oc);
            sml = fse_step(T.ml, b, sml, mc);
            sll = fse_step(T.ll, b, sll, lc);
        }
        bw_add(b, q.ll - (li & 0xFFFFFF), li >> 24);
        bw_add(b, q.ml - (mi & 0xFFFFFF), mi >> 24);
        bw_add(b, ov - (1u << oc), oc);
    }
    bw_add(b, sml, T.ml.log);
    bw_add(b, sof, T.of.log);
    bw_add(b, sll, T.ll.log);
    const uint8_t *e = bw_close(b);
    return e ? (uint32_t)(e - dst) : 0;
}

// ------------------------------------------------------------ block and frame
enum BlockType { kBlockRaw = 0, kBlockRle = 1, kBlockCompressed = 2 };

ZENC_HD void block_header(uint8_t *dst, bool last, uint32_t type, uint32_t size)
{
    const uint32_t v = (last ? 1u : 0u) | type << 1 | size << 3;
    dst[0] = (uint8_t)v;
    dst[1] = (uint8_t)(v >> 8);
    dst[2] = (uint8_t)(v >> 16);
}

// A block of n input bytes whose compressed form takes `comp` bytes (0: none).
ZENC_HD uint32_t block_choice(uint32_t n, bool one_byte_run, uint32_t comp)
{
    if (n > 0 && one_byte_run)
        return kBlockRle;
    return comp != 0 && comp < n ? kBlockCompressed : kBlockRaw;
}

ZENC_HD uint32_t match_hash(uint32_t v)
{
    return (v * 2654435761u) >> (32 - kHashLog);
}

ZENC_HD uint32_t frame_header_size(uint32_t n)
{
    return n < 256 ? 6 : n < 65792 ? 7 : 9;
}

// Frame header of n content bytes; returns its length (6, 7 or 9).
ZENC_HD uint32_t frame_header(uint8_t *dst, uint32_t n, bool checksum)
{
    const uint32_t fcs = n < 256 ? 0 : n < 65792 ? 1 : 2;
    dst[0] = 0x28;
    dst[1] = 0xB5;
    dst[2] = 0x2F;
    dst[3] = 0xFD;
    dst[4] = (uint8_t)(fcs << 6 | 1u << 5 | (checksum ? 1u << 2 : 0u));
    if (fcs == 0) {
        dst[5] = (uint8_t)n;
        return 6;
    }
    if (fcs == 1) {
        dst[5] = (uint8_t)(n - 256);
        dst[6] = (uint8_t)((n - 256) >> 8);
        return 7;
    }
    for (int i = 0; i < 4; i++)
        dst[5 + i] = (uint8_t)(n >> (8 * i));
    return 9;
}

ZENC_HD uint32_t frame_blocks(uint32_t n)
{
    return n == 0 ? 1 : (n + kZBlock - 1) / kZBlock;
}

// All blocks Raw: header, 3 bytes per block, the bytes, the checksum.
ZENC_HD uint64_t frame_bound(uint64_t n)
{
    const uint64_t nb = n == 0 ? 1 : (n + kZBlock - 1) / kZBlock;
    return (9 + 3 * nb + n + 4 + 15) & ~(uint64_t)15;
}

}   // namespace zenc
}   // namespace zsk
