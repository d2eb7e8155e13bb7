// zstd_enc_full_dev.h — the full format of the GPU zstd compressor
// (ZSK_ZSTD_FORMAT_FULL), beside the subset of zstd_enc_dev.h, whose functions
// it uses and leaves as they are.  Host and device compile the same functions:
// the full kernel of zstd_compress.hip calls them from lanes, and
// tests/native/zstd_enc_full_shim.cpp drives them serially on the CPU.
// Integer arithmetic only, so both give the same bytes.
//
// A full frame differs from a subset frame (zstd_enc_dev.h) in four ways; the
// frame header, the 128 KiB blocks, the block-type rule, the stream count at
// 256 literals, the order of the sequence bitstream and the match search are
// the subset's.
//   literals  Huffman over all 256 byte values: huf_lengths' construction and
//             ties (by symbol value), lengths <= 11.  The tree description is
//             the smaller of the two legal forms, direct on a tie:
//               direct  4-bit weights, legal when at most 128 are listed
//               FSE     a header byte < 128 (the description's size), an FSE
//                       description of the weights' distribution (accuracy
//                       log <= 6, the rule of fse_pick_log) and the weights
//                       walked by two interleaved states, last weight first
//                       (RFC 8878 4.2.1.1; libzstd's HUF_writeCTable)
//             Neither legal -- all listed weights equal, which FSE cannot
//             describe, or 128 bytes or more -- or Huffman not smaller:
//             Raw (RLE for one repeated byte), as in the subset.
//   tables    LL, OF and ML each Predefined (mode 0), RLE (mode 1: every
//             sequence of the block has the same code) or FSE_Compressed
//             (mode 2), chosen per block and per table:
//               * fewer than kSeqCustomMin (8) sequences: all Predefined
//               * accuracy log: fse_pick_log(nseq, largest code present, max)
//                 with max 9 / 8 / 9 -- highbit(nseq - 1) - 2, at most max, at
//                 least min(highbit(nseq) + 1, highbit(largest code) + 2), at
//                 least 5
//               * normalisation (fse_normalize): a count with count * size <
//                 total is "less than one" (-1); the others round
//                 count * size / total half up; a shortfall goes to the
//                 largest share (the lowest symbol on a tie), an excess is
//                 taken one at a time from whichever share is the largest
//               * cost in 1/256 bit: description bytes * 8 * 256, plus the
//                 accuracy log (the final state), plus per sequence
//                 log * 256 - log2_q8(share); Predefined has no description,
//                 RLE is its one byte and nothing per sequence.  The
//                 cheapest wins, Predefined on a tie (RLE and FSE_Compressed
//                 never meet: one code, or more than one).
//   offsets   repeat codes: rep_code below, greedy, one history per frame
//             (1, 4, 8 at its start), carried from block to block and
//             committed only by a block that is written Compressed.
// Not written: matches into earlier blocks, Repeat_Mode or treeless tables,
// dictionaries, frames above 4 MiB, a level parameter.
#pragma once

#include "zstd_enc_dev.h"

namespace zsk {
namespace zenc {

constexpr uint32_t kHufSymsF = 256;
constexpr uint32_t kHufWorkWordsF = 4 * kHufSymsF;   // huf_lengths_sorted's ws
constexpr uint32_t kHufDescMax = 132;                // a description: header byte + < 128
constexpr uint32_t kWeightSyms = 12;                 // weights 0..11
constexpr uint32_t kSeqCustomMin = 8;                // sequences from which RLE / FSE_Compressed are weighed
constexpr uint32_t kNcountMax = 96;                  // an FSE description: 4 + 53 * (10 + 2) bits at most

enum SeqMode { kSeqPredefined = 0, kSeqRle = 1, kSeqFse = 2 };

// Alphabet and largest accuracy log of table t = 0, 1, 2: LL, OF, ML.
ZENC_HD uint32_t seq_syms(uint32_t t)
{
    return t == 0 ? 36 : t == 1 ? 32 : 53;
}

ZENC_HD uint32_t seq_max_log(uint32_t t)
{
    return t == 1 ? 8 : 9;
}

// Forward (low bit first) streams -- the FSE descriptions -- are BitW's bytes
// without the final-bit marker.
ZENC_HD uint8_t *bw_flush(BitW &b)
{
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
struct HufCodeF {
    uint8_t len[kHufSymsF];
    uint16_t code[kHufSymsF];
    uint32_t max_sym;
    uint32_t max_bits;
};

// The sorted symbols' place in huf_lengths_sorted's ws.
ZENC_HD uint8_t *huf_order(uint32_t *ws)
{
    return reinterpret_cast<uint8_t *>(ws + 3 * kHufSymsF);
}

// Symbol s's place among the present symbols by (count, value): the sort of
// huf_lengths, one symbol at a time (the kernel gives every lane four).
ZENC_HD uint32_t huf_rank(const uint32_t *count, uint32_t s)
{
    const uint32_t c = count[s];
    uint32_t r = 0;
    for (uint32_t t = 0; t < kHufSymsF; t++) {
        const uint32_t ct = count[t];
        r += (ct != 0 && (ct < c || (ct == c && t < s))) ? 1u : 0u;
    }
    return r;
}

// huf_lengths over 256 symbols, the sort done: huf_order(ws) holds the present
// symbols by (count, value).  The same tree, limit and repair, tie by tie.
ZENC_HD void huf_lengths_sorted(const uint32_t *count, HufCodeF &h, uint32_t *ws)
{
    uint32_t *w = ws;                                                   // node weights, 2n
    uint16_t *par = reinterpret_cast<uint16_t *>(ws + 2 * kHufSymsF);   // 2n
    const uint8_t *order = huf_order(ws);                               // n
    uint8_t *depth = huf_order(ws) + kHufSymsF;                         // 2n
    uint32_t n = 0;
    h.max_sym = 0;
    h.max_bits = 0;
    for (uint32_t s = 0; s < kHufSymsF; s++) {
        h.len[s] = 0;
        h.code[s] = 0;
        if (count[s] != 0) {
            h.max_sym = s;
            n++;
        }
    }
    if (n < 2)
        return;
    for (uint32_t i = 0; i < n; i++)
        w[i] = count[order[i]];
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
    uint32_t K = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (depth[i] > kHufMaxBits)
            depth[i] = (uint8_t)kHufMaxBits;
        K += 1u << (kHufMaxBits - depth[i]);
    }
    const uint32_t full = 1u << kHufMaxBits;
    while (K > full) {
        uint32_t i = 0;
        while (i < n && depth[i] >= kHufMaxBits)
            i++;
        if (i == n)   // (n <= 256 < 2^kHufMaxBits symbols: never)
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
        if (i >= n)
            break;
        K += 1u << (kHufMaxBits - depth[i]);
        depth[i]--;
    }
    uint32_t mb = 0, per[kHufMaxBits + 1] = {0};
    for (uint32_t i = 0; i < n; i++) {
        h.len[order[i]] = depth[i];
        per[depth[i]]++;
        mb = depth[i] > mb ? depth[i] : mb;
    }
    h.max_bits = mb;
    // canonical codes by zstd's weight rule, as huf_lengths: cells by
    // descending length, then by symbol value
    uint32_t start[kHufMaxBits + 1] = {0}, pos = 0;
    for (uint32_t l = mb; l >= 1; l--) {
        start[l] = pos;
        pos += per[l] << (mb - l);
    }
    for (uint32_t s = 0; s <= h.max_sym; s++) {
        const uint32_t l = h.len[s];
        if (l) {
            h.code[s] = (uint16_t)(start[l] >> (mb - l));
            start[l] += 1u << (mb - l);
        }
    }
}

// Sort and lengths on one lane (the shim, and tests of the lengths alone).
ZENC_HD void huf_lengths_f(const uint32_t *count, HufCodeF &h, uint32_t *ws)
{
    uint8_t *order = huf_order(ws);
    for (uint32_t s = 0; s < kHufSymsF; s++)
        if (count[s] != 0)
            order[huf_rank(count, s)] = (uint8_t)s;
    huf_lengths_sorted(count, h, ws);
}

ZENC_HD uint32_t huf_weight(const HufCodeF &h, uint32_t s)
{
    return h.len[s] ? h.max_bits + 1 - h.len[s] : 0;
}

// ---------------------------------------------------------------------- FSE
// 8 fractional bits of log2(v), v >= 1: the mantissa's fraction f, plus
// 88 * f * (1 - f) / 256 for the curve (off by less than 0.01 bit).
ZENC_HD uint32_t log2_q8(uint32_t v)
{
    const uint32_t hb = highbit(v);
    const uint32_t f = (uint32_t)((((uint64_t)v << 8) >> hb) - 256);
    return (hb << 8) + f + ((88 * f * (256 - f)) >> 16);
}

// The accuracy log of a table for `total` symbols, the largest present one
// `max_sym`: libzstd's FSE_optimalTableLog rule.
ZENC_HD uint32_t fse_pick_log(uint32_t total, uint32_t max_sym, uint32_t max_log)
{
    const uint32_t hb = highbit(total - 1);   // total >= 2
    uint32_t log = hb >= 2 ? hb - 2 : 0;
    const uint32_t a = highbit(total) + 1, b = highbit(max_sym ? max_sym : 1) + 2, floor = a < b ? a : b;
    if (log < floor)
        log = floor;
    if (log < 5)
        log = 5;
    return log < max_log ? log : max_log;
}

// count[0..nsym) of sum total (at least two symbols present) -> shares of
// 1 << log; -1: "less than one", which takes one cell.
ZENC_HD void fse_normalize(const uint32_t *count, uint32_t nsym, uint32_t total, uint32_t log, int16_t *norm)
{
    const uint32_t size = 1u << log;
    uint32_t sum = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        const uint64_t c = count[s];
        if (c == 0) {
            norm[s] = 0;
        } else if (c * size < total) {
            norm[s] = -1;
            sum += 1;
        } else {
            norm[s] = (int16_t)((2 * c * size + total) / (2 * (uint64_t)total));
            sum += (uint32_t)norm[s];
        }
    }
    while (sum != size) {
        uint32_t big = 0;
        for (uint32_t s = 1; s < nsym; s++)
            if (norm[s] > norm[big])
                big = s;
        if (sum < size) {
            norm[big] = (int16_t)(norm[big] + (int16_t)(size - sum));
            sum = size;
        } else {
            norm[big]--;
            sum--;
        }
    }
}

// The table description of RFC 8878 4.1.1 (libzstd's FSE_writeNCount) for
// norm[0..nsym), nsym one past the last present symbol.  Its size; 0: no room.
ZENC_HD uint32_t fse_write_ncount(const int16_t *norm, uint32_t nsym, uint32_t log, uint8_t *dst, uint8_t *end)
{
    BitW b;
    bw_init(b, dst, end);
    bw_add(b, log - 5, 4);
    int32_t remaining = (int32_t)(1u << log) + 1, threshold = (int32_t)(1u << log);
    uint32_t nb = log + 1, s = 0;
    bool prev0 = false;
    while (s < nsym && remaining > 1) {
        if (prev0) {
            uint32_t start = s;
            while (s < nsym && norm[s] == 0)
                s++;
            if (s == nsym)
                break;
            while (s >= start + 3) {
                bw_add(b, 3, 2);
                start += 3;
            }
            bw_add(b, s - start, 2);
        }
        int32_t c = norm[s++];
        const int32_t mx = 2 * threshold - 1 - remaining;
        remaining -= c < 0 ? -c : c;
        c++;
        if (c >= threshold)
            c += mx;
        bw_add(b, (uint32_t)c, nb - (c < mx ? 1u : 0u));
        prev0 = c == 1;
        if (remaining < 1)
            return 0;
        while (remaining < threshold) {
            nb--;
            threshold >>= 1;
        }
    }
    if (remaining != 1)
        return 0;
    const uint8_t *e = bw_flush(b);
    return e ? (uint32_t)(e - dst) : 0;
}

// An encoding table of up to 512 cells: fse_build with the spread's scratch
// (sym, 1 << log bytes) handed in.
struct FseCTF {
    uint16_t state[1u << 9];
    int32_t dnb[53];
    int32_t dfs[53];
    uint32_t log;
};

ZENC_HD void fse_build_f(const int16_t *norm, uint32_t nsym, uint32_t log, FseCTF &t, uint8_t *sym)
{
    const uint32_t size = 1u << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
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

// A table as the sequence encoder sees it: a predefined FseCT, an FseCTF, or
// (log 0) the one state of an RLE table, which takes no bits.
struct FseView {
    const uint16_t *state;
    const int32_t *dnb;
    const int32_t *dfs;
    uint32_t log;
};

ZENC_HD uint32_t fse_init_v(const FseView &t, uint32_t s)
{
    if (t.log == 0)
        return 0;
    const uint32_t nb = (uint32_t)(t.dnb[s] + (1 << 15)) >> 16;
    const uint32_t v = (nb << 16) - (uint32_t)t.dnb[s];
    return t.state[(int32_t)(v >> nb) + t.dfs[s]];
}

ZENC_HD uint32_t fse_step_v(const FseView &t, BitW &b, uint32_t st, uint32_t s)
{
    if (t.log == 0)
        return 0;
    const uint32_t nb = (uint32_t)((int32_t)st + t.dnb[s]) >> 16;
    bw_add(b, st, nb);
    return t.state[(int32_t)(st >> nb) + t.dfs[s]];
}

// --------------------------------------------------- the tree's description
// The listed weights (symbols 0 .. max_sym - 1) FSE-coded into [dst, end):
// the table description, then one backward stream in which two states take
// turns -- the even-numbered weights on the first, the odd ones on the
// second, last weight first, the second state's final value below the
// first's.  The decoder's walk ends where the state of the last weight but
// one reads past the stream: fse_init picks a state that reads a bit.
// Returns the bytes; 0: fewer than two weights, all alike, or no room.
ZENC_HD uint32_t huf_weights_fse(const HufCodeF &h, FseCT &t, uint8_t *dst, uint8_t *end)
{
    const uint32_t n = h.max_sym;
    if (n < 2)
        return 0;
    uint32_t cnt[kWeightSyms] = {0}, top = 0;
    for (uint32_t s = 0; s < n; s++)
        cnt[huf_weight(h, s)]++;
    for (uint32_t w = 0; w < kWeightSyms; w++) {
        if (cnt[w] == n)
            return 0;
        if (cnt[w])
            top = w;
    }
    const uint32_t log = fse_pick_log(n, top, 6);
    int16_t norm[kWeightSyms];
    int8_t norm8[kWeightSyms];
    fse_normalize(cnt, kWeightSyms, n, log, norm);
    for (uint32_t w = 0; w < kWeightSyms; w++)
        norm8[w] = (int8_t)norm[w];
    const uint32_t at = fse_write_ncount(norm, top + 1, log, dst, end);
    if (at == 0)
        return 0;
    fse_build(norm8, kWeightSyms, log, t);
    BitW b;
    bw_init(b, dst + at, end);
    uint32_t st[2] = {0, 0};
    bool live[2] = {false, false};
    for (uint32_t i = n; i-- > 0;) {
        const uint32_t k = i & 1, w = huf_weight(h, i);
        if (!live[k]) {
            st[k] = fse_init(t, w);
            live[k] = true;
        } else {
            st[k] = fse_step(t, b, st[k], w);
        }
    }
    bw_add(b, st[1], log);
    bw_add(b, st[0], log);
    const uint8_t *e = bw_close(b);
    return e ? (uint32_t)(e - dst) : 0;
}

// The description into dst[0..kHufDescMax): the smaller legal form, direct on
// a tie.  Its size; 0: neither form is legal.
ZENC_HD uint32_t huf_desc_f(const HufCodeF &h, FseCT &t, uint8_t *dst)
{
    const uint32_t n = h.max_sym;
    const uint32_t direct = n >= 1 && n <= 128 ? 1 + (n + 1) / 2 : 0;
    const uint32_t body = huf_weights_fse(h, t, dst + 1, dst + 128);   // < 128 bytes
    if (direct != 0 && (body == 0 || direct <= 1 + body)) {
        dst[0] = (uint8_t)(127 + n);
        for (uint32_t s = 0; s < n; s += 2)
            dst[1 + s / 2] = (uint8_t)(huf_weight(h, s) << 4 | (s + 1 < n ? huf_weight(h, s + 1) : 0));
        return direct;
    }
    if (body == 0)
        return 0;
    dst[0] = (uint8_t)body;
    return 1 + body;
}

ZENC_HD uint32_t huf_encode_stream_f(const HufCodeF &h, const uint8_t *lit, uint32_t n, uint8_t *dst, uint8_t *end)
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

// ----------------------------------------------------------------- literals
// Step 1, from the 256-bin histogram: RLE, Raw for certain, or "try Huffman"
// (the caller then sorts, builds the lengths and the description).
ZENC_HD bool lit_wants_huf_f(const uint32_t *count, uint32_t n, LitPlan &p)
{
    p.n = n;
    p.comp = 0;
    p.mode = kLitRaw;
    p.size = lit_header_plain_size(n) + n;
    if (n == 0)
        return false;
    uint32_t distinct = 0;
    for (uint32_t s = 0; s < kHufSymsF && distinct < 2; s++)
        distinct += count[s] != 0;
    if (distinct == 1) {
        p.mode = kLitRle;
        p.size = lit_header_plain_size(n) + 1;
        return false;
    }
    return n >= 8;   // (as the subset: never smaller below)
}

// Step 2, from the description's size and the streams' code bits.
ZENC_HD void lit_plan_huf_f(uint32_t desc, const uint64_t *bits, LitPlan &p)
{
    const uint32_t ns = huf_streams(p.n);
    uint32_t comp = desc + (ns == 4 ? 6 : 0);
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

ZENC_HD uint32_t lit_write_head_f(const LitPlan &p, const uint8_t *desc, uint32_t desc_size, uint8_t *dst)
{
    if (p.mode != kLitHuf)
        return lit_header_plain(dst, p.mode, p.n);
    uint32_t at = lit_header_huf(dst, p.n, p.comp);
    for (uint32_t i = 0; i < desc_size; i++)
        dst[at++] = desc[i];
    if (huf_streams(p.n) == 4)
        for (int k = 0; k < 3; k++) {
            dst[at++] = (uint8_t)p.stream[k];
            dst[at++] = (uint8_t)(p.stream[k] >> 8);
        }
    return at;
}

// ----------------------------------------------------------- repeat offsets
struct Reps {
    uint32_t r[3];
};

ZENC_HD void reps_init(Reps &h)
{
    h.r[0] = 1;
    h.r[1] = 4;
    h.r[2] = 8;
}

// The offset value of a match at `off` behind `ll` literals, and the history
// after it (RFC 8878 3.1.1.5).  With literals the three repeat offsets are
// values 1, 2, 3; without, the second and third are 1 and 2, the first minus
// one (when not 0) is 3, and the first itself is coded plain.
ZENC_HD uint32_t rep_code(Reps &h, uint32_t ll, uint32_t off)
{
    const uint32_t r0 = h.r[0], r1 = h.r[1], r2 = h.r[2];
    if (ll != 0) {
        if (off == r0)
            return 1;
        if (off == r1) {
            h.r[0] = r1;
            h.r[1] = r0;
            return 2;
        }
        if (off == r2) {
            h.r[0] = r2;
            h.r[1] = r0;
            h.r[2] = r1;
            return 3;
        }
    } else {
        if (off == r1) {
            h.r[0] = r1;
            h.r[1] = r0;
            return 1;
        }
        if (off == r2) {
            h.r[0] = r2;
            h.r[1] = r0;
            h.r[2] = r1;
            return 2;
        }
        if (r0 - 1 != 0 && off == r0 - 1) {
            h.r[0] = r0 - 1;
            h.r[1] = r0;
            h.r[2] = r1;
            return 3;
        }
    }
    h.r[0] = off;
    h.r[1] = r0;
    h.r[2] = r1;
    return off + 3;
}

// A block's offsets into offset values, in place and in order (one lane).
ZENC_HD void seq_offsets(Reps &h, Seq *seq, uint32_t nseq)
{
    for (uint32_t i = 0; i < nseq; i++)
        seq[i].off = rep_code(h, seq[i].ll, seq[i].off);
}

// ---------------------------------------------------------- sequence tables
ZENC_HD int32_t seq_predef_norm(uint32_t table, uint32_t s)
{
    const int8_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                           2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    const int8_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                           1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    const int8_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    return table == 0 ? ll[s] : table == 2 ? ml[s] : s < 29 ? of[s] : 0;
}

// seq_tables_build from seq_predef_norm: the same tables.  The full kernel has
// its own builder so that the subset kernel stays seq_tables_build's only
// caller and is compiled as it was.
ZENC_HD void seq_tables_build_f(SeqTables &T)
{
    FseCT *const tab[3] = {&T.ll, &T.of, &T.ml};
    for (uint32_t t = 0; t < 3; t++) {
        int8_t norm[53];
        const uint32_t nsym = t == 1 ? 29 : seq_syms(t);
        for (uint32_t s = 0; s < nsym; s++)
            norm[s] = (int8_t)seq_predef_norm(t, s);
        fse_build(norm, nsym, t == 1 ? 5 : 6, *tab[t]);
    }
}

struct SeqWork {
    FseCTF ct[3];
    int16_t norm[64];
    uint8_t sym[1u << 9];
};

struct SeqPlan {
    FseView v[3];   // LL, OF, ML
    uint8_t mode[3];
    uint8_t dlen[3];
    uint8_t desc[3][kNcountMax];
};

// Cost of `count` under shares `norm` (0: the symbol cannot be coded) of a
// table of 1 << log, in 1/256 bit; ~0: impossible.
ZENC_HD uint64_t seq_cost_add(uint64_t cost, uint32_t count, int32_t norm, uint32_t log)
{
    if (count == 0 || cost == ~0ull)
        return cost;
    if (norm == 0)
        return ~0ull;
    return cost + (uint64_t)count * ((log << 8) - log2_q8(norm < 0 ? 1u : (uint32_t)norm));
}

// The three tables of a block from its code histograms (hist[t][0..64), t =
// LL, OF, ML; the offset codes are those of the offset values): the rule of
// this file's head.
ZENC_HD void seq_plan(const uint32_t (*hist)[64], uint32_t nseq, const SeqTables &P, SeqWork &W, SeqPlan &p)
{
    const FseCT *pre[3] = {&P.ll, &P.of, &P.ml};
    for (uint32_t t = 0; t < 3; t++) {
        p.v[t] = FseView{pre[t]->state, pre[t]->dnb, pre[t]->dfs, pre[t]->log};
        p.mode[t] = kSeqPredefined;
        p.dlen[t] = 0;
        if (nseq < kSeqCustomMin)
            continue;
        uint32_t distinct = 0, top = 0;
        uint64_t cost_pre = (uint64_t)pre[t]->log << 8;
        for (uint32_t s = 0; s < seq_syms(t); s++) {
            if (hist[t][s]) {
                distinct++;
                top = s;
            }
            cost_pre = seq_cost_add(cost_pre, hist[t][s], seq_predef_norm(t, s), pre[t]->log);
        }
        if (distinct == 1) {
            if ((uint64_t)8 << 8 < cost_pre) {
                p.mode[t] = kSeqRle;
                p.dlen[t] = 1;
                p.desc[t][0] = (uint8_t)top;
                p.v[t] = FseView{nullptr, nullptr, nullptr, 0};
            }
            continue;
        }
        const uint32_t log = fse_pick_log(nseq, top, seq_max_log(t));
        fse_normalize(hist[t], top + 1, nseq, log, W.norm);
        const uint32_t dl = fse_write_ncount(W.norm, top + 1, log, p.desc[t], p.desc[t] + kNcountMax);
        if (dl == 0)
            continue;
        uint64_t cost = ((uint64_t)dl * 8 << 8) + ((uint64_t)log << 8);
        for (uint32_t s = 0; s <= top; s++)
            cost = seq_cost_add(cost, hist[t][s], W.norm[s], log);
        if (cost < cost_pre) {
            for (uint32_t s = top + 1; s < seq_syms(t); s++)
                W.norm[s] = 0;
            fse_build_f(W.norm, seq_syms(t), log, W.ct[t], W.sym);
            p.mode[t] = kSeqFse;
            p.dlen[t] = (uint8_t)dl;
            p.v[t] = FseView{W.ct[t].state, W.ct[t].dnb, W.ct[t].dfs, log};
        }
    }
}

// seq_section with the plan's tables; seq[].off holds offset values.
ZENC_HD uint32_t seq_section_f(const SeqPlan &p, const Seq *seq, uint32_t nseq, uint8_t *dst, uint8_t *end)
{
    if (end - dst < 4 + (ptrdiff_t)p.dlen[0] + p.dlen[1] + p.dlen[2])
        return 0;
    uint32_t hs = seq_header(dst, nseq);
    if (nseq == 0)
        return hs;
    dst[hs - 1] = (uint8_t)(p.mode[0] << 6 | p.mode[1] << 4 | p.mode[2] << 2);
    for (uint32_t t = 0; t < 3; t++)
        for (uint32_t i = 0; i < p.dlen[t]; i++)
            dst[hs++] = p.desc[t][i];
    BitW b;
    bw_init(b, dst + hs, end);
    uint32_t sll = 0, sof = 0, sml = 0;
    for (uint32_t i = nseq; i-- > 0;) {
        const Seq q = seq[i];
        const uint32_t lc = ll_code(q.ll), mc = ml_code(q.ml), ov = q.off, oc = highbit(ov);
        const uint32_t li = ll_code_info(lc), mi = ml_code_info(mc);
        if (i == nseq - 1) {
            sml = fse_init_v(p.v[2], mc);
            sof = fse_init_v(p.v[1], oc);
            sll = fse_init_v(p.v[0], lc);
        } else {
            sof = fse_step_v(p.v[1], b, sof, oc);
            sml = fse_step_v(p.v[2], b, sml, mc);
            sll = fse_step_v(p.v[0], b, sll, lc);
        }
        bw_add(b, q.ll - (li & 0xFFFFFF), li >> 24);
        bw_add(b, q.ml - (mi & 0xFFFFFF), mi >> 24);
        bw_add(b, ov - (1u << oc), oc);
    }
    bw_add(b, sml, p.v[2].log);
    bw_add(b, sof, p.v[1].log);
    bw_add(b, sll, p.v[0].log);
    const uint8_t *e = bw_close(b);
    return e ? (uint32_t)(e - dst) : 0;
}

}   // namespace zenc
}   // namespace zsk
