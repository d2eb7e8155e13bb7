// CPU shim over libzseek_amd/csrc/zstd_enc_dev.h for tests/test_zstd_enc.py:
// the format layer of the GPU zstd compressor driven serially -- a frame from
// chosen literals and sequences, the code lengths alone, and the whole
// pipeline behind a serial restatement of the kernel's match search (64
// "lanes" per step, the lowest hitting lane wins, the hash table updated by
// the largest position).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../libzseek_amd/csrc/xxh64_host.h"
#include "../../libzseek_amd/csrc/zstd_enc_dev.h"

using namespace zsk::zenc;

namespace {

// One block from its literals and sequences, as the kernel assembles it.
uint32_t encode_block(const SeqTables &T, const uint8_t *in, uint32_t n, bool last, const uint8_t *lit,
                      uint32_t nlit, const Seq *seq, uint32_t nseq, uint8_t *dst)
{
    bool run = n > 0;
    for (uint32_t i = 1; i < n && run; i++)
        run = in[i] == in[0];
    uint32_t comp = 0;
    uint8_t *body = dst + 3, *end = body + n;
    if (!run && n > 0) {
        uint32_t count[kHufSyms] = {0}, high = 0, ws[kHufWorkWords];
        for (uint32_t i = 0; i < nlit; i++) {
            if (lit[i] < kHufSyms)
                count[lit[i]]++;
            else
                high++;
        }
        HufCode h;
        LitPlan p;
        if (lit_wants_huf(count, high, nlit, h, ws, p)) {
            uint64_t bits[4] = {0, 0, 0, 0};
            const uint32_t ns = huf_streams(nlit), seg = huf_segment(nlit);
            for (uint32_t i = 0; i < nlit; i++)
                bits[ns == 4 ? (i / seg) : 0] += h.len[lit[i]];
            lit_plan_huf(h, bits, p);
        }
        if (p.size + 1 < n) {
            uint32_t at = lit_write_head(p, h, body);
            if (p.mode == kLitRaw) {
                memcpy(body + at, lit, nlit);
            } else if (p.mode == kLitRle) {
                body[at] = lit[0];
            } else {
                const uint32_t ns = huf_streams(nlit), seg = huf_segment(nlit);
                for (uint32_t k = 0; k < ns; k++) {
                    const uint32_t a = ns == 4 ? k * seg : 0, b = ns == 4 && k < 3 ? a + seg : nlit;
                    const uint32_t w = huf_encode_stream(h, lit + a, b - a, body + at, body + at + p.stream[k]);
                    if (w != p.stream[k])
                        return 0xFFFFFFFFu;   // the plan and the encode disagree
                    at += w;
                }
            }
            const uint32_t s = seq_section(T, seq, nseq, body + p.size, end);
            comp = s ? p.size + s : 0;
        }
    }
    const uint32_t type = block_choice(n, run, comp);
    if (type == kBlockRle) {
        block_header(dst, last, type, n);
        dst[3] = in[0];
        return 4;
    }
    if (type == kBlockRaw) {
        block_header(dst, last, type, n);
        memcpy(dst + 3, in, n);
        return 3 + n;
    }
    block_header(dst, last, type, comp);
    return 3 + comp;
}

uint32_t rd4(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

// The kernel's match search on block s[b0, b0 + bn), serially.
void wave_match(const uint8_t *s, uint32_t b0, uint32_t bn, std::vector<Seq> &seq)
{
    std::vector<uint32_t> tab(1u << kHashLog, 0);
    const uint32_t end = b0 + bn;
    uint32_t anchor = b0, base = b0;
    while (base + kMinMatch <= end) {
        uint32_t cand[64], hsh[64], hit = 64;
        for (uint32_t i = 0; i < 64; i++) {
            const uint32_t pos = base + i;
            cand[i] = 0;
            if (pos + 4 > end)
                continue;
            const uint32_t v = rd4(s + pos);
            hsh[i] = match_hash(v);
            cand[i] = tab[hsh[i]];
            if (hit == 64 && cand[i] && rd4(s + cand[i] - 1) == v)
                hit = i;
        }
        // the table takes the step's positions before the next step's start
        auto insert = [&](uint32_t next) {
            for (uint32_t i = 0; i < 64; i++)
                if (base + i + 4 <= end && base + i < next && tab[hsh[i]] < base + i + 1)
                    tab[hsh[i]] = base + i + 1;
        };
        if (hit == 64) {
            insert(base + 64);
            base += 64;
            continue;
        }
        const uint32_t mpos = base + hit, mc = cand[hit] - 1;
        uint32_t ml = 4;
        while (mpos + ml < end && s[mpos + ml] == s[mc + ml])
            ml++;
        insert(mpos + ml);
        seq.push_back(Seq{mpos - anchor, ml, mpos - mc});
        anchor = base = mpos + ml;
    }
}

}   // namespace

extern "C" {

uint32_t zenc_zblock(void)
{
    return kZBlock;
}

uint64_t zenc_frame_bound(uint64_t n)
{
    return frame_bound(n);
}

// count[129] -> len[129], code[129]; returns max_bits (0: no code)
uint32_t zenc_huf_lengths(const uint32_t *count, uint8_t *len, uint16_t *code)
{
    uint32_t ws[kHufWorkWords];
    HufCode h;
    huf_lengths(count, h, ws);
    memcpy(len, h.len, sizeof(h.len));
    memcpy(code, h.code, sizeof(h.code));
    return h.max_bits;
}

// (code, base, extra bits) of a literal length / a match length
void zenc_ll_code(uint32_t ll, uint32_t *out)
{
    const uint32_t c = ll_code(ll), i = ll_code_info(c);
    out[0] = c;
    out[1] = i & 0xFFFFFF;
    out[2] = i >> 24;
}

void zenc_ml_code(uint32_t ml, uint32_t *out)
{
    const uint32_t c = ml_code(ml), i = ml_code_info(c);
    out[0] = c;
    out[1] = i & 0xFFFFFF;
    out[2] = i >> 24;
}

// A frame of content[0..n) whose block b holds nseq[b] of the (ll, ml, off)
// triples in seq, in order; the bytes after a block's last match are its
// trailing literals.  Returns the frame's size; -1: the sequences do not
// describe the content's blocks, -2: cap too small, -3: internal disagreement.
int64_t zenc_frame(const uint8_t *content, uint32_t n, const uint32_t *seq3, const uint32_t *nseq, int checksum,
                   uint8_t *dst, uint64_t cap)
{
    if (cap < frame_bound(n))
        return -2;
    SeqTables T;
    seq_tables_build(T);
    uint32_t at = frame_header(dst, n, checksum != 0);
    const uint32_t nb = frame_blocks(n);
    std::vector<uint8_t> lit(kZBlock);
    std::vector<Seq> seq;
    const uint32_t *q = seq3;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t b0 = b * kZBlock, bn = n - b0 < kZBlock ? n - b0 : kZBlock;
        seq.clear();
        uint32_t pos = b0, nlit = 0;
        for (uint32_t i = 0; i < nseq[b]; i++, q += 3) {
            const Seq s{q[0], q[1], q[2]};
            if (s.ml < 3 || s.off == 0 || (uint64_t)pos + s.ll + s.ml > b0 + bn || s.off > pos + s.ll)
                return -1;
            memcpy(lit.data() + nlit, content + pos, s.ll);
            nlit += s.ll;
            pos += s.ll + s.ml;
            seq.push_back(s);
        }
        memcpy(lit.data() + nlit, content + pos, b0 + bn - pos);
        nlit += b0 + bn - pos;
        const uint32_t w = encode_block(T, content + b0, bn, b + 1 == nb, lit.data(), nlit, seq.data(),
                                        (uint32_t)seq.size(), dst + at);
        if (w == 0xFFFFFFFFu)
            return -3;
        at += w;
    }
    if (checksum) {
        const uint32_t x = (uint32_t)zsk::xxh64(content, n);
        memcpy(dst + at, &x, 4);
        at += 4;
    }
    return at;
}

// The whole pipeline: the match search's restatement, then zenc_frame's path.
int64_t zenc_compress(const uint8_t *content, uint32_t n, int checksum, uint8_t *dst, uint64_t cap)
{
    std::vector<uint32_t> seq3, nseq;
    std::vector<Seq> seq;
    for (uint32_t b = 0; b < frame_blocks(n); b++) {
        const uint32_t b0 = b * kZBlock, bn = n - b0 < kZBlock ? n - b0 : kZBlock;
        seq.clear();
        wave_match(content, b0, bn, seq);
        nseq.push_back((uint32_t)seq.size());
        for (const Seq &s : seq) {
            seq3.push_back(s.ll);
            seq3.push_back(s.ml);
            seq3.push_back(s.off);
        }
    }
    return zenc_frame(content, n, seq3.data(), nseq.data(), checksum, dst, cap);
}

}   // extern "C"
