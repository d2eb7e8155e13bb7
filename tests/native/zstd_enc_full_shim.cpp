// CPU shim over libzseek_amd/csrc/zstd_enc_full_dev.h for
// tests/test_zstd_enc_full.py: the full format of the GPU zstd compressor
// driven serially, block by block as the full kernel of zstd_compress.hip
// assembles it -- a frame from chosen literals and sequences, the whole
// pipeline behind the subset shim's serial restatement of the match search
// (included below with its exports, so one library holds both formats), the
// offset values chosen for a list of sequences, and the code lengths alone.
#include "zstd_enc_shim.cpp"

#include "../../libzseek_amd/csrc/zstd_enc_full_dev.h"

namespace {

// One block in the full format.  seq[].off come in as offsets and leave as
// the offset values the block chose; rep is the frame's history, which only a
// block written Compressed moves on.
uint32_t encode_block_full(const SeqTables &T, Reps &rep, const uint8_t *in, uint32_t n, bool last,
                           const uint8_t *lit, uint32_t nlit, Seq *seq, uint32_t nseq, uint8_t *dst)
{
    bool run = n > 0;
    for (uint32_t i = 1; i < n && run; i++)
        run = in[i] == in[0];
    uint32_t comp = 0;
    uint8_t *body = dst + 3, *end = body + n;
    Reps next = rep;
    if (!run && n > 0) {
        seq_offsets(next, seq, nseq);
        uint32_t count[kHufSymsF] = {0}, ws[kHufWorkWordsF], dlen = 0;
        uint8_t desc[kHufDescMax];
        for (uint32_t i = 0; i < nlit; i++)
            count[lit[i]]++;
        HufCodeF h;
        FseCT wt;
        LitPlan p;
        if (lit_wants_huf_f(count, nlit, p)) {
            huf_lengths_f(count, h, ws);
            dlen = h.max_bits ? huf_desc_f(h, wt, desc) : 0;
            if (dlen) {
                uint64_t bits[4] = {0, 0, 0, 0};
                const uint32_t ns = huf_streams(nlit), seg = huf_segment(nlit);
                for (uint32_t i = 0; i < nlit; i++)
                    bits[ns == 4 ? (i / seg) : 0] += h.len[lit[i]];
                lit_plan_huf_f(dlen, bits, p);
            }
        }
        if (p.size + 1 < n) {
            uint32_t at = lit_write_head_f(p, desc, dlen, body);
            if (p.mode == kLitRaw) {
                memcpy(body + at, lit, nlit);
            } else if (p.mode == kLitRle) {
                body[at] = lit[0];
            } else {
                const uint32_t ns = huf_streams(nlit), seg = huf_segment(nlit);
                for (uint32_t k = 0; k < ns; k++) {
                    const uint32_t a = ns == 4 ? k * seg : 0, b = ns == 4 && k < 3 ? a + seg : nlit;
                    const uint32_t w = huf_encode_stream_f(h, lit + a, b - a, body + at, body + at + p.stream[k]);
                    if (w != p.stream[k])
                        return 0xFFFFFFFFu;   // the plan and the encode disagree
                    at += w;
                }
            }
            uint32_t hist[3][64];
            memset(hist, 0, sizeof(hist));
            for (uint32_t i = 0; i < nseq; i++) {
                hist[0][ll_code(seq[i].ll)]++;
                hist[1][highbit(seq[i].off)]++;
                hist[2][ml_code(seq[i].ml)]++;
            }
            std::vector<SeqWork> W(1);
            SeqPlan sp;
            seq_plan(hist, nseq, T, W[0], sp);
            const uint32_t s = seq_section_f(sp, seq, nseq, body + p.size, end);
            comp = s ? p.size + s : 0;
        }
    } else {
        for (uint32_t i = 0; i < nseq; i++)
            seq[i].off = 0;   // (no offset value was chosen)
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
    rep = next;
    block_header(dst, last, type, comp);
    return 3 + comp;
}

}   // namespace

extern "C" {

uint32_t zenc_full_custom_min(void)
{
    return kSeqCustomMin;
}

// count[256] -> len[256], code[256]; returns max_bits (0: no code)
uint32_t zenc_full_huf_lengths(const uint32_t *count, uint8_t *len, uint16_t *code)
{
    uint32_t ws[kHufWorkWordsF];
    HufCodeF h;
    huf_lengths_f(count, h, ws);
    memcpy(len, h.len, sizeof(h.len));
    memcpy(code, h.code, sizeof(h.code));
    return h.max_bits;
}

// The offset values of n (ll, ml, off) triples under one history from 1, 4, 8.
void zenc_full_offsets(const uint32_t *seq3, uint32_t n, uint32_t *ofv)
{
    Reps h;
    reps_init(h);
    for (uint32_t i = 0; i < n; i++)
        ofv[i] = rep_code(h, seq3[3 * i], seq3[3 * i + 2]);
}

// zenc_frame in the full format.  ofv (may be null) takes, per sequence, the
// offset value its block chose -- whether or not the block was then written
// Compressed; 0 in a block that was never encoded (empty, or a one-byte run).
int64_t zenc_full_frame(const uint8_t *content, uint32_t n, const uint32_t *seq3, const uint32_t *nseq, int checksum,
                        uint8_t *dst, uint64_t cap, uint32_t *ofv)
{
    if (cap < frame_bound(n))
        return -2;
    SeqTables T;
    seq_tables_build(T);
    Reps rep;
    reps_init(rep);
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
        const uint32_t w = encode_block_full(T, rep, content + b0, bn, b + 1 == nb, lit.data(), nlit, seq.data(),
                                             (uint32_t)seq.size(), dst + at);
        if (w == 0xFFFFFFFFu)
            return -3;
        if (ofv)
            for (const Seq &s : seq)
                *ofv++ = s.off;
        at += w;
    }
    if (checksum) {
        const uint32_t x = (uint32_t)zsk::xxh64(content, n);
        memcpy(dst + at, &x, 4);
        at += 4;
    }
    return at;
}

// The whole pipeline in the full format: the subset's match search, then
// zenc_full_frame's path.
int64_t zenc_full_compress(const uint8_t *content, uint32_t n, int checksum, uint8_t *dst, uint64_t cap)
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
    return zenc_full_frame(content, n, seq3.data(), nseq.data(), checksum, dst, cap, nullptr);
}

}   // extern "C"
