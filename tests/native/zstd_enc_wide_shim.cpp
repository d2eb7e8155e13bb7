// CPU shim over libzseek_amd/csrc/zstd_enc_wide_dev.h for
// tests/test_zstd_enc_wide.py: the wide match search of the GPU zstd
// compressor (ZSK_ZSTD_FORMAT_FULL_WIDE) restated serially -- one table for the
// whole frame, a block's search run over what the earlier blocks left in it --
// behind the full shim's format layer (included below with its exports and the
// subset's, so one library holds the three formats).
#include "zstd_enc_full_shim.cpp"

#include "../../libzseek_amd/csrc/zstd_enc_wide_dev.h"

namespace {

// wave_match (zstd_enc_shim.cpp) on block s[b0, b0 + bn) of the frame s over
// the frame's table: the same steps, wide_hash, and nothing cleared.
void wave_match_wide(const uint8_t *s, uint32_t b0, uint32_t bn, std::vector<uint32_t> &tab, std::vector<Seq> &seq)
{
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
            hsh[i] = wide_hash(v);
            cand[i] = tab[hsh[i]];
            if (hit == 64 && cand[i] && rd4(s + cand[i] - 1) == v)
                hit = i;
        }
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

uint32_t zenc_wide_min_frame(void)
{
    return kWideMinFrame;
}

uint32_t zenc_wide_hash_log(void)
{
    return kWideHashLog;
}

// The (ll, ml, off) triples the wide search gives block by block: seq3 (may be
// null) takes them, nseq one count per block.  Returns the triples' number.
// A frame of at most kWideMinFrame bytes gets the full format's search.
uint32_t zenc_wide_sequences(const uint8_t *content, uint32_t n, uint32_t *seq3, uint32_t *nseq)
{
    std::vector<uint32_t> tab(wide_frame(n) ? 1u << kWideHashLog : 0, 0);
    std::vector<Seq> seq;
    uint32_t total = 0;
    for (uint32_t b = 0; b < frame_blocks(n); b++) {
        const uint32_t b0 = b * kZBlock, bn = n - b0 < kZBlock ? n - b0 : kZBlock;
        seq.clear();
        if (!wide_frame(n)) {
            wave_match(content, b0, bn, seq);
        } else {
            // an empty block, or one the kernel writes RLE before it searches, leaves the table alone
            bool run = bn > 0;
            for (uint32_t i = 1; i < bn && run; i++)
                run = content[b0 + i] == content[b0];
            if (bn > 0 && !run)
                wave_match_wide(content, b0, bn, tab, seq);
        }
        nseq[b] = (uint32_t)seq.size();
        for (const Seq &s : seq) {
            if (seq3) {
                seq3[3 * total] = s.ll;
                seq3[3 * total + 1] = s.ml;
                seq3[3 * total + 2] = s.off;
            }
            total++;
        }
    }
    return total;
}

// The whole pipeline in the wide format: the search above, then
// zenc_full_frame's path.
int64_t zenc_wide_compress(const uint8_t *content, uint32_t n, int checksum, uint8_t *dst, uint64_t cap)
{
    if (!wide_frame(n))
        return zenc_full_compress(content, n, checksum, dst, cap);
    std::vector<uint32_t> nseq(frame_blocks(n));
    std::vector<uint32_t> seq3(3 * (size_t)zenc_wide_sequences(content, n, nullptr, nseq.data()) + 3);
    zenc_wide_sequences(content, n, seq3.data(), nseq.data());
    return zenc_full_frame(content, n, seq3.data(), nseq.data(), checksum, dst, cap, nullptr);
}

}   // extern "C"
