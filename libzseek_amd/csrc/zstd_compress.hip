// zstd_compress.hip — zstd frame compression on the GPU (gfx950):
// zsk_zstd_compress_frames and zsk_zstd_compress_frames_ex.  The frames are
// valid zstd (RFC 8878) that libzstd decodes to the input; they are not
// libzstd's bytes at any level, and there is one effort level.  Three formats,
// one kernel instantiation each, one launch per call:
//   subset  zstd_enc_dev.h (shared with the CPU shim of tests/test_zstd_enc.py):
//           everything that decides bytes once the matches are known.  It
//           leaves out FSE-compressed Huffman weights (so literals holding a
//           byte above 128 are stored Raw), repeat offsets, custom or repeated
//           tables, frames above 4 MiB.
//   full    zstd_enc_full_dev.h (tests/test_zstd_enc_full.py's shim): Huffman
//           over all 256 byte values with the smaller of the two tree
//           descriptions, a mode per sequence table and block, repeat offsets.
//           Same match search, so the same sequences; see "full" below.
//   wide    zstd_enc_wide_dev.h (tests/test_zstd_enc_wide.py's shim): the full
//           format's layer over another search -- a frame above 16 KiB keeps
//           one table of 2^14 positions, in the scratch, for all its blocks,
//           so matches reach earlier blocks; see "wide" below.
//
// Mapping: one single-wave workgroup per frame, the frame's blocks (kZBlock
// input bytes each) in order, each block independent of the others (but in
// the wide format): a fresh hash table, no matches into earlier blocks.
// Workgroups are persistent (at most kGridMax of them walk the batch), so the
// scratch -- a block's compacted literals and its sequences, the wide format's
// table -- is per workgroup, not per frame.
//   match      the wave looks at 64 positions a step: every lane hashes the 4
//              bytes at its position, reads the table (LDS, positions of
//              earlier steps only) and compares; the lowest lane that matches
//              wins (__ballot), the wave extends the match 256 bytes a round,
//              and the step's positions before the next step's start enter the
//              table by atomicMax -- by value, so the bytes never depend on
//              which lane arrives first
//   literals   histogram by LDS atomics while the literals are compacted; one
//              lane assigns the code lengths; the wave sums each stream's code
//              bits, which fixes the section's layout; four lanes encode the
//              four streams
//   sequences  one lane walks the three FSE states over the predefined
//              tables, which the workgroup builds in LDS once
//   assemble   the block is written where it lands: a block's size is known
//              before the next one starts, so no scan is needed
//   full       after the match search the hash table is dead and the block's
//              work lies over it (PostF).  The offsets become offset values
//              in sequence order (each depends on the history): the wave
//              loads 64 sequences and walks them as one (wave_offsets); it
//              counts the three code histograms by LDS atomics and ranks the
//              256 literal counts (every lane four symbols: the sort of
//              huf_lengths without its quadratic walk on one lane); one lane
//              builds lengths, the tree description, and -- bounded by the
//              alphabets -- normalises, describes and builds the tables it
//              chooses; bit sums, literal copy and the four streams are the
//              subset's.  The frame's offset history sits in LDS and moves on
//              only when a block is written Compressed.
//   wide       the table of a frame above kWideMinFrame bytes is the
//              workgroup's kWideTableBytes of global memory: cleared by the
//              wave, whole, at the frame's start (a persistent workgroup's
//              last frame must leave nothing: an entry past the new frame's
//              length would be a read outside it), then block after block
//              searched over it by the same find_matches, which reads it with
//              global loads and enters positions by a global atomicMax.  An
//              empty block or a one-byte run is written before the search and
//              inserts nothing.  The index is a hash's top 14 bits; a
//              candidate is an earlier position of the same frame.  Smaller
//              frames take the full format's path and are its frames.
// Source bytes are read only inside the frame (a 4-byte read always lies
// within it); nothing is written outside the slot's ZSK_ZSTD_COMPRESS_BOUND.
//
// Algorithmic bytes per frame: n read (+ the literals written and read back)
// + the frame's compressed size written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/zseek_hip.h"
#include "zsk_internal.h"
#include "zstd_enc_dev.h"
#include "zstd_enc_full_dev.h"
#include "zstd_enc_wide_dev.h"

namespace zsk {

namespace {

using namespace zenc;

static_assert(ZSK_ZSTD_COMPRESS_MAX_FRAME == kMaxFrame, "the header's cap");
static_assert(ZSK_ZSTD_COMPRESS_BOUND(0) == 16 && ZSK_ZSTD_COMPRESS_BOUND(kZBlock + 1) == ((9 + 6 + kZBlock + 1 + 4 + 15) & ~15u),
              "the header's bound follows kZBlock");

typedef uint32_t u32_ua __attribute__((aligned(1)));

constexpr uint32_t kGridMax = 1792;                   // workgroups that walk a batch: 7 per CU (LDS)
constexpr uint32_t kSeqMax = kZBlock / kMinMatch;     // sequences a block can hold
constexpr size_t kWgScratch = kZBlock + (size_t)kSeqMax * sizeof(Seq);

// The subset kernel's LDS.
struct Lds {
    uint32_t tab[1u << kHashLog];    // position + 1 by hash; 0: empty
    uint32_t count[kHufSyms + 1];    // literal histogram; [kHufSyms]: bytes above 128
    uint32_t bits[4];                // code bits per Huffman stream
    uint32_t ws[kHufWorkWords];
    HufCode huf;
    SeqTables T;
    LitPlan plan;
    uint32_t wants, comp;
};

// The full kernel's LDS.  Everything a block needs once its matches are found
// lies over the hash table, which is dead by then; within that, the Huffman
// work area and the custom FSE tables, which are not live together, share
// their bytes.  What the match search fills (count) or a frame keeps (T, rep)
// stays outside.
struct PostF {
    union {
        uint32_t ws[kHufWorkWordsF];   // huf_lengths_sorted's
        SeqWork W;                     // seq_plan's: the custom tables
    };
    HufCodeF huf;
    FseCT wt;                          // the weights' table
    uint32_t hist[3][64];              // LL, OF, ML code histograms
    SeqPlan seq;
    uint8_t hdesc[kHufDescMax];        // the tree description
    uint32_t hdesc_len;
};

struct LdsF {
    union {
        uint32_t tab[1u << kHashLog];
        PostF post;
    };
    uint32_t count[kHufSymsF];
    uint32_t bits[4];
    SeqTables T;                       // the predefined tables
    LitPlan plan;
    Reps rep, next;                    // the frame's offset history; after this block
    uint32_t wants, comp;
};
static_assert(sizeof(PostF) <= sizeof(uint32_t) << kHashLog, "the block's work fits in the dead hash table");

__host__ __device__ constexpr size_t align256(size_t v)
{
    return (v + 255) & ~(size_t)255;
}

// The scratch of a call: per workgroup the literals and sequences, then the
// checksum kernel's descriptors and sums -- the subset's and full format's
// whole scratch -- and behind that the wide format's tables, one per workgroup.
__host__ __device__ constexpr size_t wide_tables_at(uint32_t grid, uint32_t nframes)
{
    return align256((size_t)grid * kWgScratch) + align256((size_t)nframes * sizeof(zsk_compress_desc_t)) +
           align256((size_t)nframes * sizeof(uint32_t));
}

__device__ __forceinline__ uint32_t ld4(const uint8_t *p)
{
    return *reinterpret_cast<const u32_ua *>(p);
}

// in[0..n) is one repeated byte (n >= 1).
__device__ __forceinline__ bool one_byte_run(const uint8_t *in, uint32_t n)
{
    const uint32_t lane = threadIdx.x;
    const uint8_t b = in[0];
    for (uint32_t i = 0; i < n; i += 64) {
        const bool differs = i + lane < n && in[i + lane] != b;
        if (__ballot(differs))
            return false;
    }
    return true;
}

// The wide search's table lies in global memory, and is addressed as such.
typedef __attribute__((address_space(1))) uint32_t gu32;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// A position into the match search's table: the largest one stays.  In LDS for
// the subset and full searches; in global memory for the wide one, where the
// workgroup is one wave and owns its table, so only the lanes of one step
// meet, and the barrier that ends the step orders it before the next reads.
template <class TabT>
__device__ __forceinline__ void tab_max(TabT *p, uint32_t v)
{
    if constexpr (std::is_same<TabT, gu32>::value)
        __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        atomicMax(p, v);
}

// Literals s[from, from + len) behind lit[nlit), counted: the subset in bins
// 0..128 and one for the bytes above, the full format in 256.
template <bool kFull>
__device__ __forceinline__ void take_literals(uint32_t *count, const uint8_t *s, uint32_t from, uint32_t len,
                                              uint8_t *lit, uint32_t nlit)
{
    for (uint32_t i = threadIdx.x; i < len; i += 64) {
        const uint32_t c = s[from + i];
        lit[nlit + i] = (uint8_t)c;
        atomicAdd(&count[kFull || c < kHufSyms ? c : kHufSyms], 1u);
    }
}

// The match search of block s[b0, b0 + bn) (the file's head): the literals
// compacted into lit and counted, the sequences into seq.  tab and count are
// cleared by the caller; wave-uniform, and ends on a barrier.  The wide search
// (kLog = kWideHashLog) is the same walk over the frame's table in global
// memory, which the caller cleared at the frame's start: s is the frame, so
// the positions are the frame's already.
template <bool kFull, uint32_t kLog = kHashLog, class TabT = uint32_t>
__device__ __forceinline__ void find_matches(TabT *tab, uint32_t *count, const uint8_t *__restrict__ s,
                                             uint32_t b0, uint32_t bn, uint8_t *__restrict__ lit,
                                             Seq *__restrict__ seq, uint32_t &nseq_out, uint32_t &nlit_out)
{
    const uint32_t lane = threadIdx.x, end = b0 + bn;
    uint32_t anchor = b0, base = b0, nseq = 0, nlit = 0;
    while (base + kMinMatch <= end) {
        const uint32_t pos = base + lane;
        const bool valid = pos + 4 <= end;
        uint32_t v = 0, h = 0, cand = 0;
        if (valid) {
            v = ld4(s + pos);
            h = kLog == kHashLog ? match_hash(v) : wide_hash(v);
            cand = tab[h];
        }
        const bool hit = valid && cand != 0 && ld4(s + cand - 1) == v;
        const uint64_t hits = __ballot(hit);
        if (hits == 0) {
            if (valid)
                tab_max(&tab[h], pos + 1);
            __syncthreads();
            base += 64;
            continue;
        }
        const int hl = __ffsll((unsigned long long)hits) - 1;
        const uint32_t mpos = base + (uint32_t)hl, mc = (uint32_t)__shfl((int)cand, hl, 64) - 1;
        uint32_t ml = 4;
        for (;;) {   // 4 bytes a lane, 256 a round; a lane at the block's end compares what is left
            const uint32_t a = mpos + ml + 4 * lane, c = mc + ml + 4 * lane;
            uint32_t eq = 0;
            if (a + 4 <= end) {
                const uint32_t x = ld4(s + a) ^ ld4(s + c);
                eq = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
            } else {
                while (a + eq < end && s[a + eq] == s[c + eq])
                    eq++;
            }
            const uint64_t stop = __ballot(eq < 4);
            if (stop) {
                const int j = __ffsll((unsigned long long)stop) - 1;
                ml += 4 * (uint32_t)j + (uint32_t)__shfl((int)eq, j, 64);
                break;
            }
            ml += 256;
        }
        const uint32_t next = mpos + ml;
        if (valid && pos < next)
            tab_max(&tab[h], pos + 1);
        const uint32_t ll = mpos - anchor;
        take_literals<kFull>(count, s, anchor, ll, lit, nlit);
        if (lane == 0)
            seq[nseq] = Seq{ll, ml, mpos - mc};
        nseq++;
        nlit += ll;
        anchor = base = next;
        __syncthreads();
    }
    take_literals<kFull>(count, s, anchor, end - anchor, lit, nlit);
    nlit += end - anchor;
    __syncthreads();
    nseq_out = nseq;
    nlit_out = nlit;
}

// Block s[b0, b0 + bn) of the frame s at dst; returns its size with the
// 3-byte header.  Wave-uniform: every lane takes every branch together.
__device__ uint32_t compress_block(Lds &L, const uint8_t *__restrict__ s, uint32_t b0, uint32_t bn, bool last,
                                   uint8_t *__restrict__ dst, uint8_t *__restrict__ lit, Seq *__restrict__ seq)
{
    const uint32_t lane = threadIdx.x;
    if (bn == 0) {
        if (lane == 0)
            block_header(dst, last, kBlockRaw, 0);
        return 3;
    }
    if (one_byte_run(s + b0, bn)) {
        if (lane == 0) {
            block_header(dst, last, block_choice(bn, true, 0), bn);
            dst[3] = s[b0];
        }
        return 4;
    }
    for (uint32_t i = lane; i < (1u << kHashLog); i += 64)
        L.tab[i] = 0;
    for (uint32_t i = lane; i < kHufSyms + 1; i += 64)
        L.count[i] = 0;
    if (lane < 4)
        L.bits[lane] = 0;
    __syncthreads();
    uint32_t nseq, nlit;   // ---- match
    find_matches<false>(L.tab, L.count, s, b0, bn, lit, seq, nseq, nlit);
    // ---- literals: the plan
    if (lane == 0)
        L.wants = lit_wants_huf(L.count, L.count[kHufSyms], nlit, L.huf, L.ws, L.plan) ? 1u : 0u;
    __syncthreads();
    const uint32_t ns = huf_streams(nlit), seg = huf_segment(nlit);
    if (L.wants) {
        for (uint32_t k = 0; k < ns; k++) {
            const uint32_t a = ns == 4 ? k * seg : 0, b = ns == 4 && k < 3 ? a + seg : nlit;
            uint32_t sum = 0;
            for (uint32_t i = a + lane; i < b; i += 64)
                sum += L.huf.len[lit[i]];
            atomicAdd(&L.bits[k], sum);
        }
        __syncthreads();
        if (lane == 0) {
            const uint64_t bits[4] = {L.bits[0], L.bits[1], L.bits[2], L.bits[3]};
            lit_plan_huf(L.huf, bits, L.plan);
        }
        __syncthreads();
    }
    const uint32_t mode = L.plan.mode, lsize = L.plan.size;
    if (lane == 0)
        L.comp = 0;
    uint8_t *const body = dst + 3;
    if (lsize + 1 < bn) {
        // ---- literals and sequences, where they land
        if (lane == 0)
            lit_write_head(L.plan, L.huf, body);
        if (mode == kLitRaw) {
            const uint32_t head = lsize - nlit;
            for (uint32_t i = lane; i < nlit; i += 64)
                body[head + i] = lit[i];
        } else if (mode == kLitRle) {
            if (lane == 0)
                body[lsize - 1] = lit[0];
        } else if (lane < ns) {
            uint32_t off = lsize;   // the streams end the section
            for (uint32_t k = lane; k < ns; k++)
                off -= L.plan.stream[k];
            const uint32_t a = ns == 4 ? lane * seg : 0, b = ns == 4 && lane < 3 ? a + seg : nlit;
            huf_encode_stream(L.huf, lit + a, b - a, body + off, body + off + L.plan.stream[lane]);
        }
        if (lane == 0) {
            const uint32_t sz = seq_section(L.T, seq, nseq, body + lsize, body + bn);
            L.comp = sz ? lsize + sz : 0;
        }
    }
    __syncthreads();
    const uint32_t comp = L.comp;
    const uint32_t type = block_choice(bn, false, comp);
    __syncthreads();   // (L.comp is rewritten by the next block)
    if (type == kBlockCompressed) {
        if (lane == 0)
            block_header(dst, last, type, comp);
        return 3 + comp;
    }
    if (lane == 0)
        block_header(dst, last, kBlockRaw, bn);
    for (uint32_t i = lane; i < bn; i += 64)
        body[i] = s[b0 + i];
    return 3 + bn;
}

// seq_offsets by the whole wave: sequences are taken 64 at a time, a lane
// each; every lane then walks the same history through the batch in order
// (sequence j's ll and off read from lane j: wave-uniform values, so the walk
// is scalar work) and keeps the value of its own sequence.  The serial order
// without a memory round trip per step.  Returns the history after the block.
__device__ __forceinline__ Reps wave_offsets(Reps h, Seq *__restrict__ seq, uint32_t nseq)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t base = 0; base < nseq; base += 64) {
        const uint32_t i = base + lane, cnt = min(64u, nseq - base);
        uint32_t ll = 0, off = 0, mine = 0;
        if (i < nseq) {
            ll = seq[i].ll;
            off = seq[i].off;
        }
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t v = rep_code(h, (uint32_t)__builtin_amdgcn_readlane((int)ll, (int)j),
                                        (uint32_t)__builtin_amdgcn_readlane((int)off, (int)j));
            if (lane == j)
                mine = v;
        }
        if (i < nseq)
            seq[i].off = mine;
    }
    return h;
}

// ... in the full format (zstd_enc_full_dev.h).  L.rep is the frame's offset
// history before the block; a block written Compressed moves it on.  Kept out
// of line: inlined into the frame loop it takes more than 256 VGPRs (hundreds
// of SGPRs spilled into them); as a function it takes 84.  The wide kernel
// (zstd_enc_wide_dev.h) passes one argument more, the full kernel none: the
// frame's table (a gu32 *), or null for a frame the full search takes.  Only
// the search differs: with a table, block s[b0, b0 + bn) is searched over it
// as the earlier blocks left it -- an empty block or a one-byte run returns
// before that and inserts nothing -- and the LDS table is only PostF's room.
template <class... Tab>
__device__ __noinline__ uint32_t compress_block(LdsF &L, const uint8_t *__restrict__ s, uint32_t b0, uint32_t bn, bool last,
                                   uint8_t *__restrict__ dst, uint8_t *__restrict__ lit, Seq *__restrict__ seq,
                                   Tab... tab)
{
    constexpr bool kWide = sizeof...(Tab) != 0;
    const uint32_t lane = threadIdx.x;
    if (bn == 0) {
        if (lane == 0)
            block_header(dst, last, kBlockRaw, 0);
        return 3;
    }
    if (one_byte_run(s + b0, bn)) {
        if (lane == 0) {
            block_header(dst, last, block_choice(bn, true, 0), bn);
            dst[3] = s[b0];
        }
        return 4;
    }
    gu32 *wtab = nullptr;
    if constexpr (kWide)
        wtab = (tab, ...);
    const bool wide = wtab != nullptr;
    if (!wide)
        for (uint32_t i = lane; i < (1u << kHashLog); i += 64)
            L.tab[i] = 0;
    for (uint32_t i = lane; i < kHufSymsF; i += 64)
        L.count[i] = 0;
    if (lane < 4)
        L.bits[lane] = 0;
    __syncthreads();
    uint32_t nseq, nlit;   // ---- match
    if constexpr (kWide) {
        if (wide)
            find_matches<true, kWideHashLog>(wtab, L.count, s, b0, bn, lit, seq, nseq, nlit);
        else
            find_matches<true>(L.tab, L.count, s, b0, bn, lit, seq, nseq, nlit);
    } else {
        find_matches<true>(L.tab, L.count, s, b0, bn, lit, seq, nseq, nlit);
    }
    PostF &P = L.post;     // (the hash table is dead from here)

    // ---- offsets into offset values: serial in the history
    for (uint32_t i = lane; i < 3 * 64; i += 64)
        (&P.hist[0][0])[i] = 0;
    const Reps next = wave_offsets(L.rep, seq, nseq);
    if (lane == 0) {
        L.next = next;
        L.wants = lit_wants_huf_f(L.count, nlit, L.plan) ? 1u : 0u;
    }
    __syncthreads();
    const bool tries = L.wants != 0;
    // ---- the three code histograms
    for (uint32_t i = lane; i < nseq; i += 64) {
        const Seq q = seq[i];
        atomicAdd(&P.hist[0][ll_code(q.ll)], 1u);
        atomicAdd(&P.hist[1][highbit(q.off)], 1u);
        atomicAdd(&P.hist[2][ml_code(q.ml)], 1u);
    }
    // ---- literals: the sort by the wave, lengths and description by one lane
    if (tries) {
        uint8_t *const order = huf_order(P.ws);
        for (uint32_t c = lane; c < kHufSymsF; c += 64)
            if (L.count[c] != 0)
                order[huf_rank(L.count, c)] = (uint8_t)c;
    }
    __syncthreads();
    if (tries) {
        if (lane == 0) {
            huf_lengths_sorted(L.count, P.huf, P.ws);
            P.hdesc_len = P.huf.max_bits ? huf_desc_f(P.huf, P.wt, P.hdesc) : 0;
            L.wants = P.hdesc_len != 0 ? 1u : 0u;
        }
        __syncthreads();
    }
    const uint32_t ns = huf_streams(nlit), seg = huf_segment(nlit);
    if (tries && L.wants) {   // (0 now: no legal description)
        for (uint32_t k = 0; k < ns; k++) {
            const uint32_t a = ns == 4 ? k * seg : 0, b = ns == 4 && k < 3 ? a + seg : nlit;
            uint32_t sum = 0;
            for (uint32_t i = a + lane; i < b; i += 64)
                sum += P.huf.len[lit[i]];
            atomicAdd(&L.bits[k], sum);
        }
        __syncthreads();
        if (lane == 0) {
            const uint64_t bits[4] = {L.bits[0], L.bits[1], L.bits[2], L.bits[3]};
            lit_plan_huf_f(P.hdesc_len, bits, L.plan);
        }
        __syncthreads();
    }
    const uint32_t mode = L.plan.mode, lsize = L.plan.size;
    if (lane == 0)
        L.comp = 0;
    uint8_t *const body = dst + 3;
    if (lsize + 1 < bn) {
        // ---- literals and sequences, where they land
        if (lane == 0)
            lit_write_head_f(L.plan, P.hdesc, P.hdesc_len, body);
        if (mode == kLitRaw) {
            const uint32_t head = lsize - nlit;
            for (uint32_t i = lane; i < nlit; i += 64)
                body[head + i] = lit[i];
        } else if (mode == kLitRle) {
            if (lane == 0)
                body[lsize - 1] = lit[0];
        } else if (lane < ns) {
            uint32_t off = lsize;   // the streams end the section
            for (uint32_t k = lane; k < ns; k++)
                off -= L.plan.stream[k];
            const uint32_t a = ns == 4 ? lane * seg : 0, b = ns == 4 && lane < 3 ? a + seg : nlit;
            huf_encode_stream_f(P.huf, lit + a, b - a, body + off, body + off + L.plan.stream[lane]);
        }
        if (lane == 0) {
            seq_plan(P.hist, nseq, L.T, P.W, P.seq);   // (the Huffman work area is dead)
            const uint32_t sz = seq_section_f(P.seq, seq, nseq, body + lsize, body + bn);
            L.comp = sz ? lsize + sz : 0;
        }
    }
    __syncthreads();
    const uint32_t comp = L.comp;
    const uint32_t type = block_choice(bn, false, comp);
    __syncthreads();   // (L.comp is rewritten by the next block)
    if (type == kBlockCompressed) {
        if (lane == 0) {
            block_header(dst, last, type, comp);
            L.rep = L.next;
        }
        return 3 + comp;
    }
    if (lane == 0)
        block_header(dst, last, kBlockRaw, bn);
    for (uint32_t i = lane; i < bn; i += 64)
        body[i] = s[b0 + i];
    return 3 + bn;
}

// One instantiation per format: the subset's is the kernel it was before the
// full format existed, with its LDS, registers and seven workgroups per CU.
// The wide one is the full kernel with a table of kWideTableBytes per workgroup
// in the scratch, behind everything the others keep there (wide_tables_at).
// The wave clears it at the start of every frame above kWideMinFrame bytes, all
// of it, so a persistent workgroup's next frame finds nothing of the last one:
// an entry at or past the new frame's length would be a read outside the frame.
template <bool kFull, bool kWide = false>
__global__ __launch_bounds__(64) void zstd_compress_kernel(const zsk_compress_desc_t *__restrict__ desc,
                                                           uint32_t nframes, const uint8_t *__restrict__ src,
                                                           uint8_t *__restrict__ dst, uint32_t *__restrict__ csize,
                                                           const uint32_t *__restrict__ sums,
                                                           uint8_t *__restrict__ scratch)
{
    __shared__ typename std::conditional<kFull, LdsF, Lds>::type L;
    const uint32_t lane = threadIdx.x;
    if (lane == 0) {
        if constexpr (kFull)
            seq_tables_build_f(L.T);
        else
            seq_tables_build(L.T);
    }
    __syncthreads();
    uint8_t *const lit = scratch + (size_t)blockIdx.x * kWgScratch;
    Seq *const seq = reinterpret_cast<Seq *>(lit + kZBlock);
    for (uint32_t f = blockIdx.x; f < nframes; f += gridDim.x) {
        const zsk_compress_desc_t d = desc[f];
        if (d.src_size > kMaxFrame || (d.dst_off & 15)) {
            if (lane == 0)
                csize[f] = 0;
            continue;
        }
        const uint8_t *const s = src + d.src_off;
        uint8_t *const out = dst + d.dst_off;
        const uint32_t n = d.src_size;
        const bool ck = (d.flags & ZSK_COMPRESS_CONTENT_CHECKSUM) != 0;
        if (lane == 0)
            frame_header(out, n, ck);
        if constexpr (kFull) {
            if (lane == 0)
                reps_init(L.rep);
        }
        uint32_t at = frame_header_size(n);
        const uint32_t nb = frame_blocks(n);
        gu32 *wtab = nullptr;
        if constexpr (kWide) {
            if (wide_frame(n)) {
                wtab = (gu32 *)(scratch + wide_tables_at(gridDim.x, nframes) + (size_t)blockIdx.x * kWideTableBytes);
                auto *const t = (__attribute__((address_space(1))) u32x4 *)wtab;
                for (uint32_t i = lane; i < kWideTableBytes / sizeof(u32x4); i += 64)
                    t[i] = u32x4{0, 0, 0, 0};
            }
        }
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t b0 = b * kZBlock;
            if constexpr (kWide)
                at += compress_block(L, s, b0, min(n - b0, kZBlock), b + 1 == nb, out + at, lit, seq, wtab);
            else
                at += compress_block(L, s, b0, min(n - b0, kZBlock), b + 1 == nb, out + at, lit, seq);
        }
        if (ck) {
            if (lane < 4)
                out[at + lane] = (uint8_t)(sums[f] >> (8 * lane));
            at += 4;
        }
        if (lane == 0)
            csize[f] = at;
    }
}

}   // namespace

// The wide instantiation lives in an object of its own: zstd_compress_wide.hip
// is this file with ZSK_ZSTD_COMPRESS_WIDE_OBJECT defined, which leaves the
// kernel's launch below and nothing else.  In one module the full and the wide
// block encoders would share the format layer's functions, which are inlined
// into a single caller but not into two, and the full kernel would no longer
// be the code it was (130 VGPRs and 464 bytes of scratch for 84 and 352).
void launch_zstd_compress_wide_kernel(uint32_t grid, hipStream_t stream, const zsk_compress_desc_t *d_desc,
                                      uint32_t nframes, const uint8_t *d_src, uint8_t *d_dst, uint32_t *d_csize,
                                      const uint32_t *d_sums, uint8_t *d_scratch);

#ifdef ZSK_ZSTD_COMPRESS_WIDE_OBJECT

void launch_zstd_compress_wide_kernel(uint32_t grid, hipStream_t stream, const zsk_compress_desc_t *d_desc,
                                      uint32_t nframes, const uint8_t *d_src, uint8_t *d_dst, uint32_t *d_csize,
                                      const uint32_t *d_sums, uint8_t *d_scratch)
{
    hipLaunchKernelGGL((zstd_compress_kernel<true, true>), dim3(grid), dim3(64), 0, stream, d_desc, nframes, d_src,
                       d_dst, d_csize, d_sums, d_scratch);
}

}   // namespace zsk

#else

namespace {

// The descriptors the checksum kernel sees: the frames that ask for a content
// checksum, the others (and refused ones) as empty frames.
__global__ __launch_bounds__(256) void zstd_ckdesc_kernel(const zsk_compress_desc_t *__restrict__ desc, uint32_t n,
                                                          zsk_compress_desc_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    zsk_compress_desc_t d = desc[i];
    if (!(d.flags & ZSK_COMPRESS_CONTENT_CHECKSUM) || d.src_size > kMaxFrame)
        d.src_size = 0;
    out[i] = d;
}

uint32_t grid_of(uint32_t nframes)
{
    return std::min(nframes, kGridMax);
}

}   // namespace

bool zstd_format_known(int format)
{
    return format == ZSK_ZSTD_FORMAT_SUBSET || format == ZSK_ZSTD_FORMAT_FULL || format == ZSK_ZSTD_FORMAT_FULL_WIDE;
}

// (the same for the subset and the full format: what the full one adds lives
// in LDS; the wide format adds a table per resident workgroup)
size_t zstd_compress_scratch_size(uint32_t nframes, int format)
{
    if (nframes == 0)
        return 0;
    const size_t base = wide_tables_at(grid_of(nframes), nframes);
    return format == ZSK_ZSTD_FORMAT_FULL_WIDE ? base + (size_t)grid_of(nframes) * kWideTableBytes : base;
}

int launch_zstd_compress(const zsk_compress_desc_t *d_desc, uint32_t nframes, const uint8_t *d_src, uint8_t *d_dst,
                         uint32_t *d_csize, void *d_scratch, size_t scratch_size, const uint32_t *d_sums,
                         hipStream_t stream, int format)
{
    if (!zstd_format_known(format))
        return -1;
    if (nframes == 0)
        return 0;
    if (!d_desc || !d_src || !d_dst || !d_csize || !d_scratch ||
        scratch_size < zstd_compress_scratch_size(nframes, format))
        return -1;
    if (format == ZSK_ZSTD_FORMAT_FULL_WIDE && ((uintptr_t)d_scratch & 15))   // (the tables: 16-byte stores)
        return -1;
    const uint32_t grid = grid_of(nframes);
    uint8_t *const wg = static_cast<uint8_t *>(d_scratch);
    if (!d_sums) {
        zsk_compress_desc_t *const ckdesc = reinterpret_cast<zsk_compress_desc_t *>(wg + align256((size_t)grid * kWgScratch));
        uint32_t *const sums = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ckdesc) +
                                                            align256((size_t)nframes * sizeof(zsk_compress_desc_t)));
        hipLaunchKernelGGL(zstd_ckdesc_kernel, dim3((nframes + 255) / 256), dim3(256), 0, stream, d_desc, nframes,
                           ckdesc);
        if (hipGetLastError() != hipSuccess || launch_src_checksums(ckdesc, nframes, d_src, sums, stream) != 0)
            return -1;
        d_sums = sums;
    }
    if (format == ZSK_ZSTD_FORMAT_FULL_WIDE)
        launch_zstd_compress_wide_kernel(grid, stream, d_desc, nframes, d_src, d_dst, d_csize, d_sums, wg);
    else if (format == ZSK_ZSTD_FORMAT_FULL)
        hipLaunchKernelGGL(zstd_compress_kernel<true>, dim3(grid), dim3(64), 0, stream, d_desc, nframes, d_src, d_dst,
                           d_csize, d_sums, wg);
    else
        hipLaunchKernelGGL(zstd_compress_kernel<false>, dim3(grid), dim3(64), 0, stream, d_desc, nframes, d_src, d_dst,
                           d_csize, d_sums, wg);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}   // namespace zsk

extern "C" ZSEEK_EXPORT size_t zsk_zstd_compress_scratch_size(uint32_t nframes, uint64_t src_bytes)
{
    (void)src_bytes;   // the scratch is per resident workgroup and per frame, not per input byte
    return zsk::zstd_compress_scratch_size(nframes, ZSK_ZSTD_FORMAT_SUBSET);
}

extern "C" ZSEEK_EXPORT int zsk_zstd_compress_frames(const zsk_compress_desc_t *d_desc, uint32_t nframes,
                                                     const void *d_src, void *d_dst, uint32_t *d_csize,
                                                     void *d_scratch, size_t scratch_size, void *stream)
{
    return zsk::launch_zstd_compress(d_desc, nframes, static_cast<const uint8_t *>(d_src),
                                     static_cast<uint8_t *>(d_dst), d_csize, d_scratch, scratch_size, nullptr,
                                     static_cast<hipStream_t>(stream), ZSK_ZSTD_FORMAT_SUBSET);
}

extern "C" ZSEEK_EXPORT size_t zsk_zstd_compress_scratch_size_ex(uint32_t nframes, uint64_t src_bytes, int format)
{
    (void)src_bytes;
    return zsk::zstd_format_known(format) ? zsk::zstd_compress_scratch_size(nframes, format) : 0;
}

extern "C" ZSEEK_EXPORT int zsk_zstd_compress_frames_ex(const zsk_compress_desc_t *d_desc, uint32_t nframes,
                                                        const void *d_src, void *d_dst, uint32_t *d_csize,
                                                        void *d_scratch, size_t scratch_size, void *stream,
                                                        int format)
{
    return zsk::launch_zstd_compress(d_desc, nframes, static_cast<const uint8_t *>(d_src),
                                     static_cast<uint8_t *>(d_dst), d_csize, d_scratch, scratch_size, nullptr,
                                     static_cast<hipStream_t>(stream), format);
}

#endif   // ZSK_ZSTD_COMPRESS_WIDE_OBJECT
