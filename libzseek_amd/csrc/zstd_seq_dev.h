// zstd_seq_dev.h -- the sequence replay on the device: item emission, the
// bitstream reader, seq_body, the literal fix-up.  Included by zstd_huf_seq.hip
// alone, after its g_sdiag (tuning builds: seq_body adds to it).
#pragma once

#include "zstd_dev.h"

namespace zsk {
namespace {

using namespace lz4d;

// literal / match length codes: base | extra bits << 24 (RFC 8878 §3.1.1.3.2.1)
__constant__ uint32_t c_ll[36] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,
    16 | 1u << 24, 18 | 1u << 24, 20 | 1u << 24, 22 | 1u << 24, 24 | 2u << 24, 28 | 2u << 24,
    32 | 3u << 24, 40 | 3u << 24, 48 | 4u << 24, 64 | 6u << 24, 128 | 7u << 24, 256 | 8u << 24,
    512 | 9u << 24, 1024 | 10u << 24, 2048 | 11u << 24, 4096 | 12u << 24, 8192 | 13u << 24,
    16384 | 14u << 24, 32768 | 15u << 24, 65536 | 16u << 24};
__constant__ uint32_t c_ml[53] = {
    3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27,
    28, 29, 30, 31, 32, 33, 34, 35 | 1u << 24, 37 | 1u << 24, 39 | 1u << 24, 41 | 1u << 24,
    43 | 2u << 24, 47 | 2u << 24, 51 | 3u << 24, 59 | 3u << 24, 67 | 4u << 24, 83 | 4u << 24,
    99 | 5u << 24, 131 | 7u << 24, 259 | 8u << 24, 515 | 9u << 24, 1027 | 10u << 24,
    2051 | 11u << 24, 4099 | 12u << 24, 8195 | 13u << 24, 16387 | 14u << 24, 32771 | 15u << 24,
    65539 | 16u << 24};

// ---- sequences: one lane per seek-table entry ------------------------------------------
// Replays the frame's op list: FSE states (tables from the block slots),
// repeat offsets, every libzstd check, items in the LZ4 item format with the
// full offset; then the final status, item count and checksum request.
// Items go straight from registers to the frame's slots: every emit issues
// exactly three 8-byte buffer stores (the ones it does not need are disabled
// by an out-of-range offset), so the compiler's vmcnt waits for the next
// sequence's bitstream window -- loaded before the stores -- never wait on
// them.  Consecutive 8-byte stores of a lane fill its lines in L2.
struct LSink {
    __amdgpu_buffer_rsrc_t r;   // the wave's item slots (one resource per replay)
    uint32_t ib;                // this frame's slot 0 in r (items)
    uint32_t k, cap;
};

typedef uint32_t u32x2s __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void lput3(const LSink &S, uint32_t n, uint64_t v0, uint64_t v1, uint64_t v2)
{
    const uint32_t a = 8u * (S.ib + S.k);
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2s, v0), S.r, n >= 1 ? a : kOOR, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2s, v1), S.r, n >= 2 ? a + 8 : kOOR + 8, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2s, v2), S.r, n >= 3 ? a + 16 : kOOR + 16, 0, 0);
}

// the 8-byte item format of lz4_split.hip (Sink), with the full offset in
// extended items (an extended pair never starts in slot 63 of a 64-slot
// group: a zero item pads it)
// (ONE: every lane runs the emit in step; lane 0's stores land)
template <bool ONE = false>
__device__ __forceinline__ bool lemit(LSink &S, uint32_t src, uint32_t lit, uint32_t off, uint32_t ml)
{
    const bool ext = lit > 255 || ml > 258 || (ml != 0 && ml < 4) || off > 0xFFFF;
    const uint32_t pad = ext && (S.k & 63) == 63 ? 1u : 0u;
    const uint32_t n = ext ? 2 + pad : 1;
    const bool ok = S.k + n <= S.cap;
    const uint64_t e0 = ((uint64_t)off << 32) | src | kItemExt, e1 = ((uint64_t)ml << 32) | lit;
    const uint64_t sh = ((uint64_t)(off | lit << 16 | (ml ? ml - 3 : 0) << 24) << 32) | src;
    // (ONE: thread 0's -- lane 0 of the first wave -- land)
    lput3(S, ok && (!ONE || threadIdx.x == 0) ? n : 0, ext ? (pad ? 0 : e0) : sh, pad ? e0 : e1, e1);
    S.k += ok ? n : 0;
    return ok;
}

// Sequence bitstream reader, no ring: at each sequence the lane loads the 16
// bytes (4 dwords) just below its cursor together with the sequence's table
// cells — one wait covers both — and consumes from registers: C = the top
// two dwords, two reserve dwords shifted in by fills.  A sequence reads at
// most 89 bits; the window holds at least 97 below the cursor.  Coordinates
// are bits from the stream's dword-aligned base x0; bits below the stream's
// first byte (xs) read as 0.
struct SRd {
    __amdgpu_buffer_rsrc_t r;
    uint32_t x0;
    int32_t xs;
    int32_t cur;        // stream bits below cur are unread
    uint64_t C;         // bits [base, base + 64)
    int32_t base, nb;   // nb = cur - base valid bits at the bottom of C
    uint32_t r1, r0;    // the two dwords below C
    u32x4 L;            // the window in flight (sr_issue -> sr_use)
    int32_t D;
    uint32_t sl;        // the one-frame route: the stream's dwords staged at this LDS address (0: not)
    uint32_t zv;        // (ONE) an opaque per-lane zero added to LDS addresses (below)
};

// len >= 1.  False when the stream's last byte (its end mark) is 0.
__device__ __forceinline__ bool sr_init(SRd &b, __amdgpu_buffer_rsrc_t r, uint32_t x, uint32_t len)
{
    b.r = r;
    b.x0 = x & ~3u;
    b.xs = 8 * (int32_t)(x & 3u);
    const uint32_t rel = (x & 3u) + len;
    const uint32_t last = b.sl ? (uint32_t)*la<uint8_t>(b.sl + rel - 1)
                               : (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, b.x0 + rel - 1, 0, 0);
    b.cur = 8 * (int32_t)(rel - 1) + (last ? 31 - __builtin_clz(last) : 0);
    return last != 0;
}

// the window below the cursor in two halves: sr_issue loads it (one 16-byte
// load on every path, so the compiler's vmcnt counts stay exact; near the
// stream's base it loads dwords [0, 4) and sr_use shifts them up by -k0,
// dwords below the base reading as 0), sr_use unpacks it where it is first
// needed -- a sequence's window is issued at the end of the one before,
// ahead of that one's item stores
template <bool ONE>
__device__ __forceinline__ void sr_issue(SRd &b)
{
    const int32_t D = (b.cur + 31) >> 5, k0 = D - 4;   // dwords [k0, D) hold bits [32 k0, 32 D)
    // (ONE: the staged stream has 16 zero bytes below it, bits [-128, 0): a
    // window wholly below the stream -- a corrupt stream read past its start,
    // which libzstd 1.4.9 reads as zeros -- is those bytes too)
    if (ONE)
        b.L = *la<u32x4_a4>(b.sl + 4u * (uint32_t)(k0 > -4 ? k0 : -4) + b.zv);
    else
        b.L = __builtin_bit_cast(
            u32x4, __builtin_amdgcn_raw_buffer_load_b128(b.r, b.x0 + 4u * (uint32_t)(k0 > 0 ? k0 : 0), 0, 0));
    b.D = D;
}

template <bool ONE = false>
__device__ __forceinline__ void sr_use(SRd &b)
{
    const int32_t D = b.D, k0 = D - 4;
    u32x4 w = b.L;
    // the window reaches the stream's first dword only at a block's last few
    // sequences: a branch the wave skips, not selects on every sequence (ONE:
    // the staged copy reads zeros there itself)
    if (!ONE && k0 <= 0) {
        const u32x4 L = b.L;
        const int32_t sft = -k0;
        w.x = sft == 0 ? L.x : 0u;
        w.y = sft == 0 ? L.y : sft == 1 ? L.x : 0u;
        w.z = sft == 0 ? L.z : sft == 1 ? L.y : sft == 2 ? L.x : 0u;
        w.w = sft == 0 ? L.w : sft == 1 ? L.z : sft == 2 ? L.y : sft == 3 ? L.x : 0u;
        // dword 0 holds the stream's first byte: clear the bits below it
        w.x &= above(b.xs, 32 * k0);
        w.y &= above(b.xs, 32 * k0 + 32);
        w.z &= above(b.xs, 32 * k0 + 64);
        w.w &= above(b.xs, 32 * k0 + 96);
    }
    b.C = (uint64_t)w.w << 32 | w.z;
    b.base = 32 * (D - 2);
    b.nb = b.cur - b.base;   // 33..64
    b.r1 = w.y;
    b.r0 = w.x;
}

template <bool ONE>
__device__ __forceinline__ void sr_load(SRd &b)
{
    sr_issue<ONE>(b);
    sr_use<ONE>(b);
}

__device__ __forceinline__ void sr_fill(SRd &b)
{
    const bool need = b.nb < 32;
    b.C = need ? (b.C << 32) | b.r1 : b.C;
    b.r1 = need ? b.r0 : b.r1;
    b.nb = need ? b.nb + 32 : b.nb;
    b.base = need ? b.base - 32 : b.base;
}

// n (<= 31) bits; nb >= n (a bitfield extract: width 0 reads 0)
__device__ __forceinline__ uint32_t sr_take(SRd &b, uint32_t n)
{
    const uint32_t v =
        __builtin_amdgcn_ubfe((uint32_t)(b.C >> ((uint32_t)(b.nb - (int32_t)n) & 63)), 0u, n);
    b.nb -= (int32_t)n;
    return v;
}

// close the sequence: the cursor moves past what was consumed
__device__ __forceinline__ void sr_done(SRd &b)
{
    b.cur = b.base + b.nb;
}


// 32 frames per wave (lanes 32..63 idle), one wave per workgroup: each
// frame's three FSE tables are copied into 1600 bytes of LDS when they fit
// (else read from the slot), so the per-sequence lookups stay on chip; with
// three such workgroups per CU the LDS, not the lanes, sets how many frames
// are in flight.  Same-box A/B at config 5 (sequence kernel alone in the
// profile, beside the Huffman kernel): 5.6 ms as here; tables read from the
// slot only, 64 or 32 frames per wave, 9.3 ms; 408 or 544 cells per frame
// (more workgroups per CU, more blocks' tables read from the slot) 8.2 and
// 6.6 ms; 1,056 or 1,312 cells (more blocks' tables in LDS, fewer frames per
// CU) 11.4 and 12.8 ms per launch against 10.6; the LL / ML code tables
// computed (packed constants and selects) instead of read from LDS, 11.05;
// 24 or 20 frames per wave (four or five single-wave workgroups per CU, one
// per SIMD) the same as 32.  Round 3, under the 4-chunk pipeline (other
// chunks' kernels beside it): tables from the slot (no LDS) 10.96 ms per
// launch at 32 frames per wave, 11.42 at 64, against 10.34 as here; the
// sequence loop made branch-free (repeat offsets, checks, window unpack)
// 11 % more wave cycles (its window wait no longer clear of the stores).
// OFG: only the LL and ML tables in LDS (544 cells: four workgroups per CU,
// 128 frames in flight instead of 96); the OF cell of the next sequence is
// loaded from the slot right after its state is known, just ahead of the
// next window load, so the one wait for the window covers it.  Same-box A/B
// at config 5: kernel alone 2.42 ms against 2.79 with all three tables in
// LDS (800 cells); the 4-chunk pipeline 9.25 / 9.27 against 9.43 / 9.40 ms
// per launch.
// GM generalizes it: bit t set = table t (LL, OF, ML) read from the slot, its
// cell loaded one sequence ahead; the others are staged in LDS.  More tables
// from the slot lose: OF + ML (288 cells, eight workgroups per CU) 4.71 ms
// alone, all three 6.45 ms, against 2.43 (pipeline 9.70 / 10.15 vs 9.26).
// Round 4: the bitstream through a per-lane LDS ring (64 dwords, refilled 4
// per sequence two sequences ahead, so the window is an LDS read and no load
// is waited on per sequence) loses -- the loop is issue-bound, not waiting on
// the window: same-box config 5, 3 chunks, 8.52 ms as here against 9.18 / 9.45
// with the ring beside these tables, 10.9 with the ring and all three tables in
// LDS (11.2 at 64 frames per wave); 4 chunks 8.85 against 9.05 / 10.6
// (profiles/r04_zstd_ring_ab.txt; the variant since removed).  The losing
// layouts above -- tables from the slot at 64 or 32 frames per wave, all three
// tables in LDS -- are no longer built either (tuning builds selected them
// with ZSEEK_ZSTD_SEQ=1 / 2 / 3).
constexpr uint32_t kSeqLanes = 32;
constexpr uint32_t kSeqCells = 544;   // u16 cells per frame (LL + ML 512 + copy slack)
constexpr uint32_t kSeqGm = 2;        // OF from the slot
// ONE (the one-frame route, a request's few frames): a wave per frame, every
// lane replaying the same frame in step (one lane's item stores land), with
// all three tables (up to 512 + 256 + 512 cells) and each block's sequence
// bitstream (up to kSeqStage bytes) staged in LDS by the whole wave.  A lone
// frame's replay is one dependent chain: with the window and the OF cell read
// from L2 / HBM per sequence it ran at ~0.8 us per sequence (853 us for a
// 64 KiB frame); from LDS the chain waits on LDS latency only.
constexpr uint32_t kSeqOneCells = 1312;
constexpr uint32_t kSeqStage = 131072 + 64;   // > a block's largest sequences section

// its LDS (a struct: the one-frame decode kernel below shares it with the
// Huffman job's, as a union)
template <uint32_t LANES, uint32_t CELLS, bool ONE>
struct SeqLds {
    uint32_t codes[89];
    __attribute__((aligned(16))) uint16_t ftab[CELLS && !ONE ? LANES * CELLS : 8];
    __attribute__((aligned(16))) uint8_t sstage[ONE ? kSeqStage + 32 : 16];
    uint64_t xtab[ONE ? kSeqOneCells : 1];                 // ONE: the expanded cells (below)
    __attribute__((aligned(16))) uint32_t srec[ONE ? 2 * 64 * 8 : 4];   // ONE: a batch's records (two buffers)
    uint32_t xflag;     // (two waves) a failure: stop
    uint32_t xst[8];    // (two waves) the replay state handed over
};

// the replay of workgroup bid (one wave: threads 0-63; TWO: two, the
// one-frame replay's chain on wave 0 and its vector phase on wave 1)
template <uint32_t LANES, uint32_t CELLS, uint32_t GM = 0, bool ONE = false, bool TWO = false>
__device__ __forceinline__ void seq_body(
    SeqLds<LANES, CELLS, ONE> &SH, uint32_t bid, const FrameDesc *__restrict__ desc, uint32_t n,
    const uint8_t *__restrict__ comp, uint8_t *__restrict__ ops, const uint64_t *__restrict__ blk_base,
    const uint8_t *__restrict__ slots, uint32_t *__restrict__ stop,
    const uint64_t *__restrict__ rec_base, uint64_t *__restrict__ items, uint32_t *__restrict__ nitems,
    int32_t *__restrict__ status, uint64_t *__restrict__ ck, uint32_t *__restrict__ fail_at, uint32_t f0)
{
    auto &codes = SH.codes;
    auto &ftab = SH.ftab;
    auto &sstage = SH.sstage;
    auto &xtab = SH.xtab;
    auto &srec = SH.srec;
#ifdef ZSK_TUNING
    const uint64_t tk0 = __builtin_readcyclecounter(), rt0 = __builtin_amdgcn_s_memrealtime();
    uint64_t tloop = 0, nseqs = 0, tchain = 0;
#endif
    for (uint32_t i = threadIdx.x; i < 89; i += 64)
        codes[i] = i < 36 ? c_ll[i] : c_ml[i - 36];
    if (threadIdx.x == 0)
        SH.xflag = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t f = ONE ? f0 + bid : f0 + bid * LANES + lane;   // frames [f0, n)
    const bool act = (ONE || lane < LANES) && f < n;
    FrameDesc d = {0, 0, 0, 0};
    if (act)
        d = desc[f];
    // one resource over the wave's frames (else lane by lane, each its own)
    const uint64_t lo = uni64(wave_min64(act ? d.c_off : ~0ull)) & ~15ull;
    const uint64_t hi = uni64(wave_max64(act ? d.c_off + d.c_size : 0ull));
    // the wave's item slots as one resource (else lane by lane, as comp);
    // reduced over the active lanes with every lane still present (an idle
    // lane's registers are not a value)
    uint64_t rb = 0;
    uint32_t icap = 0;
    if (act) {
        rb = rec_base[f];
        icap = (uint32_t)(rec_base[f + 1] - rb);
    }
    const uint64_t ilo = uni64(wave_min64(act ? rb : ~0ull)), ihi = uni64(wave_max64(act ? rb + icap : 0ull));
    if (!act)
        return;
    const uint64_t ob = op_base(blk_base, f);
    const uint32_t opn = (uint32_t)(op_base(blk_base, f + 1) - ob);
    ZOp *op = reinterpret_cast<ZOp *>(ops) + ob;
    LSink S;
    S.k = 0;
    S.cap = icap;
    uint16_t *const mytab = &ftab[CELLS && !ONE ? lane * CELLS : 0];
    // o and cap count from the start of the entry's current frame, at o0 in the
    // entry's output (OP_FBEGIN rebases them): libzstd's prefix starts at the
    // frame, so a match may reach back o + ll bytes and no further
    uint32_t cap = d.d_size;
    uint32_t o = 0, o0 = 0, rep0 = 1, rep1 = 4, rep2 = 8;
    uint64_t c = 0;
    int32_t st = zerr(ZE_GENERIC);
    // output offset where a failure is met: the start of the failing block
    // (every op of a block starts at its output start: literals advance
    // nothing, sequences and runs advance o), the frame's end for its
    // end-of-frame checks -- what libzstd's streaming decoder has produced
    // when it meets the failure (decompress.c:414-454)
    uint32_t fa = 0;
    uint32_t kstop = opn;   // the op the replay stopped at
    auto replay = [&](__amdgpu_buffer_rsrc_t r, uint64_t base, __amdgpu_buffer_rsrc_t ir, uint64_t i0) {
        S.r = ir;
        S.ib = (uint32_t)(rb - i0);
        for (uint32_t k = 0; k < opn; k++) {
            const ZOp P = op[k];
            uint32_t err = 0;
            fa = o0 + o;
            kstop = k;
            if (P.k == OP_LIT) {
                // the Huffman kernel runs beside this one: whether this
                // block's literals decoded is settled by zstd_lit_fix_kernel,
                // from the item count and output offset kept here
                op[k].b = S.k;
                op[k].c = o0 + o;
            } else if (P.k == OP_SEQ) {
                const uint32_t nseq = P.a;
                uint32_t lp_ = P.d;
                const uint32_t le = P.d + P.e;
                if (nseq) {
                    SRd b;
                    b.sl = 0;
                    b.zv = 0;
                    const uint32_t sx = (uint32_t)(d.c_off - base) + P.b;
                    bool staged = !ONE;
                    if (ONE && P.c != 0 && (sx & 3u) + P.c + 16 <= kSeqStage) {
                        // the stream's dwords into LDS, 16 bytes per lane per
                        // step, after 16 zero bytes; the bytes of its first dword
                        // below the stream zeroed too (the window's "bits below
                        // the stream read as 0" without a branch per sequence)
                        const uint32_t x0 = sx & ~3u, nb = (sx & 3u) + P.c, sl = ldsaddr(sstage) + 16;
                        // (TWO: wave 0 stages, then a barrier -- wave 1 reads
                        // the same bytes, so both waves take the same branches)
                        const bool stager = !TWO || threadIdx.x < 64;
                        if constexpr (TWO)
                            __syncthreads();   // (the last block's stage read by both)
                        wave_lds_sync();
                        if (stager)
                            for (uint32_t q = 16 * lane; q < nb; q += 1024)
                                *la<u32x4_a4>(sl + q) =
                                    __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, x0 + q, 0, 0));
                        wave_lds_sync();
                        if (stager && lane == 0) {
                            *la<u32x4>(sl - 16) = (u32x4){0, 0, 0, 0};
                            *la<uint32_t>(sl) &= above(8 * (int32_t)(sx & 3u), 0);
                        }
                        wave_lds_sync();
                        if constexpr (TWO)
                            __syncthreads();
                        b.sl = sl;
                        staged = true;
                    }
                    if (P.c == 0) {   // sequences counted and no stream: BIT_initDStream's error
                        err = ZE_CORRUPT;
                    } else if (!staged) {   // (ONE: a block's sequences always fit the stage)
                        err = ZE_GENERIC;
                    } else if (!sr_init(b, r, sx, P.c)) {
                        err = ZE_CORRUPT;
                    } else {
                        const uint32_t tll = P.g & 15, tof = (P.g >> 4) & 15, tml = (P.g >> 8) & 15;
                        // the block's tables into this lane's LDS cells when they
                        // fit: LL, OF, ML back to back (16-byte copies)
                        const uint16_t *gt = reinterpret_cast<const uint16_t *>(slots + (uint64_t)P.f * kZSlot + kSlotFse);
                        const uint32_t nll = 1u << tll, nof = 1u << tof, nml = 1u << tml;
                        const uint16_t *TL = gt + kFseOff[0], *TO = gt + kFseOff[1], *TM = gt + kFseOff[2];
                      if constexpr (ONE) {
                        // the one-frame replay: every cell expanded once by the
                        // wave into 8 bytes -- lo: the LDS address of its next
                        // state's base cell; hi: the state's bit count (bits
                        // 0-3, bit 4 clear: a bitfield extract's width or offset
                        // operand as it is), the value's extra bits (8-12), a
                        // bad-symbol flag (13), the symbol (16-21), the cell's
                        // whole bit count (value + state, 24-29) -- so a
                        // sequence's chain is one LDS read per table and its next
                        // cells' addresses two ops away from the bits (no
                        // code-table read, no next-state arithmetic).  Same bit
                        // order, values and checks as the loop below.
                        const uint32_t xb = ldsaddr(xtab), ncell = nll + nof + nml;
                        wave_lds_sync();
                        for (uint32_t cix = lane; cix < ((!TWO || threadIdx.x < 64) ? ncell : 0u); cix += 64) {
                            const uint32_t t = cix < nll ? 0u : cix < nll + nof ? 1u : 2u;
                            const uint32_t toff = t == 0 ? 0u : t == 1 ? nll : nll + nof;
                            const uint32_t x = cix - toff;
                            const uint32_t e = t == 0 ? TL[x] : t == 1 ? TO[x] : TM[x];
                            const uint32_t tl = t == 0 ? tll : t == 1 ? tof : tml;
                            const uint32_t sym = e & 63, ns = e >> 6;
                            const uint32_t nbits = tl + (uint32_t)__builtin_clz(ns) - 31;
                            const uint32_t nbase = (ns << nbits) - (1u << tl);
                            const bool bad = sym > (t == 0 ? 35u : t == 1 ? 31u : 52u);
                            // OF: value 2^code + code extra bits; LL / ML: the code table
                            const uint32_t code = bad || t == 1 ? 0u : codes[t == 0 ? sym : 36 + sym];
                            const uint32_t add = bad ? 0u : t == 1 ? sym : code >> 24;
                            const uint32_t hi32 = nbits | add << 8 | (bad ? 1u : 0u) << 13 | (bad ? 0u : sym) << 16 |
                                                  (add + nbits) << 24;
                            *la<uint64_t>(xb + 8 * cix) = (uint64_t)hi32 << 32 | (xb + 8 * (toff + nbase));
                        }
                        wave_lds_sync();
                        if constexpr (TWO)
                            __syncthreads();   // (wave 0's cells, seen by both)
                        // (an opaque per-lane zero in the addresses keeps the chain
                        // in VGPRs: scalarized, each LDS result waited for and
                        // copied to SGPRs at once -- the window's and the cells'
                        // reads no longer in flight together)
                        uint32_t zv;
                        asm volatile("v_mov_b32 %0, 0" : "=v"(zv));
                        b.zv = zv;
                        auto XL = [&](uint32_t x) { return *la<uint64_t>(xb + 8 * x + zv); };
                        auto XO = [&](uint32_t x) { return *la<uint64_t>(xb + 8 * (nll + x) + zv); };
                        auto XM = [&](uint32_t x) { return *la<uint64_t>(xb + 8 * (nll + nof + x) + zv); };
                        sr_load<ONE>(b);
                        uint64_t cl, co, cm;
                        {
                            const uint32_t sll = sr_take(b, tll), sof = sr_take(b, tof), sml = sr_take(b, tml);
                            sr_done(b);
                            cl = XL(sll);
                            co = XO(sof);
                            cm = XM(sml);
                        }
                        // the window: stream dwords [(cur >> 5) - 3, + 4), the
                        // staged zeros below the stream for a cursor past its start
                        const uint32_t sl = b.sl;
                        auto win = [&](int32_t cur) {
                            const int32_t k0 = (cur >> 5) - 3;
                            return *la<u32x4_a4>(sl + 4u * (uint32_t)(k0 > -4 ? k0 : -4) + zv);
                        };
                        int32_t cur = b.cur;
                        u32x4 W = win(cur);
#ifdef ZSK_TUNING
                        const uint64_t tl0 = __builtin_readcyclecounter();
                        nseqs += nseq;
#endif
                        // batches of up to 64 sequences: (1) the chain, wave-
                        // uniform -- cells, state bits, next states -> one 32-byte
                        // record per sequence in LDS: its 64 value bits and its
                        // three cells (a bad cell goes on: its state fields are
                        // valid); (2) lane q takes record q: the values,
                        // repeat offsets, item slots, the output / literal prefix
                        // sums, the replay's
                        // checks in its order (a bad cell first), the first
                        // failing sequence by ballot, and the items of the
                        // sequences before it (a lane's own stores).  Everything
                        // the serial loop below leaves -- items, o, lp_, S.k,
                        // err -- is the same.
                        const uint32_t rec = ldsaddr(srec);
                        // the chain of a batch of nb sequences: records at rb
                        auto chain = [&](uint32_t rb, uint32_t nb) {
                                if (lane == 0)
                                for (uint32_t q = 0; q < nb; q++) {
                                    // the 96 stream bits below cur, top-aligned: bit
                                    // 95 of N3:N2:N1 is stream bit cur - 1 (the
                                    // align takes the shift's low five bits)
                                    const uint32_t N3 = __builtin_amdgcn_alignbit(W.w, W.z, (uint32_t)cur),
                                                   N2 = __builtin_amdgcn_alignbit(W.z, W.y, (uint32_t)cur),
                                                   N1 = __builtin_amdgcn_alignbit(W.y, W.x, (uint32_t)cur);
                                    const uint64_t H = (uint64_t)N3 << 32 | N2;
                                    const uint32_t hl = (uint32_t)(cl >> 32), hm = (uint32_t)(cm >> 32), ho = (uint32_t)(co >> 32);
                                    // the sequence's bits: OF, ML, LL values, then the
                                    // LL, ML, OF states (T <= 31 + 16 + 16 + 26 = 89)
                                    // (byte-select adds: the three counts are the cells' top bytes)
                                    uint32_t T;
                                    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:BYTE_3\n\t"
                                        "v_add_u32_sdwa %0, %0, %3 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3"
                                        : "=&v"(T)
                                        : "v"(hl), "v"(hm), "v"(ho));
                                    // (T <= 64: from N3:N2; else at bit 96 - T < 32 of N2:N1)
                                    const uint32_t yH = (uint32_t)(H >> ((64 - T) & 63)),
                                                   yM = __builtin_amdgcn_alignbit(N2, N1, 0u - T);
                                    // (a select in asm: the compiler made the choice an
                                    // if / else over the exec mask, twice the ops)
                                    uint32_t Y;
                                    asm("v_cmp_ge_u32 vcc, 64, %1\n\tv_cndmask_b32 %0, %2, %3, vcc"
                                        : "=v"(Y)
                                        : "v"(T), "v"(yM), "v"(yH)
                                        : "vcc");
                                    // (the extract takes offset and width from the low
                                    // five bits: the state counts straight from hi)
                                    const uint32_t ao = (uint32_t)co + (__builtin_amdgcn_ubfe(Y, 0, ho) << 3),
                                                   am = (uint32_t)cm + (__builtin_amdgcn_ubfe(Y, ho, hm) << 3),
                                                   al = (uint32_t)cl + (__builtin_amdgcn_ubfe(Y, ho + hm, hl) << 3);
                                    const int32_t cur2 = cur - (int32_t)T;
                                    // the record (this sequence's values are the
                                    // vector phase's, from H and the cells), stored
                                    // ahead of the next sequence's reads: after them,
                                    // the wait for them would wait for it too
                                    // (two paired stores in asm: the compiler's own
                                    // choice varied with the kernel it sat in, up to
                                    // four stores and four address moves)
                                    asm volatile("ds_write2_b64 %0, %1, %2 offset1:1\n\t"
                                                 "ds_write2_b64 %0, %3, %4 offset0:2 offset1:3"
                                                 :
                                                 : "v"(rb + 32 * q), "v"(H), "v"(cl), "v"(cm), "v"(co)
                                                 : "memory");
                                    const u32x4 W2 = win(cur2);
                                    const uint64_t cl2 = *la<uint64_t>(al), cm2 = *la<uint64_t>(am), co2 = *la<uint64_t>(ao);
                                    cl = cl2;
                                    cm = cm2;
                                    co = co2;
                                    W = W2;
                                    cur = cur2;
                                }
                        };
                        // the vector phase of a batch of nd records at rb
                        auto vphase = [&](uint32_t rb, uint32_t nd) {
                                const bool on = lane < nd;
                                uint32_t ofv = 0, ml = 0, ll = 0, bad = 0;
                                if (on) {
                                    const u32x4 R = *la<u32x4>(rb + 32 * lane), R2 = *la<u32x4>(rb + 32 * lane + 16);
                                    const uint32_t hl = R.w, hm = R2.y, ho = R2.w;
                                    const uint32_t ob = __builtin_amdgcn_ubfe(ho, 8, 5), mb = __builtin_amdgcn_ubfe(hm, 8, 5),
                                                   lb = __builtin_amdgcn_ubfe(hl, 8, 5), vb = ob + mb + lb;
                                    const uint64_t H = (uint64_t)R.y << 32 | R.x;
                                    const uint32_t X = (uint32_t)(H >> ((64 - vb) & 63));
                                    ofv = (1u << ob) + __builtin_amdgcn_ubfe(R.y, 32 - ob, ob);
                                    ll = (codes[__builtin_amdgcn_ubfe(hl, 16, 6)] & 0xFFFFFF) + __builtin_amdgcn_ubfe(X, 0, lb);
                                    ml = (codes[36 + __builtin_amdgcn_ubfe(hm, 16, 6)] & 0xFFFFFF) + __builtin_amdgcn_ubfe(X, lb, mb);
                                    bad = ((ho | hm | hl) >> 13) & 1;
                                }
                                // repeat offsets (RFC 8878 §3.1.2.5) by a scan: each
                                // sequence maps the history (a, b, c) = (rep0, rep1,
                                // rep2) to a new one -- a new offset v: (v, a, b);
                                // index 0: (a, b, c); 1: (b, a, c); 2: (c, a, b); 3:
                                // (a - 1 but >= 1, a, b) -- and its offset is the new
                                // first entry.  A composed map keeps, per entry,
                                // either a value (tag 3) or "old entry t less d"
                                // (tag t, d decrements: max(x - d, 1), as repeated
                                // decrements of values >= 1 compose).  Six shuffle
                                // steps compose each lane's prefix; applied to the
                                // batch's starting history they give every offset.
                                uint32_t tg[3], vl[3];
                                {
                                    const bool fresh = ofv > 3;
                                    const uint32_t idx = fresh ? 0u : ofv - 1 + (ll == 0);
                                    tg[0] = fresh ? 3u : idx == 3 ? 0u : idx;
                                    vl[0] = fresh ? ofv - 3 : idx == 3 ? 1u : 0u;
                                    tg[1] = !fresh && idx == 0 ? 1u : 0u;
                                    tg[2] = !fresh && idx <= 1 ? 2u : 1u;
                                    vl[1] = vl[2] = 0;
                                    if (!on) {   // identity
                                        tg[0] = 0;
                                        tg[1] = 1;
                                        tg[2] = 2;
                                        vl[0] = 0;
                                    }
                                }
    #pragma unroll
                                for (uint32_t sft = 1; sft < 64; sft <<= 1) {
                                    uint32_t pt[3], pv[3];
    #pragma unroll
                                    for (int q = 0; q < 3; q++) {
                                        pt[q] = (uint32_t)__shfl_up((int)tg[q], sft, 64);
                                        pv[q] = (uint32_t)__shfl_up((int)vl[q], sft, 64);
                                    }
                                    if (lane >= sft) {
    #pragma unroll
                                        for (int q = 0; q < 3; q++) {   // mine after the earlier prefix
                                            const uint32_t t = tg[q], v = vl[q];
                                            const uint32_t et = t == 0 ? pt[0] : t == 1 ? pt[1] : pt[2];
                                            const uint32_t ev = t == 0 ? pv[0] : t == 1 ? pv[1] : pv[2];
                                            tg[q] = t == 3 ? 3u : et;
                                            vl[q] = t == 3 ? v : et == 3 ? (ev > v ? ev - v : 1u) : ev + v;
                                        }
                                    }
                                }
                                auto apply = [&](uint32_t t, uint32_t v) -> uint32_t {
                                    if (t == 3)
                                        return v;
                                    const uint32_t x = t == 0 ? rep0 : t == 1 ? rep1 : rep2;
                                    return x > v ? x - v : 1u;
                                };
                                const uint32_t off = apply(tg[0], vl[0]);
                                if (nd) {
                                    const uint32_t n0 = lane_val(off, (int)nd - 1),
                                                   n1v = lane_val(apply(tg[1], vl[1]), (int)nd - 1),
                                                   n2v = lane_val(apply(tg[2], vl[2]), (int)nd - 1);
                                    rep0 = n0;
                                    rep1 = n1v;
                                    rep2 = n2v;
                                }
                                // item slots (lemit's rule: an extended pair never
                                // starts in slot 63 of a 64-slot group, a zero item
                                // pads it): a scan without pads, then, only if some
                                // extended pair lands on slot 63, the slots again
                                // sequence by sequence
                                const bool ext = on && (ll > 255 || ml > 258 || (ml != 0 && ml < 4) || off > 0xFFFF);
                                const uint32_t n1 = on ? (ext ? 2u : 1u) : 0u;
                                uint32_t kq = S.k + wave_incl_add(n1) - n1, pad = 0;
                                if (__ballot(ext && (kq & 63) == 63)) {
                                    uint32_t k = S.k;
                                    for (uint32_t q = 0; q < nd; q++) {
                                        const bool eq = lane_val(ext ? 1u : 0u, (int)q) != 0;
                                        const uint32_t pq = eq && (k & 63) == 63 ? 1u : 0u;
                                        if (lane == q) {
                                            kq = k;
                                            pad = pq;
                                        }
                                        k += eq ? 2 + pq : 1;
                                    }
                                }
                                const uint32_t ni = ext ? 2 + pad : 1;
                                const uint32_t ill = wave_incl_add(ll), iol = wave_incl_add(ll + ml);
                                const uint32_t lpq = lp_ + ill - ll, oq = o + iol - (ll + ml);
                                const uint32_t kind = bad                ? (uint32_t)ZE_CORRUPT
                                                      : ll + ml > cap - oq ? (uint32_t)ZE_DST_SMALL
                                                      : le - lpq < ll    ? (uint32_t)ZE_CORRUPT
                                                      : off > oq + ll    ? (uint32_t)ZE_CORRUPT
                                                      : kq + ni > S.cap  ? (uint32_t)ZE_GENERIC
                                                                         : 0u;
                                const uint64_t em = __ballot(on && kind != 0);
                                const uint32_t e = em ? (uint32_t)__builtin_ctzll(em) : nd;
                                if (lane < e) {
                                    const uint64_t e0 = ((uint64_t)off << 32) | lpq | kItemExt, e1 = ((uint64_t)ml << 32) | ll;
                                    const uint64_t sh = ((uint64_t)(off | ll << 16 | (ml ? ml - 3 : 0) << 24) << 32) | lpq;
                                    LSink Q = S;
                                    Q.k = kq;
                                    lput3(Q, ni, ext ? (pad ? 0 : e0) : sh, pad ? e0 : e1, e1);
                                }
                                if (e > 0) {
                                    lp_ += lane_val(ill, (int)e - 1);
                                    o += lane_val(iol, (int)e - 1);
                                }
                                if (e < nd) {
                                    err = lane_val(kind, (int)e);
                                    S.k = lane_val(kq, (int)e);
                                } else {
                                    if (nd)
                                        S.k = lane_val(kq + ni, (int)nd - 1);
                                }
                        };
                        if constexpr (TWO) {
                            // two waves (the fused launch's first two): wave 0
                            // runs batch k's chain while wave 1 runs batch k - 1's
                            // vector phase -- records double-buffered, one
                            // barrier per step; a failure found by wave 1 stops
                            // both after the step; then wave 1's replay state and
                            // wave 0's cursor are exchanged, so both waves go on
                            // with the same values
                            const uint32_t wv = threadIdx.x >> 6, nbat = (nseq + 63) / 64;
                            for (uint32_t kb = 0; kb <= nbat; kb++) {
                                if (wv == 0 && kb < nbat) {
#ifdef ZSK_TUNING
                                    const uint64_t tc0 = __builtin_readcyclecounter();
#endif
                                    chain(rec + 2048 * (kb & 1), min(64u, nseq - 64 * kb));
#ifdef ZSK_TUNING
                                    tchain += __builtin_readcyclecounter() - tc0;
#endif
                                }
                                if (wv == 1 && kb >= 1) {
                                    vphase(rec + 2048 * ((kb - 1) & 1), min(64u, nseq - 64 * (kb - 1)));
                                    if (err && lane == 0)
                                        SH.xflag = 1;
                                }
                                __syncthreads();
                                if (uni(*lp<uint32_t>(&SH.xflag)))
                                    break;
                            }
                            if (wv == 1 && lane == 0) {
                                SH.xst[0] = o;
                                SH.xst[1] = lp_;
                                SH.xst[2] = S.k;
                                SH.xst[3] = err;
                                SH.xst[4] = rep0;
                                SH.xst[5] = rep1;
                                SH.xst[6] = rep2;
                            }
                            if (wv == 0 && lane == 0)
                                SH.xst[7] = (uint32_t)cur;
                            __syncthreads();
                            o = uni(*lp<uint32_t>(&SH.xst[0]));
                            lp_ = uni(*lp<uint32_t>(&SH.xst[1]));
                            S.k = uni(*lp<uint32_t>(&SH.xst[2]));
                            err = uni(*lp<uint32_t>(&SH.xst[3]));
                            rep0 = uni(*lp<uint32_t>(&SH.xst[4]));
                            rep1 = uni(*lp<uint32_t>(&SH.xst[5]));
                            rep2 = uni(*lp<uint32_t>(&SH.xst[6]));
                            cur = (int32_t)uni(*lp<uint32_t>(&SH.xst[7]));
                            __syncthreads();   // (everyone has read; the flag reset for the next block)
                            if (threadIdx.x == 0)
                                SH.xflag = 0;
                            __syncthreads();
                        } else {
                            for (uint32_t i = 0; i < nseq && !err;) {
                                const uint32_t nb = min(64u, nseq - i);
                                wave_lds_sync();   // the last batch's records read
#ifdef ZSK_TUNING
                                const uint64_t tc0 = __builtin_readcyclecounter();
#endif
                                chain(rec, nb);
                                wave_lds_sync();
#ifdef ZSK_TUNING
                                tchain += __builtin_readcyclecounter() - tc0;
#endif
                                vphase(rec, nb);
                                i += nb;
                            }
                        }
                        b.cur = __builtin_amdgcn_readlane(cur, 0);
#ifdef ZSK_TUNING
                        tloop += __builtin_readcyclecounter() - tl0;
#endif
                      } else {
                        // cells staged in LDS per table (0: read from the slot)
                        const uint32_t nlll = (GM & 1) ? 0u : nll, nofl = (GM & 2) ? 0u : nof,
                                       nmll = (GM & 4) ? 0u : nml;
                        const bool fit = nlll + nofl + nmll == 0 || (CELLS && nlll + nofl + nmll + 32 <= CELLS);
                        if (fit) {
                            // (ONE: the whole wave copies, 8 cells per lane per step)
                            auto cp = [&](const uint16_t *src, uint32_t at, uint32_t cells) {
                                for (uint32_t c = ONE ? 8 * lane : 0; c < cells; c += ONE ? 512 : 8)
                                    *reinterpret_cast<u32x4 *>(mytab + at + c) = *reinterpret_cast<const u32x4 *>(src + c);
                            };
                            if (ONE)
                                wave_lds_sync();
                            cp(TL, 0, nlll);
                            cp(TO, nlll, nofl);
                            cp(TM, nlll + nofl, nmll);
                            if (ONE)
                                wave_lds_sync();
                        }
                        // the sequence loop, over tables in LDS (ds_read: the
                        // lookups' waits stay off vmcnt) or in the slot
                        auto seqs = [&](auto TLf, auto TOf, auto TMf) {
                            sr_load<ONE>(b);

                            uint32_t sll = sr_take(b, tll), sof = sr_take(b, tof), sml = sr_take(b, tml);
                            sr_done(b);
                            sr_issue<ONE>(b);
                            // three disabled stores: the loop's entry then has the
                            // VMEM pattern of its back edge (window, then three
                            // stores), so the window's wait stays vmcnt(3)
                            lput3(S, 0, 0, 0, 0);
                            // the slot tables' cells, one sequence ahead
                            uint32_t ell_n = 0, eof_n = 0, eml_n = 0;
                            if (GM & 1)
                                ell_n = TLf(sll);
                            if (GM & 2)
                                eof_n = TOf(sof);
                            if (GM & 4)
                                eml_n = TMf(sml);
                            for (uint32_t i = 0; i < nseq; i++) {
                                const uint32_t ell = (GM & 1) ? ell_n : TLf(sll), eof = (GM & 2) ? eof_n : TOf(sof),
                                               eml = (GM & 4) ? eml_n : TMf(sml);
                                sr_use(b);
                                const uint32_t llc = ell & 63, ofc = eof & 63, mlc = eml & 63;
                                if (llc > 35 || ofc > 31 || mlc > 52) {
                                    err = ZE_CORRUPT;
                                    break;
                                }
                                // offset bits (<= 31; the window holds >= 33), a fill before
                                // the ML + LL extra bits (<= 32) and one before the three
                                // state updates (<= 26)
                                // offset value < 2^32 (ofc <= 31)
                                const uint32_t ofv = (1u << ofc) + sr_take(b, ofc);
                                const uint32_t mlcode = codes[36 + mlc], llcode = codes[llc];
                                sr_fill(b);
                                // the ML and LL extra bits (<= 32, ML above LL) in one extract
                                const uint32_t mlb = mlcode >> 24, llb = llcode >> 24;
                                const uint32_t X = (uint32_t)(b.C >> ((uint32_t)(b.nb - (int32_t)(mlb + llb)) & 63));
                                b.nb -= (int32_t)(mlb + llb);
                                const uint32_t ll = (llcode & 0xFFFFFF) + __builtin_amdgcn_ubfe(X, 0u, llb);
                                const uint32_t ml = (mlcode & 0xFFFFFF) + __builtin_amdgcn_ubfe(X, llb, mlb);
                                // repeat offsets as selects (RFC 8878 §3.1.2.5): a new
                                // offset (ofv > 3) or repeat idx 0..3; idx 0 keeps the
                                // history, idx 1 swaps the first two, 2 and 3 rotate
                                // (selects by the index bits: a nested ?: chain
                                // compiled to branches)
                                const bool fresh = ofv > 3;
                                const uint32_t idx = fresh ? 0u : ofv - 1 + (ll == 0);
                                const uint32_t r01 = (idx & 1) ? rep1 : rep0,
                                               r23 = (idx & 1) ? max(rep0 - 1, 1u) : rep2;   // rep0 - 1, 0 read as 1
                                const uint32_t off = fresh ? ofv - 3 : (idx & 2) ? r23 : r01;
                                const bool sh1 = fresh || idx != 0, sh2 = fresh || idx >= 2;
                                rep2 = sh2 ? rep1 : rep2;
                                rep1 = sh1 ? rep0 : rep1;
                                rep0 = sh1 ? off : rep0;
                                sr_fill(b);
                                // the three next states (fse_next's bits, <= 26: LL, ML,
                                // OF from the top) in one extract
                                const uint32_t nsl = ell >> 6, nsm = eml >> 6, nso = eof >> 6;
                                const uint32_t bl = tll + (uint32_t)__builtin_clz(nsl) - 31,
                                               bm = tml + (uint32_t)__builtin_clz(nsm) - 31,
                                               bo = tof + (uint32_t)__builtin_clz(nso) - 31;
                                const uint32_t Y = (uint32_t)(b.C >> ((uint32_t)(b.nb - (int32_t)(bl + bm + bo)) & 63));
                                b.nb -= (int32_t)(bl + bm + bo);
                                sll = ((nsl << bl) - (1u << tll)) + __builtin_amdgcn_ubfe(Y, bm + bo, bl);
                                sml = ((nsm << bm) - (1u << tml)) + __builtin_amdgcn_ubfe(Y, bo, bm);
                                sof = ((nso << bo) - (1u << tof)) + __builtin_amdgcn_ubfe(Y, 0u, bo);
                                if (GM & 1)
                                    ell_n = TLf(sll);
                                if (GM & 2)
                                    eof_n = TOf(sof);
                                if (GM & 4)
                                    eml_n = TMf(sml);
                                sr_done(b);
                                sr_issue<ONE>(b);
                                // o <= cap: no 32-bit overflow in these tests
                                if (ll + ml > cap - o)
                                    err = ZE_DST_SMALL;
                                else if (le - lp_ < ll)
                                    err = ZE_CORRUPT;
                                else if (off > o + ll)
                                    err = ZE_CORRUPT;
                                else if (!lemit(S, lp_, ll, (uint32_t)off, ml))
                                    err = ZE_GENERIC;
                                if (err)
                                    break;
                                lp_ += ll;
                                o += ll + ml;
                            }
                        };
                        const uint32_t tb = (uint32_t)(uintptr_t)lp<uint16_t>(mytab);
                        if (fit)
                            seqs([&](uint32_t x) -> uint32_t {
                                     return (GM & 1) ? (uint32_t)TL[x] : (uint32_t)*la<uint16_t>(tb + 2 * x);
                                 },
                                 [&](uint32_t x) -> uint32_t {
                                     return (GM & 2) ? (uint32_t)TO[x] : (uint32_t)*la<uint16_t>(tb + 2 * (nlll + x));
                                 },
                                 [&](uint32_t x) -> uint32_t {
                                     return (GM & 4) ? (uint32_t)TM[x]
                                                     : (uint32_t)*la<uint16_t>(tb + 2 * (nlll + nofl + x));
                                 });
                        else
                            seqs([&](uint32_t x) -> uint32_t { return TL[x]; }, [&](uint32_t x) -> uint32_t { return TO[x]; },
                                 [&](uint32_t x) -> uint32_t { return TM[x]; });
                      }
                        if (!err && b.cur - b.xs > 0)
                            err = ZE_CORRUPT;
                    }
                }
                if (!err) {
                    const uint32_t last = le - lp_;
                    if (o + last > cap)
                        err = ZE_DST_SMALL;
                    else if (last && !lemit<ONE>(S, lp_, last, 0, 0))
                        err = ZE_GENERIC;
                    else
                        o += last;
                }
            } else if (P.k == OP_RUN) {
                if (P.b > cap - o)
                    err = ZE_DST_SMALL;
                else if (P.b && !lemit<ONE>(S, P.a, P.b, 0, 0))
                    err = ZE_GENERIC;
                else
                    o += P.b;
            } else if (P.k == OP_FBEGIN) {
                rep0 = 1;
                rep1 = 4;
                rep2 = 8;
                o0 += o;
                cap -= o;
                o = 0;
            } else if (P.k == OP_FEND) {
                if ((P.a & 1) && (uint64_t)o != ((uint64_t)P.c << 32 | P.b))
                    err = ZE_CORRUPT;
                else if (P.a & 2) {
                    // a checksum request: the frame's range into its op
                    op[k].a = P.a | 4;
                    op[k].e = o0;
                    op[k].f = o;
                    c = 1ull << 63;
                }
            } else if (P.k == OP_ERR) {
                st = (int32_t)P.a;
                break;
            } else {   // OP_DONE (anything else: a list the frame kernel never wrote)
                st = P.k == OP_DONE ? (o == cap ? ST_OK : ST_SHORT_FRAME) : zerr(ZE_GENERIC);
                break;
            }
            if (err) {
                st = zerr(err);
                break;
            }
        }
    };
    auto irsrc = [&](uint64_t a, uint64_t b) {
        return __builtin_amdgcn_make_buffer_rsrc((void *)(items + a), 0, (int)(uint32_t)(8 * (b - a)), kRsrcDw3);
    };
    if (ONE || (hi > lo && hi - lo < kMaxSpan && 8 * (ihi - ilo) < kMaxSpan)) {
        // (ONE: one frame's span, < 4 GiB compressed and items)
        replay(span_rsrc(comp, lo, hi - lo), lo, irsrc(ilo, ihi), ilo);
    } else {
        for (uint64_t m = __ballot(true); m; m &= m - 1) {
            const int l = __builtin_ctzll(m);
            const uint64_t s0 = uni64(__shfl(d.c_off, l, 64)) & ~15ull;
            const uint64_t s1 = uni64(__shfl(d.c_off + d.c_size, l, 64));
            const uint64_t i0 = uni64(__shfl(rb, l, 64)), i1 = uni64(__shfl(rb + S.cap, l, 64));
            if ((int)lane == l)
                replay(span_rsrc(comp, s0, s1 - s0), s0, irsrc(i0, i1), i0);
        }
    }
    if (ONE && threadIdx.x != 0)
        return;
#ifdef ZSK_TUNING
    if (ONE) {
        atomicAdd(&g_sdiag[0], (unsigned long long)(__builtin_readcyclecounter() - tk0));
        atomicAdd(&g_sdiag[1], (unsigned long long)tloop);
        atomicAdd(&g_sdiag[5], (unsigned long long)tchain);
        atomicAdd(&g_sdiag[2], (unsigned long long)nseqs);
        atomicAdd(&g_sdiag[3], (unsigned long long)(__builtin_amdgcn_s_memrealtime() - rt0));
        atomicAdd(&g_sdiag[4], 1ull);
    }
#endif
    status[f] = st;
    nitems[f] = S.k;
    ck[f] = c;
    stop[f] = kstop;
    if (fail_at)
        fail_at[f] = st == ST_OK ? 0 : fa;
}

// After the Huffman and sequence kernels (which run side by side): a frame
// whose replay passed a literals op of a block with a corrupt Huffman stream
// fails there, as libzstd does — that block's literals are decoded before its
// sequences — with the items and output offset the replay had at that op.
__device__ __forceinline__ void lit_fix(uint32_t f, const uint8_t *__restrict__ ops,
                                        const uint64_t *__restrict__ blk_base, const uint8_t *__restrict__ hbad,
                                        const uint32_t *__restrict__ stop, int32_t *__restrict__ status,
                                        uint32_t *__restrict__ nitems, uint32_t *__restrict__ fail_at)
{
    const ZOp *op = reinterpret_cast<const ZOp *>(ops) + op_base(blk_base, f);
    const uint32_t ks = stop[f];
    for (uint32_t k = 0; k < ks; k++) {
        const ZOp P = op[k];
        if (P.k == OP_LIT && *reinterpret_cast<const uint32_t *>(hbad + 4ull * P.a)) {
            status[f] = zerr(ZE_CORRUPT);
            nitems[f] = P.b;
            if (fail_at)
                fail_at[f] = P.c;
            return;
        }
    }
}

}   // namespace
}   // namespace zsk
