// zstd_frame.hip -- the zstd decoder's frame kernel, a wave per seek-table
// entry (described at the kernel; its table builders are in zstd_tab_dev.h).
#include <stdio.h>
#include <stdlib.h>

#include "zstd_internal.h"

#ifdef ZSK_TUNING
// tuning builds: the frame kernel's cycles, lane 0 at section ends: [0]
// kernel, [1] Huffman descriptions, [2] sequence tables (+ slot cells), [3]
// window stagings, [4] frames, [5..7] the weights description: normalized
// counts, table, walk; printed under ZSEEK_ZFRAME_TIMERS
namespace zsk { namespace { __device__ unsigned long long g_zftime[12]; } }
#define ZF_T0(v) const uint64_t v = __builtin_readcyclecounter();
#define ZF_ADD(i, v)                                                                                  \
    if (lane_id() == 0)                                                                               \
        atomicAdd(&g_zftime[i], (unsigned long long)(__builtin_readcyclecounter() - v));
#else
#define ZF_T0(v)
#define ZF_ADD(i, v)
#endif
#include "zstd_tab_dev.h"

namespace zsk {
namespace {

using namespace lz4d;

constexpr uint32_t kZW = 2;          // waves (frames) per workgroup

// predefined distributions (RFC 8878 §3.1.1.3.2.2)
__constant__ int8_t c_ll_def[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                    2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
__constant__ int8_t c_ml_def[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
__constant__ int8_t c_of_def[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};

// HUF_selectDecoder (libzstd 1.4.9): the double-symbol decoder (X2) when its
// modelled time (+1/8 for its larger table) beats X1's, per compression-ratio
// bucket q and 256-byte output units.  dst >= 1.
__device__ __forceinline__ uint32_t huf_select_x2(uint32_t dst, uint32_t csrc)
{
    constexpr uint16_t kT[16][4] = {
        {0, 0, 1, 1},          {0, 0, 1, 1},          {38, 130, 1313, 74},   {448, 128, 1353, 74},
        {556, 128, 1353, 74},  {714, 128, 1418, 74},  {883, 128, 1437, 74},  {897, 128, 1515, 75},
        {926, 128, 1613, 75},  {947, 128, 1729, 77},  {1107, 128, 2083, 81}, {1177, 128, 2379, 87},
        {1242, 128, 2415, 93}, {1349, 128, 2644, 106}, {1455, 128, 2422, 124}, {722, 128, 1891, 145},
    };
    const uint32_t q = csrc >= dst ? 15u : csrc * 16u / dst, d256 = dst >> 8;
    const uint32_t t0 = kT[q][0] + kT[q][1] * d256;
    uint32_t t1 = kT[q][2] + kT[q][3] * d256;
    t1 += t1 >> 3;
    return t1 < t0 ? 1u : 0u;
}

// ---- frame kernel state ------------------------------------------------------------------
struct Frame {
    In I;
    uint32_t clen;     // compressed entry bytes
    uint64_t c_abs;    // comp coordinate of the entry
    uint64_t d_abs;    // literal-scratch coordinate of the entry
    uint8_t *lit;      // literal scratch of this frame (laid out like its output)
    uint32_t cap;      // output capacity (seek-table dSize)
    uint32_t lo;       // literal bytes placed in the scratch
    uint32_t huf_log;  // 0: no Huffman table yet
    uint32_t huf_slot; // block slot holding the current Huffman cells
    uint32_t tlog[3];  // LL / OF / ML table logs (valid flags below)
    uint32_t tvalid;   // bit t: table t valid
    ZOp *ops;          // this frame's op list
    uint32_t nop, op_cap;
    uint64_t blk0;     // first block slot of the frame
    uint32_t nblk, blk_cap;
    uint8_t *slots;
    HufJob *jobs;
    // the one-frame route's helper wave (HelpBox below): a posted Huffman
    // description (its block's jobs and table log completed at the block's end)
    struct HelpBox *help = nullptr;
    bool posted = false;
    uint32_t post_ns = 0;
};

// The one-frame route's frame kernel runs a second wave beside the frame's:
// a block's Huffman description (a serial walk of its weights, ~60K cycles)
// is decoded there while the frame's wave parses the block's sequence
// section (the FSE tables, ~90K) -- the description's size is known from its
// first byte, so nothing after it waits for its decode.  One box in LDS per
// workgroup; the waves meet at two barriers per posted description (A: posted
// or done, B: decoded).
struct HelpBox {
    uint32_t kind;   // 1 = decode the description at q (qn bytes) into slot g; 0 = done
    uint32_t q, qn;
    uint32_t g;
    uint32_t hs, lg;   // result: bytes used (0 = corrupt), table log
};

// append an op (wave-uniform; lane 0 writes).  The last slot is kept for the
// error that ends a list which would overflow.
__device__ __forceinline__ bool put_op(Frame &F, uint32_t k, uint32_t a = 0, uint32_t b = 0, uint32_t c = 0,
                                       uint32_t d = 0, uint32_t e = 0, uint32_t f = 0, uint32_t g = 0)
{
    if (F.nop + 1 >= F.op_cap && k != OP_ERR && k != OP_DONE)
        return false;
    if (lane_id() == 0)
        F.ops[F.nop] = ZOp{k, a, b, c, d, e, f, g};
    F.nop++;
    return true;
}

// write bytes [p, p + n) of v (16 bytes) into the literal scratch, clamped at
// the frame's capacity (corrupt frames may announce more literals)
__device__ __forceinline__ void lit_put(Frame &F, uint32_t p, u32x4 v, uint32_t n)
{
    if (p >= F.cap)
        return;
    if (p + n > F.cap)
        n = F.cap - p;
    store_exact(F.lit + p, v, n);
}

// Literals section at frame offset p (block bytes [p, p + n)) of the block
// with slot g; *used, *litn, *huf (Huffman streams queued).  Returns 0 or a
// zstd error.  Wave-wide.
__device__ __forceinline__ uint32_t literals(ZLds &L, Frame &F, uint64_t g, uint32_t p, uint32_t n,
                                             uint32_t *used, uint32_t *litn, bool *huf)
{
    const uint32_t lane = lane_id();
    *huf = false;
    if (n < 3)
        return ZE_CORRUPT;
    const uint32_t wx = stage_win(L, F.I, p);
    auto B = [&](uint32_t i) { return uni(wb(L, wx, F.I, p + i)); };
    const uint32_t b0 = B(0), type = b0 & 3, sf = (b0 >> 2) & 3;
    if (type <= 1) {
        uint32_t lh, size;
        if (sf == 1) {
            lh = 2;
            size = (b0 | B(1) << 8) >> 4;
        } else if (sf == 3) {
            lh = 3;
            size = (b0 | B(1) << 8 | B(2) << 16) >> 4;
        } else {
            lh = 1;
            size = b0 >> 3;
        }
        if (type == 0) {
            if (lh + size > n)
                return ZE_CORRUPT;
            // raw literals: wave copy compressed -> scratch
            const Span sp = make_span(F.I.base4 + F.I.s0, F.clen);
            for (uint32_t k = 16 * lane; k < size; k += 1024) {
                const u32x4 v = load16u(sp.r, sp.s0 + p + lh + k);
                lit_put(F, F.lo + k, v, size - k < 16 ? size - k : 16);
            }
            *used = lh + size;
        } else {
            if (lh + 1 > n || size > kZBlockMax)
                return ZE_CORRUPT;
            const uint32_t bv = B(lh) * 0x01010101u;
            for (uint32_t k = 16 * lane; k < size; k += 1024)
                lit_put(F, F.lo + k, (u32x4){bv, bv, bv, bv}, size - k < 16 ? size - k : 16);
            *used = lh + 1;
        }
        *litn = size;
        return 0;
    }
    if (n < 5)
        return ZE_CORRUPT;
    const uint32_t lhc = b0 | B(1) << 8 | B(2) << 16 | B(3) << 24;
    uint32_t lh, size, csize, ns = 4;
    if (sf <= 1) {
        ns = sf == 0 ? 1 : 4;
        lh = 3;
        size = (lhc >> 4) & 0x3FF;
        csize = (lhc >> 14) & 0x3FF;
    } else if (sf == 2) {
        lh = 4;
        size = (lhc >> 4) & 0x3FFF;
        csize = lhc >> 18;
    } else {
        lh = 5;
        size = (lhc >> 4) & 0x3FFFF;
        csize = (lhc >> 22) + (B(4) << 10);
    }
    if (size > kZBlockMax || csize + lh > n)
        return ZE_CORRUPT;
    uint32_t q = p + lh, qn = csize;
    if (type == 2) {
        // libzstd's decoder choice (ZSTD_decodeLiteralsBlock): one stream ->
        // X1; four -> HUF_decompress4X_hufOnly: no literals is an error, then
        // X1 or X2 by HUF_selectDecoder.  A treeless section reuses the
        // table's decoder (the X2 flag rides in huf_slot).
        if (ns == 4 && size == 0)
            return ZE_CORRUPT;
        const uint32_t x2 = ns == 4 ? huf_select_x2(size, csize) : 0u;
        uint32_t lg = 0, hs = 0;
        if (F.help) {
            // the helper wave decodes it; its size from its first byte (the
            // size checks huf_read makes before decoding)
            const uint32_t h0 = uni(wb(L, wx, F.I, q));
            if (h0 < 128) {
                if (1 + h0 > qn)
                    return ZE_CORRUPT;
                hs = 1 + h0;
            } else {
                const uint32_t bytes = (h0 - 127 + 1) / 2;
                if (1 + bytes > qn)
                    return ZE_CORRUPT;
                hs = 1 + bytes;
            }
            if (lane == 0) {
                F.help->kind = 1;
                F.help->q = q;
                F.help->qn = qn;
                F.help->g = (uint32_t)g;
            }
            __syncthreads();   // A: posted
            F.posted = true;
            lg = 1;   // (placeholder: the log arrives at the block's end)
        } else {
            ZF_T0(t0)
            hs = huf_read(L, F.I, wx, q, qn, &lg, reinterpret_cast<uint16_t *>(F.slots + g * kZSlot));
            ZF_ADD(1, t0)
            if (!hs)
                return ZE_CORRUPT;
        }
        F.huf_log = lg;
        F.huf_slot = (uint32_t)g | x2 << 27;
        q += hs;
        qn -= hs;
    } else if (!F.huf_log) {
        return ZE_DICT_CORRUPT;
    }
    uint32_t len[4] = {0, 0, 0, 0};
    if (ns == 1) {
        len[0] = qn;
    } else {
        if (qn < 10)
            return ZE_CORRUPT;
        const uint32_t wx2 = stage_win(L, F.I, q);
        auto C = [&](uint32_t i) { return uni(wb(L, wx2, F.I, q + i)); };
        len[0] = C(0) | C(1) << 8;
        len[1] = C(2) | C(3) << 8;
        len[2] = C(4) | C(5) << 8;
        if (len[0] + len[1] + len[2] + 6 > qn)
            return ZE_CORRUPT;
        len[3] = qn - 6 - len[0] - len[1] - len[2];
        if (3 * ((size + 3) / 4) > size)
            return ZE_CORRUPT;
        q += 6;
    }
    for (uint32_t k = 0; k < ns; k++)
        if (len[k] == 0)
            return ZE_CORRUPT;   // a stream without its end mark
    // one job per stream; the cells are in the slot of the block that sent the
    // table (this one, or an earlier one for a treeless literals section)
    const uint32_t lg = F.huf_log;
    if (lane < ns) {
        const uint32_t seg = ns == 1 ? size : (size + 3) / 4;
        const uint32_t off = q + (lane > 0 ? len[0] : 0) + (lane > 1 ? len[1] : 0) + (lane > 2 ? len[2] : 0);
        const uint32_t dst = F.lo + lane * seg;
        const uint32_t cnt = lane + 1 < ns ? seg : size - lane * seg;
        const uint32_t room = dst < F.cap ? F.cap - dst : 0;
        HufJob J;
        J.src = F.c_abs + off;
        J.dst = F.d_abs + dst;
        J.len = lane == 0 ? len[0] : lane == 1 ? len[1] : lane == 2 ? len[2] : len[3];
        J.cnt = cnt;
        J.lim = cnt < room ? cnt : room;
        J.tab = F.huf_slot | (F.posted ? 0u : lg << 28);   // (posted: the log is or-ed in later)
        F.jobs[4 * g + lane] = J;
    }
    F.post_ns = ns;
    *huf = true;
    *used = lh + csize;
    *litn = size;
    return 0;
}

// one of the sequence tables; returns bytes used, or ~0u with *err
__device__ __forceinline__ uint32_t seq_table(ZLds &L, Frame &F, uint32_t t, uint32_t mode, uint32_t p,
                              uint32_t avail, uint32_t *err)
{
    const uint32_t lane = lane_id();
    uint32_t *tab = L.fse[t];
    const uint32_t max_sym = t == 0 ? 35 : t == 1 ? 31 : 52, max_log = t == 1 ? 8 : 9;
    if (mode == 0) {
        const int8_t *def = t == 0 ? c_ll_def : t == 1 ? c_of_def : c_ml_def;
        const uint32_t nsym = t == 0 ? 36 : t == 1 ? 29 : 53, lg = t == 1 ? 5 : 6;
        for (uint32_t s = lane; s < nsym; s += 64)
            L.norm[s] = def[s];
        fse_build(L, tab, nsym, lg);
        F.tlog[t] = lg;
        F.tvalid |= 1u << t;
        return 0;
    }
    if (mode == 1) {
        if (avail == 0) {
            *err = ZE_SRC_WRONG;
            return ~0u;
        }
        const uint32_t wx = stage_win(L, F.I, p);
        const uint32_t sym = uni(wb(L, wx, F.I, p));
        if (sym > max_sym) {
            *err = ZE_CORRUPT;
            return ~0u;
        }
        if (lane == 0)
            *lp<uint32_t>(tab) = sym;
        F.tlog[t] = 0;
        F.tvalid |= 1u << t;
        return 1;
    }
    if (mode == 2) {
        const uint32_t wx = stage_win(L, F.I, p);
        uint32_t tl = 0, nsym = 0, e = 0, used = 0;
        norm_clear(L, max_sym + 1);
        ZF_T0(tn0)
        used = read_ncount(L, F.I.s0 + p - wx, avail, max_sym, max_log, &tl, &nsym, &e);
        ZF_ADD(8, tn0)
        if (uni(e) || uni(used) == 0) {
            *err = ZE_CORRUPT;
            return ~0u;
        }
        ZF_T0(tn1)
        fse_build(L, tab, uni(nsym), uni(tl));
        ZF_ADD(9, tn1)
        F.tlog[t] = uni(tl);
        F.tvalid |= 1u << t;
        return uni(used);
    }
    if (!((F.tvalid >> t) & 1)) {
        *err = ZE_CORRUPT;
        return ~0u;
    }
    return 0;
}

// One compressed block [p, p + n): literals, then the sequence section's
// header and tables -> the block's slot and ops.  Returns 0 or a zstd error.
// Wave-wide.
__device__ __forceinline__ uint32_t block_body(ZLds &L, Frame &F, uint32_t p, uint32_t n)
{
    const uint32_t lane = lane_id();
    if (n >= kZBlockMax)
        return ZE_SRC_WRONG;
    if (F.nblk >= F.blk_cap)
        return ZE_GENERIC;
    const uint64_t g = F.blk0 + F.nblk++;
    uint32_t lused = 0, litn = 0;
    bool huf = false;
    uint32_t e = literals(L, F, g, p, n, &lused, &litn, &huf);
    if (e)
        return e;
    if (huf && !put_op(F, OP_LIT, (uint32_t)g))
        return ZE_GENERIC;
    uint32_t q = p + lused;
    const uint32_t qe = p + n;
    if (q >= qe)
        return ZE_SRC_WRONG;
    const uint32_t wx = stage_win(L, F.I, q);
    auto B = [&](uint32_t i) { return uni(wb(L, wx, F.I, q + i)); };
    uint32_t nseq = B(0);
    // (a count of 0 written in a 2- or 3-byte form still has its mode byte and
    // table descriptions read, as ZSTD_decodeSeqHeaders does: only a first
    // byte of 0 ends the section)
    const bool tables = nseq != 0;
    if (nseq == 0) {
        if (qe - q != 1)
            return ZE_SRC_WRONG;
        q += 1;
    } else if (nseq == 255) {
        if (q + 3 > qe)
            return ZE_SRC_WRONG;
        nseq = (B(1) | B(2) << 8) + 0x7F00;
        q += 3;
    } else if (nseq > 127) {
        if (q + 2 > qe)
            return ZE_SRC_WRONG;
        nseq = ((nseq - 128) << 8) + B(1);
        q += 2;
    } else {
        q += 1;
    }
    uint32_t tl = 0;
    if (tables) {
        if (q + 1 > qe)
            return ZE_SRC_WRONG;
        const uint32_t modes = uni(wb(L, wx, F.I, q));
        q++;
        const uint32_t mode[3] = {modes >> 6, (modes >> 4) & 3, (modes >> 2) & 3};
        ZF_T0(t0)
#pragma unroll
        for (uint32_t t = 0; t < 3; t++) {
            uint32_t err = 0;
            const uint32_t u = seq_table(L, F, t, mode[t], q, qe - q, &err);
            if (u == ~0u)
                return err;
            q += u;
        }
        // the three tables -> the block's slot as u16 cells: symbol | next-state
        // rank ns << 6 (nbits and base follow from ns and the table log)
        uint16_t *dst = reinterpret_cast<uint16_t *>(F.slots + g * kZSlot + kSlotFse);
        ZF_T0(tn2)
        wave_lds_sync();
#pragma unroll
        for (uint32_t t = 0; t < 3; t++) {
            const uint32_t size = 1u << F.tlog[t];
            for (uint32_t u = lane; u < size; u += 64) {
                const uint32_t c = *lp<uint32_t>(&L.fse[t][u]);
                const uint32_t ns = ((c >> 16) + size) >> ((c >> 8) & 0xFF);
                dst[kFseOff[t] + u] = (uint16_t)((c & 0xFF) | ns << 6);
            }
        }
        tl = F.tlog[0] | F.tlog[1] << 4 | F.tlog[2] << 8;
        ZF_ADD(10, tn2)
        ZF_ADD(2, t0)
    }
    if (!put_op(F, OP_SEQ, nseq, q, qe > q ? qe - q : 0, F.lo, litn, (uint32_t)g, tl))
        return ZE_GENERIC;
    F.lo += litn;
    return 0;
}

// A block; with the helper wave, its posted Huffman description joined at the
// end: a corrupt description is the block's error (libzstd decodes the
// literals before the sequences), its ops dropped and its jobs cleared, else
// the table log goes into the block's jobs.
__device__ __forceinline__ uint32_t block(ZLds &L, Frame &F, uint32_t p, uint32_t n)
{
    const uint32_t nop0 = F.nop;
    const uint32_t e = block_body(L, F, p, n);
    if (!F.posted)
        return e;
    __syncthreads();   // B: decoded
    F.posted = false;
    const uint32_t lane = lane_id(), hs = F.help->hs, lg = F.help->lg, g = F.help->g;
    if (!hs) {
        if (lane < 4)
            F.jobs[4 * g + lane] = HufJob{0, 0, 0, 0, 0, 0};
        F.nop = nop0;
        F.huf_log = 0;
        return ZE_CORRUPT;
    }
    F.huf_log = lg;
    if (lane < F.post_ns)
        F.jobs[4 * g + lane].tab |= lg << 28;
    return e;
}

// One seek-table entry: every zstd frame in it (ZSTD_decompressDCtx) -> ops.
// Returns 0, or the zstd error at which the op list ends.
__device__ __forceinline__ uint32_t decode_entry(ZLds &L, Frame &F, uint32_t clen)
{
    const uint32_t lane = lane_id();
    uint32_t ip = 0, frames = 0;
    while (clen - ip >= 5) {
        uint32_t wx = stage_win(L, F.I, ip);
        auto B = [&](uint32_t i) { return uni(wb(L, wx, F.I, ip + i)); };
        const uint32_t magic = B(0) | B(1) << 8 | B(2) << 16 | B(3) << 24;
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
            if (clen - ip < 8)
                return ZE_SRC_WRONG;
            const uint64_t sk = 8 + (uint64_t)(B(4) | B(5) << 8 | B(6) << 16 | B(7) << 24);
            if (sk > clen - ip)
                return ZE_SRC_WRONG;
            ip += (uint32_t)sk;
            continue;
        }
        if (magic != kZMagic)
            return frames ? ZE_SRC_WRONG : ZE_PREFIX;
        frames++;
        const uint32_t n = clen - ip;
        if (n < 9)
            return ZE_SRC_WRONG;
        const uint32_t fhd = B(4);
        const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, csum = (fhd >> 2) & 1,
                       did = fhd & 3;
        const uint32_t dsz = did == 3 ? 4 : did;
        const uint32_t hsize = 5 + !single + dsz + (fcs_flag == 0 ? single : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8);
        if (n < hsize + 3)
            return ZE_SRC_WRONG;
        if (fhd & 0x08)
            return ZE_FRAMEPARAM;
        uint32_t h = 5;
        if (!single) {
            if ((B(h) >> 3) + 10 > 31)
                return ZE_WINDOW;
            h++;
        }
        uint32_t dict = 0;
        for (uint32_t i = 0; i < dsz; i++)
            dict |= B(h + i) << (8 * i);
        h += dsz;
        uint64_t fcs = ~0ull;
        if (fcs_flag == 0 && single)
            fcs = B(h);
        else if (fcs_flag == 1)
            fcs = (B(h) | B(h + 1) << 8) + 256;
        else if (fcs_flag == 2)
            fcs = B(h) | B(h + 1) << 8 | B(h + 2) << 16 | (uint64_t)B(h + 3) << 24;
        else if (fcs_flag == 3)
            fcs = (uint64_t)(B(h) | B(h + 1) << 8 | B(h + 2) << 16 | B(h + 3) << 24) |
                  ((uint64_t)(B(h + 4) | B(h + 5) << 8 | B(h + 6) << 16 | B(h + 7) << 24) << 32);
        if (dict)
            return ZE_DICT_WRONG;
        ip += hsize;
        // frame state
        F.huf_log = 0;
        F.tvalid = 0;
        if (!put_op(F, OP_FBEGIN))
            return ZE_GENERIC;
        for (;;) {
            if (clen - ip < 3)
                return ZE_SRC_WRONG;
            wx = stage_win(L, F.I, ip);
            const uint32_t bh = B(0) | B(1) << 8 | B(2) << 16;
            const uint32_t lastb = bh & 1, type = (bh >> 1) & 3, bsize = bh >> 3;
            const uint32_t csz = type == 1 ? 1 : bsize;
            if (type == 3)
                return ZE_CORRUPT;
            ip += 3;
            if (csz > clen - ip)
                return ZE_SRC_WRONG;
            if (type == 0 || type == 1) {
                // into the scratch (clamped at the capacity); the sequence
                // kernel checks the output room in order
                if (type == 0) {
                    const Span sp = make_span(F.I.base4 + F.I.s0, F.clen);
                    for (uint32_t k = 16 * lane; k < bsize; k += 1024) {
                        const u32x4 v = load16u(sp.r, sp.s0 + ip + k);
                        lit_put(F, F.lo + k, v, bsize - k < 16 ? bsize - k : 16);
                    }
                } else {
                    const uint32_t bv = uni(wb(L, wx, F.I, ip)) * 0x01010101u;
                    for (uint32_t k = 16 * lane; k < bsize; k += 1024)
                        lit_put(F, F.lo + k, (u32x4){bv, bv, bv, bv}, bsize - k < 16 ? bsize - k : 16);
                }
                if (!put_op(F, OP_RUN, F.lo, bsize))
                    return ZE_GENERIC;
                F.lo += bsize;
            } else {
                const uint32_t e = block(L, F, ip, bsize);
                if (e)
                    return e;
            }
            ip += csz;
            if (lastb)
                break;
        }
        uint32_t fl = fcs != ~0ull ? 1u : 0u, want = 0;
        bool trunc = false;
        if (csum) {
            if (clen - ip < 4) {
                trunc = true;
            } else {
                wx = stage_win(L, F.I, ip);
                want = B(0) | B(1) << 8 | B(2) << 16 | B(3) << 24;
                fl |= 2;
                ip += 4;
            }
        }
        if (!put_op(F, OP_FEND, fl, (uint32_t)fcs, (uint32_t)(fcs >> 32), want))
            return ZE_GENERIC;
        if (trunc)
            return ZE_CHECKSUM;
    }
    if (clen != ip)
        return ZE_SRC_WRONG;
    return 0;
}

// Frame kernel: one wave per seek-table entry.  Headers, literal sections
// (raw / RLE literals straight into the scratch), Huffman and FSE tables
// (built in LDS, stored to the block's slot), Huffman stream jobs and the op
// list the sequence kernel replays.
// HELP: one frame per workgroup, wave 1 the helper wave (HelpBox above);
// else kZW frames per workgroup, one per wave.
template <bool HELP>
__global__ __launch_bounds__(64 * kZW) __attribute__((amdgpu_waves_per_eu(4))) void zstd_frame_kernel(
    const FrameDesc *__restrict__ desc, uint32_t n, const uint8_t *__restrict__ comp,
    uint8_t *__restrict__ lit, uint64_t lit_cap, const uint64_t *__restrict__ rec_base,
    uint64_t capacity, const uint64_t *__restrict__ blk_base, uint8_t *__restrict__ ops,
    uint8_t *__restrict__ slots, uint8_t *__restrict__ jobs, uint32_t f0, const uint64_t *__restrict__ fit)
{
    static_assert(kZW >= 2, "the helper wave needs a second ZLds");
    __shared__ ZLds lds[kZW];
    __shared__ HelpBox box;
    // (the asynchronous decode: a batch that did not fit its bounds; the
    // whole workgroup, before any barrier)
    if (fit && *fit)
        return;
    ZF_T0(tk)
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t f = HELP ? uni(f0 + blockIdx.x) : uni(f0 + blockIdx.x * kZW + w);   // frames [f0, n)
    if (f >= n)
        return;   // (HELP: the whole workgroup)
    ZLds &L = lds[w];
    const FrameDesc d = desc[f];
    Frame F;
    if (HELP && w == 1) {
        // helper: the frame's In, then the posted descriptions until done
        const uintptr_t fa = reinterpret_cast<uintptr_t>(comp + d.c_off);
        F.I.base4 = reinterpret_cast<const uint8_t *>(fa & ~(uintptr_t)3);
        F.I.s0 = (uint32_t)(fa & 3);
        F.I.amax = d.c_size ? (F.I.s0 + d.c_size - 1) & ~3u : 0;
        for (;;) {
            __syncthreads();   // A
            if (uni(box.kind) == 0)
                break;
            const uint32_t q = uni(box.q), qn = uni(box.qn), g = uni(box.g);
            const uint32_t wx = stage_win(L, F.I, q);
            uint32_t lg = 0;
            ZF_T0(t0)
            const uint32_t hs = huf_read(L, F.I, wx, q, qn, &lg, reinterpret_cast<uint16_t *>(slots + (uint64_t)g * kZSlot));
            ZF_ADD(1, t0)
            if (lane_id() == 0) {
                box.hs = hs;
                box.lg = lg;
            }
            __syncthreads();   // B
        }
        return;
    }
    if (HELP)
        F.help = &box;
    const uintptr_t fa = reinterpret_cast<uintptr_t>(comp + d.c_off);
    F.I.base4 = reinterpret_cast<const uint8_t *>(fa & ~(uintptr_t)3);
    F.I.s0 = (uint32_t)(fa & 3);
    F.I.amax = d.c_size ? (F.I.s0 + d.c_size - 1) & ~3u : 0;
    F.c_abs = d.c_off;
    F.d_abs = d.d_off;
    F.lit = lit + d.d_off;
    F.clen = d.c_size;
    F.cap = d.d_size;
    F.lo = 0;
    F.huf_log = 0;
    F.tvalid = 0;
    F.tlog[0] = F.tlog[1] = F.tlog[2] = 0;
    const uint64_t ob = op_base(blk_base, f);
    F.ops = reinterpret_cast<ZOp *>(ops) + ob;
    F.nop = 0;
    F.op_cap = (uint32_t)(op_base(blk_base, f + 1) - ob);
    F.blk0 = blk_base[f];
    F.nblk = 0;
    F.blk_cap = (uint32_t)(blk_base[f + 1] - F.blk0);
    F.slots = slots;
    F.jobs = reinterpret_cast<HufJob *>(jobs);
    // this frame's Huffman jobs zeroed (a block without Huffman literals, or
    // one the frame never reaches, has no streams) -- no memset of the whole
    // job array per launch; ordered before the jobs literals() writes
    for (uint32_t i = lane_id(); i < 4 * F.blk_cap; i += 64)
        F.jobs[4 * F.blk0 + i] = HufJob{0, 0, 0, 0, 0, 0};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    uint32_t e;
    // scratch sized by the plan: a frame that would not fit is refused, never
    // written out of bounds
    if (rec_base[f + 1] > capacity || d.c_size >= 0x7FFFFF00u ||
        d.d_off + (uint64_t)d.d_size + 16 > lit_cap)
        e = ZE_GENERIC;
    else
        e = decode_entry(L, F, d.c_size);
    if (e)
        put_op(F, OP_ERR, (uint32_t)zerr(e));
    else
        put_op(F, OP_DONE);
    if (HELP) {
        if (lane_id() == 0)
            box.kind = 0;
        __syncthreads();   // A: done
    }
    ZF_ADD(0, tk)
#ifdef ZSK_TUNING
    if (lane_id() == 0)
        atomicAdd(&g_zftime[4], 1ull);
#endif
}

}   // namespace

void launch_zstd_frame(const ZstdCall &C, ZstdScratch *s, const ZstdChunk &c, bool help, hipStream_t stream)
{
    static const bool help_off = env_is_zero("ZSEEK_FRAME_HELP");
    const uint32_t m = c.f1 - c.f0;
    const auto go = [&](auto kernel, uint32_t groups) {
        hipLaunchKernelGGL(kernel, dim3(groups), dim3(64 * kZW), 0, stream, C.desc, c.f1, C.comp, s->lit, s->lit_cap,
                           s->rec_base, s->items_cap, s->blk_base, s->ops, s->slots, s->hjobs, c.f0, C.fit);
    };
    if (help && !help_off)
        go(zstd_frame_kernel<true>, m);
    else
        go(zstd_frame_kernel<false>, (m + kZW - 1) / kZW);
#ifdef ZSK_TUNING
    static const bool ztimers = getenv("ZSEEK_ZFRAME_TIMERS") != nullptr;
    static int zcalls = 0;
    if (ztimers && ++zcalls % 100 == 0) {
        unsigned long long z[12] = {0};
        (void)hipMemcpyFromSymbolAsync(z, HIP_SYMBOL(g_zftime), sizeof(z), 0, hipMemcpyDeviceToHost, stream);
        (void)hipStreamSynchronize(stream);
        const double fr = z[4] ? (double)z[4] : 1.0;
        fprintf(stderr,
                "zstd frame kernel cycles per frame: total %.0f huffman descriptions %.0f sequence tables %.0f "
                "window stagings %.0f | weights: ncount %.0f build %.0f walk %.0f | sequence tables: "
                "ncount %.0f build %.0f cells out %.0f (%llu frames)\n",
                z[0] / fr, z[1] / fr, z[2] / fr, z[3] / fr, z[5] / fr, z[6] / fr, z[7] / fr, z[8] / fr,
                z[9] / fr, z[10] / fr, z[4]);
    }
#endif
}

}   // namespace zsk
