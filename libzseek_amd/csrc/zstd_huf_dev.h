// zstd_huf_dev.h -- Huffman literal streams on the device (kernels in
// zstd_huf_seq.hip): the backward bit reader, the lane-per-stream decoder,
// libzstd's X2 decoder for streams X1 rejects, the workgroup-per-stream one.
#pragma once

#include "zstd_dev.h"

namespace zsk {
namespace {

using namespace lz4d;

// ---- backward bitstreams, lane per stream -------------------------------------------
// Bits of one stream of comp, read from its end: C holds stream bits
// [pos, pos + nb) (coordinates in bits from the stream's 16-aligned chunk
// base x0; bits below the stream's first byte read as 0).  The lane's stream
// bytes pass through a ring of kRS 16-byte slots in LDS (dword k of slot s of
// lane l at ring base + s * 1024 + k * 256 + 4 * l: a wave's ring reads hit 64
// different banks whatever dword each lane reads): br_step, once per decode step at a fixed
// place in the loop, commits the chunk loaded one step earlier and issues the
// next load — unconditionally, re-fetching the last chunk when the ring is
// full — so no load result is ever waited for in the step that issued it and
// no load sits in a divergent branch.  br_fill refills C from the ring.  The
// buffer resource is wave-uniform (a span of comp covering the wave's
// streams); x0 is the lane's offset in it.
constexpr int32_t kRS = 4;

struct BRd {
    __amdgpu_buffer_rsrc_t r;
    uint64_t C;
    u32x4 P, P2;     // chunks `pend`, `pend2`, committed to the ring at the next step
    uint32_t x0;
    uint32_t ring;   // LDS address of this lane's dword 0 of slot 0
    int32_t nb, pos, xs;
    int32_t pq;      // next chunk to fetch (decreasing; < 0 reads zeros)
    int32_t pend, pend2;
};

__device__ __forceinline__ u32x4 chunk16(const BRd &b, int32_t q)
{
    return __builtin_bit_cast(
        u32x4, __builtin_amdgcn_raw_buffer_load_b128(b.r, q >= 0 ? b.x0 + 16u * (uint32_t)q : kOOR, 0, 0));
}

__device__ __forceinline__ uint32_t slot_addr(const BRd &b, int32_t q)
{
    return b.ring + (uint32_t)(q & (kRS - 1)) * 1024u;
}

__device__ __forceinline__ void slot_put(const BRd &b, int32_t q, u32x4 v)
{
    const uint32_t a = slot_addr(b, q);
    *la<uint32_t>(a) = v.x;
    *la<uint32_t>(a + 256) = v.y;
    *la<uint32_t>(a + 512) = v.z;
    *la<uint32_t>(a + 768) = v.w;
}

// The stream at offset x (len >= 1 bytes) of resource r, ring at LDS address
// ring.  False when its last byte (the end mark) is 0.
__device__ __forceinline__ bool br_init(BRd &b, __amdgpu_buffer_rsrc_t r, uint32_t x, uint32_t len, uint32_t ring,
                                        bool d2 = false)
{
    b.r = r;
    b.ring = ring;
    b.x0 = x & ~15u;
    const uint32_t rel = (x & 15u) + len;   // bytes from x0 to the stream's end
    b.xs = 8 * (int32_t)(x & 15u);
    const uint32_t last = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, b.x0 + rel - 1, 0, 0);
    const int32_t xm = 8 * (int32_t)(rel - 1) + (last ? 31 - __builtin_clz(last) : 0);
    const int32_t D = xm >> 5, i = D & 3, q = D >> 2;
    u32x4 c[kRS - 1];
#pragma unroll
    for (int k = 0; k < kRS - 1; k++)
        c[k] = chunk16(b, q - k);
#pragma unroll
    for (int k = 0; k < kRS - 1; k++)
        slot_put(b, q - k, c[k]);
    b.pq = q - (kRS - 1);
    b.P = chunk16(b, b.pq);
    b.P2 = b.P;
    b.pend = b.pend2 = b.pq;
    b.pq--;
    const uint32_t top = i == 3 ? c[0].w : i == 2 ? c[0].z : i == 1 ? c[0].y : c[0].x;
    b.pos = 32 * D;
    b.C = top & ((1u << (xm & 31)) - 1) & above(b.xs, b.pos);
    b.nb = xm & 31;
    if (d2) {   // a second chunk in flight (br_step<1, 2>), room permitting
        const int32_t qcur = (b.pos - 32) >> 7;
        const bool room = b.pq >= qcur - (kRS - 1);
        const int32_t t = room ? b.pq : b.pq + 1;
        b.P2 = chunk16(b, t);
        b.pend2 = t;
        b.pq = room ? b.pq - 1 : b.pq;
    }
    return last != 0;
}

// Once per decode step: commit the pending chunk(s), fetch the next one(s)
// (F = 1 or 2 chunks per step).  D = 2 (with F = 1): two chunks in flight,
// each committed two steps after its load, so the load's wait never waits
// on the literal store of the step just before it (vmcnt retires in issue
// order): a store has two steps to land instead of one.  A room check at
// issue suffices: the slot it fills held a chunk above the one then in use.
template <int F = 1, int D = 1>
__device__ __forceinline__ void br_step(BRd &b)
{
    if (D == 2) {
        slot_put(b, b.pend, b.P);
        b.P = b.P2;
        b.pend = b.pend2;
        const int32_t qcur = (b.pos - 32) >> 7;
        const bool room = b.pq >= qcur - (kRS - 1);
        const int32_t t = room ? b.pq : b.pq + 1;
        b.P2 = chunk16(b, t);
        b.pend2 = t;
        b.pq = room ? b.pq - 1 : b.pq;
        return;
    }
    slot_put(b, b.pend, b.P);
    if (F == 2)
        slot_put(b, b.pend2, b.P2);
    const int32_t qcur = (b.pos - 32) >> 7;   // chunk of the next dword to absorb
    bool room = b.pq >= qcur - (kRS - 1);
    int32_t t = room ? b.pq : b.pq + 1;
    b.P = chunk16(b, t);
    b.pend = t;
    b.pq = room ? b.pq - 1 : b.pq;
    if (F == 2) {
        room = b.pq >= qcur - (kRS - 1);
        t = room ? b.pq : b.pq + 1;
        b.P2 = chunk16(b, t);
        b.pend2 = t;
        b.pq = room ? b.pq - 1 : b.pq;
    }
}

// refill C to >= 32 bits when below (branch-free)
__device__ __forceinline__ void br_fill(BRd &b)
{
    const int32_t p2 = b.pos - 32, dw = p2 >> 5;
    const uint32_t v = *la<uint32_t>(slot_addr(b, dw >> 2) + 256u * (uint32_t)(dw & 3)) & above(b.xs, p2);
    const bool need = b.nb < 32;
    b.C = need ? (b.C << 32) | v : b.C;
    b.nb = need ? b.nb + 32 : b.nb;
    b.pos = need ? p2 : b.pos;
}

// stream bits not consumed yet (< 0 once read past the start)
__device__ __forceinline__ int32_t br_left(const BRd &b)
{
    return b.pos + b.nb - b.xs;
}

// ---- Huffman literals: one lane per stream -------------------------------------------
// 16 blocks (64 streams) per wave; their tables packed into LDS when they fit
// (else read from the slots).  Cells are nbits | symbol << 8.  In the main
// loop a lane refills its bit container every G symbols (G * lg <= 32) and
// decodes those G symbols from a 32-bit MSB-first window w of the
// container's top bits: index = w >> (32 - lg), consume = w <<= cell (the
// shift takes the cell's low 5 bits, nbits).  16 decoded bytes are stored at
// a time, aligned.
constexpr uint32_t kHufLdsCells = 2048;

template <int G, int F, int DIAG, int B = 4, typename Tab>
__device__ __forceinline__ void huf_stream(BRd &b, Tab T, uint32_t lg, uint8_t *out, uint64_t dst, uint32_t cnt,
                                           uint32_t lim)
{
    const uint32_t mask = (1u << lg) - 1, sh = 32 - lg;
    auto one = [&]() -> uint32_t {
        const uint32_t e = T((uint32_t)(b.C >> (uint32_t)(b.nb - (int32_t)lg)) & mask);
        b.nb -= (int32_t)(e & 0xFF);
        return e >> 8;
    };
    uint32_t i = 0;
    // head (< 16 symbols, <= 180 bits): the ring holds kRS - 1 chunks after br_init
    while (i < cnt && ((dst + i) & 15)) {
        br_fill(b);
        const uint32_t s = one();
        if (i < lim)
            out[i] = (uint8_t)s;
        i++;
    }
    // 16 symbols per step
    auto step16 = [&]() -> u32x4 {
        if (!(DIAG & 2))
            br_step<F, F == 1 ? 2 : 1>(b);
        u32x4 acc = {0, 0, 0, 0};
        uint32_t w = 0, used = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k % G == 0) {
                b.nb -= (int32_t)used;
                br_fill(b);
                w = (uint32_t)(b.C >> (uint32_t)(b.nb - 32));
                used = 0;
            }
            const uint32_t e = (DIAG & 4) ? (w >> 26) << 8 | 6u : T(w >> sh);
            w <<= (e & 31);   // nbits
            used += e & 0xFF;
            if ((k & 3) == 0)
                acc[k >> 2] = e >> 8;
            else
                acc[k >> 2] |= (e >> 8) << (8 * (k & 3));
        }
        b.nb -= (int32_t)used;
        return acc;
    };
    auto put16 = [&](uint32_t at, const u32x4 &v) {
        if (!(DIAG & 1))
            *reinterpret_cast<u32x4 *>(out + at) = v;
    };
    // to a 128-byte boundary of the output, a step at a time
    while (i + 16 <= lim && ((dst + i) & (16 * B - 1))) {
        const u32x4 v = step16();
        put16(i, v);
        i += 16;
    }
    // then 4 steps per iteration and their 64 bytes stored back to back: a
    // line arrives in two halves, where 16-byte stores a step apart left
    // partial lines in L2 to be evicted (and merged in HBM) under this
    // kernel's write load (5.2 -> 3.9 ms; no stores at all: 1.9 ms; 8 steps
    // need more than the 128 VGPRs four waves per SIMD leave: spills).
    // Round 3, config 5 (6-bit codes, kernels serialized): 2.90 ms; without
    // the stores 1.85, also without the ring refills 1.33, also without the
    // lookups 0.58.  Neither 128-byte bursts (three waves per SIMD) nor
    // keeping the second step's chunk wait clear of the stores just issued
    // (the loop head's wait-count merge made it wait for them) moved it;
    // nontemporal stores doubled it (6.03 ms: L2 write-combining is doing
    // real work here).
    while (i + 16 * B <= lim) {
        u32x4 v[B];
#pragma unroll
        for (int k = 0; k < B; k++)
            v[k] = step16();
#pragma unroll
        for (int k = 0; k < B; k++)
            put16(i + 16 * k, v[k]);
        i += 16 * B;
    }
    while (i + 16 <= lim) {
        const u32x4 v = step16();
        put16(i, v);
        i += 16;
    }
    while (i < cnt) {
        br_step<F, F == 1 ? 2 : 1>(b);
        br_fill(b);
        const uint32_t s = one();
        if (i < lim)
            out[i] = (uint8_t)s;
        i++;
    }
}

// ---- libzstd's X2 decoder on a stream X1 rejects --------------------------------------
// On a valid stream X1 and X2 decode the same bytes; they differ only on
// streams X1 rejects (HUF_decodeLastSymbolX2: at a stream's last output byte a
// two-symbol cell consumes both codes' bits, clamped at the stream's start,
// and a read with no bits left looks at the bit container's top bits).  So a
// lane keeps the fast X1 walk and, for an X2 stream it rejected, re-walks it
// here in X2 cells (tests/test_zstd_oracle.py pins the rule the oracle and
// this walk share against libzstd 1.4.9).  The re-walk reads one cell at a
// time; only streams that failed X1 -- corrupt ones -- pay for it.

// the stream at byte x of resource r, read backward through a 64-bit window
// (two dwords, reloaded when a read leaves it: one load per ~4 cells)
struct X2Bits {
    __amdgpu_buffer_rsrc_t r;
    uint32_t x;
    uint32_t wlo;   // absolute bit of the window's bit 0 (a multiple of 32)
    uint64_t w;
    // bits [q - n, q) (bit q - 1 most significant), bits below the stream's
    // first byte 0; n <= 12
    __device__ uint32_t get(int32_t q, uint32_t n)
    {
        if (q <= 0)
            return 0;
        const int32_t lo = q - (int32_t)n, l0 = lo > 0 ? lo : 0;
        const uint32_t a = 8 * x + (uint32_t)l0, e = 8 * x + (uint32_t)q;
        if (a < wlo || e > wlo + 64) {
            const uint32_t d = a >> 5;
            w = (uint64_t)(uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, 4 * d, 0, 0) |
                (uint64_t)(uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, 4 * d + 4, 0, 0) << 32;
            wlo = 32 * d;
        }
        const uint32_t bits = (uint32_t)(w >> (a - wlo)) & ((1u << (uint32_t)(q - l0)) - 1);
        return lo < 0 ? bits << (uint32_t)(-lo) : bits;
    }
};

// X2 result of the stream (len bytes at x, cnt symbols, cells tab of table
// log lg): bit 0 ok; bit 16: the last byte is bits 8..15 (a read with no
// bits left), else the X1 walk's bytes stand.
__device__ __attribute__((noinline)) uint32_t x2_rescue(__amdgpu_buffer_rsrc_t r, uint32_t x, uint32_t len,
                                                        uint32_t cnt, const uint16_t *tab, uint32_t lg)
{
    const uint32_t last = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, x + len - 1, 0, 0);
    if (!last || !cnt)
        return 0;
    int32_t rr = 8 * (int32_t)(len - 1) + (31 - __builtin_clz(last));   // bits below the end mark
    X2Bits B{r, x, 0xFFFFFFC0u, 0};
    auto Z = [&](int32_t q) -> uint32_t { return tab[B.get(q, lg)]; };
    uint32_t p = 0;
    while (p + 2 <= cnt) {   // HUF_decodeStreamX2's cells before the last byte
        if (rr <= 0)
            return 0;
        const uint32_t nb1 = Z(rr) & 0xFF, nb2 = Z(rr - (int32_t)nb1) & 0xFF;
        const bool two = nb1 + nb2 <= 12;
        p += two ? 2 : 1;
        rr -= (int32_t)(two ? nb1 + nb2 : nb1);
    }
    if (p == cnt)
        return rr == 0 ? 1u : 0u;
    if (rr > 0) {   // HUF_decodeLastSymbolX2
        const uint32_t nb1 = Z(rr) & 0xFF, nb2 = Z(rr - (int32_t)nb1) & 0xFF;
        if (nb1 + nb2 <= 12)
            return rr <= (int32_t)(nb1 + nb2) ? 1u : 0u;
        return rr == (int32_t)nb1 ? 1u : 0u;
    }
    if (rr < 0)
        return 0;
    // no bits left: the cell at the container's top 12 bits (the stream's
    // first 8 bytes, zero past its end); only a two-symbol cell leaves it
    // consumed exactly
    uint64_t c = 0;
    for (uint32_t i = 0; i < 8 && i < len; i++)
        c |= (uint64_t)(uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, x + i, 0, 0) << (8 * i);
    const uint32_t v = (uint32_t)(c >> 52);
    const uint32_t g1 = tab[v >> (12 - lg)], nb1 = g1 & 0xFF;
    const uint32_t nb2 = tab[((v << nb1) & 0xFFF) >> (12 - lg)] & 0xFF;
    if (nb1 + nb2 > 12)
        return 0;
    return 1u | 0x10000u | (g1 >> 8) << 8;
}

// ---- Huffman literals, the one-frame route: a workgroup per stream ----------------------
// A lone frame's four streams on four lanes were a 366 us serial chain (~130
// cycles a symbol: an LDS lookup per symbol).  Here 256 threads split the
// stream's bits into chunks and decode them at once.  A symbol boundary at a
// chunk's top is unknown until the chunks above are decoded, but it lies in
// the top lg bits of the chunk (no code is longer than lg): so each thread
// decodes its chunk from every one of those lg entry bits (lockstep, ILP over
// the entries), recording for each entry where the walk leaves the chunk and
// how many symbols it took.  One thread then follows the true entries from
// the stream's end mark chunk by chunk (the exit of one chunk is the next
// one's entry), giving each chunk its entry and output base; a second pass
// decodes each chunk from its true entry into an LDS copy of the output,
// written out in 16-byte stores.  Identical bytes to the serial walk (the
// same cells and bit reads, bits below the stream read as 0): a stream is
// valid iff the followed walk makes exactly cnt symbols and ends at bit 0.
// Anything else -- a stream the walk rejects (X2 rescue), too long for the
// stage, an empty end mark -- is decoded by thread 0 exactly as
// zstd_huf_kernel's lane does.
constexpr uint32_t kHufOneT = 256;
constexpr uint32_t kHufOneStage = 65536;    // stream bytes staged (else the serial walk)
constexpr uint32_t kHufOneOut = 32768;      // symbols staged (else the serial walk)
constexpr uint32_t kHufOneMaxLg = 12;

// its LDS (a struct: the one-frame decode kernel below shares it with the
// sequence replay's, as a union)
struct HufOneLds {
    __attribute__((aligned(16))) uint8_t sst[16 + kHufOneStage + 32];
    __attribute__((aligned(16))) uint8_t obuf[kHufOneOut + 16];
    __attribute__((aligned(16))) uint16_t tab[1u << kHufOneMaxLg];
    uint32_t cand[kHufOneT * kHufOneMaxLg];   // exit offset | symbols << 8, per chunk and entry
    uint32_t ent[kHufOneT];                   // true entry | output base << 4
    uint32_t verdict;
    __attribute__((aligned(16))) uint8_t rings[kRS * 1024];   // the serial walk's ring
};

// job j by the workgroup's kHufOneT threads (t = thread index)
__device__ __forceinline__ void huf_one_body(HufOneLds &H, uint32_t j, uint32_t t, const uint8_t *__restrict__ jobs,
                                             const uint8_t *__restrict__ comp, const uint8_t *__restrict__ slots,
                                             uint8_t *__restrict__ lit, uint8_t *__restrict__ hbad)
{
    auto &sst = H.sst;
    auto &obuf = H.obuf;
    auto &tab = H.tab;
    auto &cand = H.cand;
    auto &ent = H.ent;
    auto &verdict = H.verdict;
    auto &rings = H.rings;
    const HufJob J = reinterpret_cast<const HufJob *>(jobs)[j];
    if (J.len == 0) {
        if (t == 0)
            hbad[j] = 0;
        return;
    }
    const uint32_t lg = J.tab >> 28, jslot = J.tab & kHufSlotMask, jx2 = (J.tab >> 27) & 1;
    const uint16_t *gt = reinterpret_cast<const uint16_t *>(slots + (uint64_t)jslot * kZSlot);
    const uint64_t s0 = J.src & ~15ull;
    const __amdgpu_buffer_rsrc_t r = span_rsrc(comp, s0, J.src + J.len - s0);
    const uint32_t x = (uint32_t)(J.src - s0);
    const uint32_t sl = ldsaddr(sst) + 16;
    bool par = J.len <= kHufOneStage && J.cnt <= kHufOneOut && lg >= 1 && lg <= kHufOneMaxLg;
    if (par) {
        // the stream's bytes (16 zero bytes below them), the cells
        if (t < 4)
            *la<uint32_t>(sl - 16 + 4 * t) = 0;
        for (uint32_t q = 16 * t; q < J.len; q += 16 * kHufOneT)
            *la<u32x4>(sl + q) = load16u(r, x + q);
        for (uint32_t c = t; c < (1u << lg); c += kHufOneT)
            tab[c] = gt[c];
        __syncthreads();
    }
    const uint32_t last = par ? (uint32_t)*la<uint8_t>(sl + J.len - 1) : 0u;
    par = par && last != 0;
    if (par) {
        const int32_t S = 8 * (int32_t)(J.len - 1) + (31 - __builtin_clz(last));   // bits below the end mark
        const uint32_t mask = (1u << lg) - 1;
        // lg bits below bit p (bit p - 1 most significant); bits below 0 read 0
        auto cell = [&](int32_t p) -> uint32_t {
            const int32_t lo = p - (int32_t)lg;
            const int32_t d = lo >> 5;   // >= -1: the zero bytes below
            const uint32_t a = (uint32_t)((int32_t)sl + 4 * d);
            const uint64_t w = (uint64_t)*la<uint32_t>(a) | (uint64_t)*la<uint32_t>(a + 4) << 32;
            return tab[(uint32_t)(w >> (uint32_t)(lo - 32 * d)) & mask];
        };
        // chunks of C >= 16 bits (> lg), at most kHufOneT of them, each with
        // bits: hi > 0
        const int32_t C = max<int32_t>(16, (S + (int32_t)kHufOneT - 1) / (int32_t)kHufOneT);
        const uint32_t T = (uint32_t)max<int32_t>(1, (S + C - 1) / C);
        const int32_t hi = S - (int32_t)t * C, lo = max(hi - C, 0);
        if (t < T) {
            const uint32_t ne = t == 0 ? 1u : lg;
            int32_t pc[kHufOneMaxLg];
            uint32_t nc[kHufOneMaxLg];
#pragma unroll
            for (uint32_t c = 0; c < kHufOneMaxLg; c++) {
                pc[c] = hi - (int32_t)c;
                nc[c] = 0;
            }
            for (bool any = true; any;) {
                any = false;
#pragma unroll
                for (uint32_t c = 0; c < kHufOneMaxLg; c++) {
                    if (c < ne && pc[c] > lo) {
                        const uint32_t e = cell(pc[c]);
                        pc[c] -= (int32_t)max(e & 0xFFu, 1u);
                        nc[c]++;
                        any = true;
                    }
                }
            }
#pragma unroll
            for (uint32_t c = 0; c < kHufOneMaxLg; c++)
                if (c < ne)
                    cand[t * kHufOneMaxLg + c] = (uint32_t)(lo - pc[c]) | nc[c] << 8;
        }
        __syncthreads();
        if (t == 0) {
            uint32_t c = 0, base = 0;
            for (uint32_t k = 0; k < T; k++) {
                ent[k] = c | base << 4;
                const uint32_t v = cand[k * kHufOneMaxLg + c];
                base += v >> 8;
                c = v & 0xFF;
            }
            verdict = c == 0 && base == J.cnt ? 1u : 0u;
        }
        __syncthreads();
        par = verdict != 0;
        if (par) {
            if (t < T) {
                const uint32_t e0 = ent[t];
                int32_t p = hi - (int32_t)(e0 & 15);
                for (uint32_t i = e0 >> 4; p > lo; i++) {
                    const uint32_t e = cell(p);
                    obuf[i] = (uint8_t)(e >> 8);
                    p -= (int32_t)max(e & 0xFFu, 1u);
                }
            }
            __syncthreads();
            // out: [0, lim) of the decoded symbols, 16-byte stores where aligned
            uint8_t *out = lit + J.dst;
            const uint32_t n = J.lim, head = min(n, (uint32_t)((16 - ((uintptr_t)out & 15)) & 15));
            if (t < head)
                out[t] = obuf[t];
            const uint32_t nq = (n - head) / 16;
            for (uint32_t q = t; q < nq; q += kHufOneT)
                *reinterpret_cast<u32x4 *>(out + head + 16 * q) = *la<u32x4_u>(ldsaddr(obuf) + head + 16 * q);
            const uint32_t tail = head + 16 * nq;
            if (tail + t < n)
                out[tail + t] = obuf[tail + t];
            if (t == 0)
                hbad[j] = 0;
            return;
        }
    }
    // the serial walk (zstd_huf_kernel's lane), thread 0
    if (t != 0)
        return;
    BRd b;
    bool bad = !br_init(b, r, x, J.len, ldsaddr(rings));
    auto Tg = [&](uint32_t i) -> uint32_t { return gt[i]; };
    huf_stream<2, 2, 0, 4>(b, Tg, lg, lit + J.dst, J.dst, J.cnt, J.lim);
    bad = bad || br_left(b) != 0;
    if (bad && jx2) {
        const uint32_t xr = x2_rescue(r, x, J.len, J.cnt, gt, lg);
        bad = !(xr & 1);
        if ((xr & 0x10000) && J.cnt - 1 < J.lim)
            lit[J.dst + J.cnt - 1] = (uint8_t)(xr >> 8);
    }
    hbad[j] = bad ? 1 : 0;
}

}   // namespace
}   // namespace zsk
