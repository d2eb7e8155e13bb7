// zstd_tab_dev.h -- the frame kernel's table builders: its LDS per wave, the
// forward window, FSE counts and tables, Huffman tree descriptions.  Included
// by zstd_frame.hip alone, after its section timers (ZF_T0 / ZF_ADD, g_zftime).
#pragma once
#ifndef ZF_T0
#error "zstd_frame.hip defines ZF_T0 / ZF_ADD before it includes zstd_tab_dev.h"
#endif

#include "zstd_dev.h"

namespace zsk {
namespace {

using namespace lz4d;

// LDS per wave of the frame kernel
struct ZLds {
    uint32_t fse[3][512];     // LL / OF / ML cells: symbol | nbits << 8 | base << 16
    __attribute__((aligned(8))) uint8_t win[256];   // forward window: headers, table descriptions
    uint32_t wfse[64];        // FSE table of compressed Huffman weights
    int16_t norm[256];        // normalized counts
    uint16_t spr[512];        // FSE spread: symbol of each cell in spread order
    uint8_t wts[256];         // Huffman weights
    uint32_t cnt[256];        // per-symbol next-state counters
};

// ---- compressed input: coordinates x relative to the frame's 4-aligned base
struct In {
    const uint8_t *base4;   // frame start rounded down to 4 bytes
    uint32_t s0;            // frame byte 0 is coordinate s0
    uint32_t amax;          // last dword coordinate inside the frame
};

// 256 bytes (4 per lane) from the dword coordinate a into LDS at dst,
// asynchronous (global_load_lds_dword; waited by dma_wait).  Coordinates
// outside the frame are clamped onto its last dword: those bytes are never
// interpreted.
__device__ __forceinline__ void dma256(const In &I, uint32_t a, uint32_t dst)
{
    uint32_t x = a + 4 * lane_id();
    x = x > I.amax ? I.amax : x;
    __builtin_amdgcn_global_load_lds((const void *)(I.base4 + x), la<void>(uni(dst)), 4, 0, 0);
}

// s_waitcnt vmcnt(0) through the builtin, so the compiler's wait-count pass
// knows the LDS-DMA writes have landed and adds no waits of its own before
// later LDS reads (expcnt / lgkmcnt fields left at their maximum)
__device__ __forceinline__ void dma_wait()
{
    __builtin_amdgcn_s_waitcnt(0x0F70);
    wave_lds_sync();
}

// forward window: 256 bytes from frame offset p (rounded down to 4); returns
// the coordinate of win[0]
__device__ __forceinline__ uint32_t stage_win(ZLds &L, const In &I, uint32_t p)
{
    ZF_T0(t0)
    const uint32_t a = (I.s0 + p) & ~3u;
    dma256(I, a, ldsaddr(L.win));
    dma_wait();
    ZF_ADD(3, t0)
    return a;
}

__device__ __forceinline__ uint32_t wb(const ZLds &L, uint32_t wx, const In &I, uint32_t p)
{
    return *lp<uint8_t>(L.win + (I.s0 + p - wx));
}

// ---- FSE tables -----------------------------------------------------------------
// Normalized counts from the window at bit 0 of window offset wofs,
// RFC 8878 §4.1.1 / FSE_readNCount.  Returns bytes used, or 0 on error
// (*err set).  norm[] receives nsym entries; the caller zeroes norm[0..max_sym]
// first (zero counts are not written).  The bits are read through a 64-bit
// register window W = window bits [wp, wp + 64), reloaded every 32 bits.
// Wave-uniform (every lane runs it, its state in scalar registers: the scalar
// unit has issue to spare in the VALU-bound frame kernel; lane 0 stores).
__device__ __forceinline__ uint32_t read_ncount(ZLds &L, uint32_t wofs, uint32_t avail, uint32_t max_sym,
                                                uint32_t max_log, uint32_t *tlog, uint32_t *nsym, uint32_t *err)
{
    // (uniform in the compiler's eyes: else the walk is a divergent loop,
    // every branch an exec-mask save / restore)
    wofs = uni(wofs);
    avail = uni(avail);
    uint32_t pos = 8 * wofs, wp = pos + 64;   // forces the first load
    uint64_t W = 0;
    // the window's 64 dwords one per lane: a reload is two readlanes, not an
    // LDS round trip (the walk is a lone wave's serial chain)
    const uint32_t wv = *lp<uint32_t>(L.win + 4 * lane_id());
    auto bits = [&](uint32_t n) -> uint32_t {   // n <= 16 bits at pos, not consumed
        if (pos - wp >= 32) {
            wp = pos & ~31u;
            const uint32_t d = wp >> 5;
            const uint32_t lo = d < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)wv, (int)d) : 0u;
            const uint32_t hi = d + 1 < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)wv, (int)(d + 1)) : 0u;
            W = ((uint64_t)hi << 32) | lo;
        }
        return (uint32_t)(W >> (pos - wp)) & ((1u << n) - 1);
    };
    const uint32_t tl = bits(4) + 5;
    pos += 4;
    if (tl > max_log) {
        *err = ZE_CORRUPT;
        return 0;
    }
    // (threshold = 1 << (nbits - 1) throughout: derived, not carried -- one
    // loop value fewer in the frame kernel's tight scalar register budget)
    int32_t remaining = (1 << tl) + 1;
    uint32_t nbits = tl + 1, sym = 0;
    bool prev0 = false;
    while (remaining > 1 && sym <= max_sym) {
        if (prev0) {
            uint32_t n0 = sym;
            while (bits(16) == 0xFFFF) {
                n0 += 24;
                pos += 16;
            }
            while (bits(2) == 3) {
                n0 += 3;
                pos += 2;
            }
            n0 += bits(2);
            pos += 2;
            if (n0 > max_sym) {
                *err = ZE_CORRUPT;
                return 0;
            }
            sym = n0;   // the skipped counts stay 0
        }
        const int32_t threshold = 1 << (nbits - 1);
        const int32_t mx = 2 * threshold - 1 - remaining;
        const int32_t v = (int32_t)bits(nbits);
        // (both field widths as selects, no branch per symbol)
        const bool lo = (v & (threshold - 1)) < mx;
        const int32_t wide = v & (2 * threshold - 1);
        int32_t count = lo ? v & (threshold - 1) : wide >= threshold ? wide - mx : wide;
        pos += lo ? nbits - 1 : nbits;
        count--;
        remaining -= count < 0 ? -count : count;
        // (every lane, the same value: no exec-mask branch; a zero count
        // writes the zero norm_clear left)
        *lp<int16_t>(&L.norm[sym]) = (int16_t)count;
        sym++;
        prev0 = count == 0;
        // FSE_readNCount's `while (remaining < threshold) { nbBits--;
        // threshold >>= 1; }`: remaining stays >= 1 (a count never exceeds
        // it), so the field width becomes min(nbits, log2(remaining) + 1)
        nbits = min(nbits, 32u - (uint32_t)__builtin_clz((uint32_t)remaining));
    }
    // (ran off the window -- no valid description is that long -- checked
    // once here: past it the walk reads zeros, the loop ends within max_sym
    // symbols and the description is refused as before)
    const uint32_t used = (pos + 7) / 8 - wofs;
    if (pos > 8 * 256 || remaining != 1 || used > avail) {
        *err = ZE_CORRUPT;
        return 0;
    }
    *tlog = tl;
    *nsym = sym;
    return used;
}

// norm[0..n) = 0, wave-wide (before read_ncount)
__device__ __forceinline__ void norm_clear(ZLds &L, uint32_t n)
{
    for (uint32_t i = lane_id(); i < n; i += 64)
        *lp<int16_t>(&L.norm[i]) = 0;
    wave_lds_sync();
}

// Decoding table from norm[0..nsym) with accuracy log tl (FSE_buildDTable):
// cell = symbol | nbits << 8 | base << 16.  Wave-wide.  With nsym <= 64 (every
// table zstd defines: LL 36, OF 32, ML 53, Huffman weights 13 symbols) it is
// built without serial loops: the spread visits positions (j * step) & mask
// and the valid ones (<= high) take the cells in symbol order, so a prefix
// count over j gives each position its cell and a prefix max over the symbol
// starts gives each cell its symbol; next states are ranked per 64-cell group
// by ballots, with the per-symbol counters in lane registers.
__device__ __forceinline__ void fse_build(ZLds &L, uint32_t *tab, uint32_t nsym, uint32_t tl)
{
    const uint32_t lane = lane_id();
    const uint32_t size = 1u << tl, mask = size - 1;
    const uint32_t step = (size >> 1) + (size >> 3) + 3;
    const uint64_t below = (1ull << lane) - 1;
    wave_lds_sync();   // norm[] from lane 0
    if (nsym > 64) {
        if (lane == 0) {
            uint32_t high = size - 1;
            for (uint32_t s = 0; s < nsym; s++)
                if (L.norm[s] == -1)
                    *lp<uint32_t>(tab + high--) = s;
            uint32_t pos = 0;
            for (uint32_t s = 0; s < nsym; s++) {
                for (int32_t i = 0; i < L.norm[s]; i++) {
                    *lp<uint32_t>(tab + pos) = s;
                    do
                        pos = (pos + step) & mask;
                    while (pos > high);
                }
            }
        }
        for (uint32_t s = lane; s < nsym; s += 64)
            L.cnt[s] = L.norm[s] == -1 ? 1u : (uint32_t)L.norm[s];
        wave_lds_sync();
        for (uint32_t u0 = 0; u0 < size; u0 += 64) {
            const uint32_t u = u0 + lane;
            const bool act = u < size;
            const uint32_t s = act ? (*lp<uint32_t>(tab + u) & 0xFF) : 0xFFFFu;
            uint64_t rem = __ballot(act);
            while (rem) {
                const uint32_t sj = lane_val(s, __builtin_ctzll(rem));
                const uint64_t m = __ballot(act && s == sj);
                const uint32_t base = uni(L.cnt[sj]);
                if ((m >> lane) & 1) {
                    const uint32_t ns = base + (uint32_t)__builtin_popcountll(m & below);
                    const uint32_t nb = tl - (uint32_t)hibit(ns);
                    *lp<uint32_t>(tab + u) = sj | nb << 8 | ((ns << nb) - size) << 16;
                }
                if (lane == 0)
                    L.cnt[sj] = base + (uint32_t)__builtin_popcountll(m);
                wave_lds_sync();
                rem &= ~m;
            }
        }
        return;
    }
    // lane s: symbol s
    const int32_t nc = lane < nsym ? (int32_t)*lp<int16_t>(&L.norm[lane]) : 0;
    const uint32_t c = nc > 0 ? (uint32_t)nc : 0u;
    const bool low = nc == -1;
    const uint32_t K = wave_incl_add(c) - c;   // the symbol's first cell in spread order
    const uint64_t lm = __ballot(low);
    const uint32_t high = size - 1 - (uint32_t)__builtin_popcountll(lm);
    for (uint32_t u = lane; u < size; u += 64)
        *lp<uint16_t>(&L.spr[u]) = 0;
    wave_lds_sync();
    if (c)
        *lp<uint16_t>(&L.spr[K]) = (uint16_t)(lane + 1);
    wave_lds_sync();
    uint32_t carry = 0;
    for (uint32_t k0 = 0; k0 < size; k0 += 64) {
        const uint32_t k = k0 + lane;
        const uint32_t v = k < size ? (uint32_t)*lp<uint16_t>(&L.spr[k]) : 0u;
        const uint32_t pm = max(carry, wave_incl_max(v));
        if (k < size)
            *lp<uint16_t>(&L.spr[k]) = (uint16_t)(pm - 1);
        carry = lane_val(pm, 63);
    }
    wave_lds_sync();
    uint32_t kb = 0;
    for (uint32_t j0 = 0; j0 < size; j0 += 64) {
        const uint32_t j = j0 + lane, p = (j * step) & mask;
        const bool valid = j < size && p <= high;
        const uint64_t m = __ballot(valid);
        if (valid)
            *lp<uint32_t>(tab + p) = *lp<uint16_t>(&L.spr[kb + (uint32_t)__builtin_popcountll(m & below)]);
        kb += (uint32_t)__builtin_popcountll(m);
    }
    if (low)   // low-probability symbols at the top, in symbol order from size - 1 down
        *lp<uint32_t>(tab + size - 1 - (uint32_t)__builtin_popcountll(lm & below)) = lane;
    wave_lds_sync();
    // next states: lane s holds symbol s's counter; per 64-cell group each lane
    // finds the lanes holding its symbol with six bit-sliced ballots (symbols
    // < 64), ranks itself among them, and the group's per-symbol totals come
    // back through cnt[] (one ballot loop per distinct symbol cost ~5x the
    // VALU issue of the whole kernel's other table work)
    uint32_t cntr = low ? 1u : c;
    for (uint32_t u0 = 0; u0 < size; u0 += 64) {
        const uint32_t u = u0 + lane;
        const bool act = u < size;
        const uint32_t s = act ? (*lp<uint32_t>(tab + u) & 0xFF) : 0u;
        uint64_t m = __ballot(act);
#pragma unroll
        for (int bit = 0; bit < 6; bit++) {
            const bool one = (s >> bit) & 1;
            const uint64_t bb = __ballot(one);
            m &= one ? bb : ~bb;
        }
        const uint32_t base = (uint32_t)__shfl((int)cntr, (int)s, 64);
        *lp<uint32_t>(&L.cnt[lane]) = 0;
        wave_lds_sync();
        if (act) {
            const uint32_t ns = base + (uint32_t)__builtin_popcountll(m & below);
            const uint32_t nb = tl - (uint32_t)hibit(ns);
            *lp<uint32_t>(tab + u) = s | nb << 8 | ((ns << nb) - size) << 16;
            *lp<uint32_t>(&L.cnt[s]) = (uint32_t)__builtin_popcountll(m);   // equal for every lane of s
        }
        wave_lds_sync();
        cntr += *lp<uint32_t>(&L.cnt[lane]);
        wave_lds_sync();
    }
}

// ---- Huffman tables --------------------------------------------------------------
// Tree description at frame offset p (window staged at wx); returns its size
// or 0 on error.  Writes the 2^log decoding cells (nbits | symbol << 8) to
// cells (HBM); *log receives the table log.  Wave-wide.
__device__ __forceinline__ uint32_t huf_read(ZLds &L, const In &I, uint32_t wx, uint32_t p, uint32_t avail,
                                             uint32_t *log, uint16_t *cells)
{
    const uint32_t lane = lane_id();
    const uint32_t hb = uni(wb(L, wx, I, p));
    const uint32_t wofs = uni(I.s0 + p - wx + 1);   // window offset of the description body (uniform: see read_ncount)
    uint32_t nw = 0, used = 0, err = 0;
    if (hb < 128) {
        if (1 + hb > avail || wofs + hb > 256)
            return 0;
        uint32_t tl = 0, nsym = 0;
        uint32_t hs = 0;
        ZF_T0(tq0)
        norm_clear(L, 256);
        hs = read_ncount(L, wofs, hb, 255, 6, &tl, &nsym, &err);
        ZF_ADD(5, tq0)
        hs = uni(hs);
        if (uni(err))
            return 0;
        tl = uni(tl);
        nsym = uni(nsym);
        ZF_T0(tq1)
        fse_build(L, L.wfse, nsym, tl);
        ZF_ADD(6, tq1)
        ZF_T0(tq2)
        {
            // backward stream inside the window: two interleaved states
            // (wave-uniform, as read_ncount; lane 0 stores the weights)
            const uint32_t b0 = wofs + hs, bn = hb - hs;
            const uint32_t lastb = bn ? uni(*lp<uint8_t>(L.win + b0 + bn - 1)) : 0;
            // the window's dwords and the weights' FSE cells (<= 64) one per
            // lane: the walk reads them by readlane, not LDS round trips
            const uint32_t wv = *lp<uint32_t>(L.win + 4 * lane);
            const uint32_t fv = *lp<uint32_t>(L.wfse + (lane < (1u << tl) ? lane : 0u));
            auto w32 = [&](uint32_t bit) -> uint32_t {   // win32 from the registers
                const uint32_t d = bit >> 5;
                const uint32_t lo = d < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)wv, (int)d) : 0u;
                const uint32_t hi = d + 1 < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)wv, (int)(d + 1)) : 0u;
                return (uint32_t)((((uint64_t)hi << 32) | lo) >> (bit & 31));
            };
            auto cellw = [&](uint32_t st) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)fv, (int)st); };
            if (!lastb) {
                err = 1;
            } else {
                int32_t pos = (int32_t)(8 * (bn - 1)) + hibit(lastb);
                // n backward bits ending at pos (bits below the stream read as 0)
                auto rb = [&](uint32_t n) -> uint32_t {
                    pos -= (int32_t)n;
                    const int32_t x = (int32_t)(8 * b0) + pos;
                    uint32_t v = (x >= 0 ? w32((uint32_t)x) : w32(0) << (uint32_t)(-x)) & ((1u << n) - 1);
                    if (pos < 0)
                        v = -pos >= (int32_t)n ? 0u : v & (~0u << (uint32_t)(-pos));
                    return v;
                };
                auto put = [&](uint32_t c) {
                    if (lane == 0)
                        L.wts[nw] = (uint8_t)c;
                    nw++;
                };
                uint32_t s1 = rb(tl), s2 = rb(tl);
                for (;;) {
                    if (nw > 253) {
                        err = 1;
                        break;
                    }
                    uint32_t c = cellw(s1);
                    put(c);
                    s1 = (c >> 16) + rb((c >> 8) & 0xFF);
                    if (pos < 0) {
                        put(cellw(s2));
                        break;
                    }
                    if (nw > 253) {
                        err = 1;
                        break;
                    }
                    c = cellw(s2);
                    put(c);
                    s2 = (c >> 16) + rb((c >> 8) & 0xFF);
                    if (pos < 0) {
                        put(cellw(s1));
                        break;
                    }
                }
            }
        }
        wave_lds_sync();   // lane 0's weights before every lane reads them
        ZF_ADD(7, tq2)
        used = 1 + hb;
    } else {
        nw = hb - 127;
        const uint32_t bytes = (nw + 1) / 2;
        if (1 + bytes > avail || wofs + bytes > 256)
            return 0;
        for (uint32_t i = lane; i < nw; i += 64) {
            const uint32_t by = *lp<uint8_t>(L.win + wofs + i / 2);
            L.wts[i] = (uint8_t)((i & 1) ? (by & 15) : (by >> 4));
        }
        used = 1 + bytes;
    }
    if (uni(err))
        return 0;
    nw = uni(nw);
    // weights -> table log, implied last weight, canonical cell ranges
    uint32_t total = 0, bad = 0, r1 = 0;
    for (uint32_t i = lane; i < nw; i += 64) {
        const uint32_t w = L.wts[i];
        bad |= w >= 12;
        total += (1u << w) >> 1;
        r1 += w == 1;
    }
    // wave sums (few values; DPP-free reduction through readlane is enough here)
    for (int k = 32; k >= 1; k >>= 1) {
        total += __shfl_xor(total, k, 64);
        r1 += __shfl_xor(r1, k, 64);
        bad |= __shfl_xor(bad, k, 64);
    }
    total = uni(total);
    r1 = uni(r1);
    if (uni(bad) || total == 0)
        return 0;
    const uint32_t lg = (uint32_t)hibit(total) + 1;
    if (lg > 12)
        return 0;
    const uint32_t rest = (1u << lg) - total;
    if (rest != (1u << hibit(rest)))
        return 0;
    const uint32_t lastw = (uint32_t)hibit(rest) + 1;
    if (lane == 0)
        L.wts[nw] = (uint8_t)lastw;
    wave_lds_sync();
    r1 += lastw == 1;
    if (r1 < 2 || (r1 & 1))
        return 0;
    nw++;
    // canonical cells, straight into the block's slot: class k (weight k,
    // 2^(k-1) cells per symbol) follows the lower classes, its symbols in
    // symbol order
    uint32_t wl[4];
#pragma unroll
    for (int ps = 0; ps < 4; ps++) {
        const uint32_t s = 64 * ps + lane;
        wl[ps] = s < nw ? (uint32_t)*lp<uint8_t>(&L.wts[s]) : 0u;
    }
    const uint64_t below = (1ull << lane) - 1;
    uint32_t c0 = 0;
    for (uint32_t k = 1; k <= lg; k++) {
        uint32_t n = 0;
#pragma unroll
        for (int ps = 0; ps < 4; ps++) {
            const uint64_t m = __ballot(wl[ps] == k);
            if (wl[ps] == k)
                *lp<int16_t>(&L.norm[n + (uint32_t)__builtin_popcountll(m & below)]) = (int16_t)(64 * ps + lane);
            n += (uint32_t)__builtin_popcountll(m);
        }
        if (!n)
            continue;
        wave_lds_sync();
        const uint32_t sh = k - 1, ck = n << sh, nb = lg + 1 - k;
        for (uint32_t u = lane; u < ck; u += 64)
            cells[c0 + u] = (uint16_t)((uint32_t)*lp<int16_t>(&L.norm[u >> sh]) << 8 | nb);
        c0 += ck;
        wave_lds_sync();   // before the list is rewritten
    }
    *log = lg;
    return used;
}

}   // namespace
}   // namespace zsk
