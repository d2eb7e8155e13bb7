// zstd_huf_seq.hip -- the kernels that run side by side behind the frame
// kernel: Huffman literal streams (zstd_huf_dev.h) and the sequence replay
// (zstd_seq_dev.h), with the one-frame route's fused kernel and the literal
// fix-up that joins them.  One file for both stages: x2_rescue is kept out of
// line and compiled to fit the callers it sees -- zstd_huf_kernel,
// zstd_huf_one_kernel and zstd_one_kernel; in two files each got its own,
// differently compiled copy.
#include <stdio.h>
#include <stdlib.h>

#ifdef ZSK_TUNING
// ZSEEK_ZSTD_HUF_DIAG: zstd_huf_kernel's waves per lgmax, LDS / global path
namespace zsk { namespace { __device__ unsigned int g_hdiag[32]; } }
// ZSEEK_SEQ_TIMERS, the one-frame replay: [0] kernel cycles, [1] sequence-loop
// cycles, [2] sequences, [3] kernel real-time ticks (100 MHz), [4] frames, [5]
// cycles of the chain alone
namespace zsk { namespace { __device__ unsigned long long g_sdiag[8]; } }
#endif
#include "zstd_huf_dev.h"
#include "zstd_internal.h"
#include "zstd_seq_dev.h"

namespace zsk {
namespace {

using namespace lz4d;

// B: steps per store burst (4 = 64 bytes)
template <int DIAG, int B = 4>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void zstd_huf_kernel(
    const uint8_t *__restrict__ jobs, uint32_t nj, const uint8_t *__restrict__ comp,
    const uint8_t *__restrict__ slots, uint8_t *__restrict__ lit, uint8_t *__restrict__ hbad,
    const uint64_t *__restrict__ jr)
{
    __shared__ __attribute__((aligned(16))) uint16_t tabs[kHufLdsCells];
    __shared__ __attribute__((aligned(16))) uint8_t rings[kRS * 1024];
    const uint32_t lane = threadIdx.x;
    if (jr) {
        // the asynchronous decode: the grid covers the call's block capacity,
        // jobs / hbad are the arrays' starts and the chunk's blocks are
        // [jr[0], jr[1]) in device memory; a surplus workgroup leaves here
        const uint64_t b0 = jr[0];
        nj = (uint32_t)(4 * (jr[1] - b0));
        if (blockIdx.x * 64 >= nj)
            return;
        jobs += 4 * b0 * sizeof(HufJob);
        hbad += 4 * b0;
    }
    const uint32_t j = blockIdx.x * 64 + lane;
    HufJob J = {0, 0, 0, 0, 0, 0};
    if (j < nj)
        J = reinterpret_cast<const HufJob *>(jobs)[j];
    const bool act = J.len != 0;
    const uint32_t jlg = J.tab >> 28, jslot = J.tab & kHufSlotMask, jx2 = (J.tab >> 27) & 1;
    const uint32_t lgmax = lane_val(wave_incl_max(act ? jlg : 0u), 63);
    // cells of each block's table (stream 0's lane), packed in block order
    const uint32_t cells = (lane & 3) == 0 && act ? ((1u << jlg) < 8 ? 8u : 1u << jlg) : 0u;
    const uint32_t incl = wave_incl_add(cells);
    const uint32_t first = (uint32_t)__shfl((int)(incl - cells), (int)(lane & ~3u), 64);
    const bool in_lds = lane_val(incl, 63) <= kHufLdsCells;
    // the longest streams (a literal-only 64 KiB block: 16 Ki symbols each,
    // ~2.5x the usual) bound the kernel: their waves issue first
    if (lane_val(wave_incl_max(act ? J.cnt : 0u), 63) > 12000)
        __builtin_amdgcn_s_setprio(3);
    if (in_lds) {
        for (uint32_t b = 0; b < 16; b++) {
            const uint32_t nc = lane_val(cells, 4 * b);
            if (!nc)
                continue;
            const uint32_t c0 = lane_val(incl, 4 * b) - nc;
            const uint8_t *src = slots + (uint64_t)lane_val(jslot, 4 * b) * kZSlot;
            for (uint32_t c = lane; c < nc / 8; c += 64)
                *lp<u32x4>(&tabs[c0 + 8 * c]) = *reinterpret_cast<const u32x4 *>(src + 16 * c);
        }
        __syncthreads();
    }
    // one resource over the wave's streams (else lane by lane, each its own)
    const uint64_t lo = uni64(wave_min64(act ? J.src : ~0ull)) & ~15ull;
    const uint64_t hi = uni64(wave_max64(act ? J.src + J.len : 0ull));
#ifdef ZSK_TUNING
    if (DIAG && lane == 0) {
        atomicAdd(&g_hdiag[lgmax & 15], 1u);
        atomicAdd(&g_hdiag[16 + (in_lds ? 1 : 0)], 1u);
    }
#endif
    if (j >= nj)
        return;
    bool bad = false;
    auto run = [&](__amdgpu_buffer_rsrc_t r, uint64_t base) {
        BRd b;
        bad = !br_init(b, r, (uint32_t)(J.src - base), J.len, (uint32_t)(uintptr_t)lp<uint8_t>(rings) + 4 * lane,
                       in_lds && lgmax <= 8);   // huf_stream<4, 1>: two chunks in flight
        uint8_t *out = lit + J.dst;
        if (in_lds) {
            const uint32_t tb = (uint32_t)(uintptr_t)lp<uint16_t>(&tabs[first]);
            auto T = [&](uint32_t i) -> uint32_t { return *la<uint16_t>(tb + 2 * i); };
            if (lgmax <= 8)
                huf_stream<4, 1, DIAG, B>(b, T, jlg, out, J.dst, J.cnt, J.lim);
            else
                huf_stream<2, 2, DIAG, B>(b, T, jlg, out, J.dst, J.cnt, J.lim);
        } else {
            const uint16_t *gt = reinterpret_cast<const uint16_t *>(slots + (uint64_t)jslot * kZSlot);
            auto T = [&](uint32_t i) -> uint32_t { return gt[i]; };
            huf_stream<2, 2, DIAG, B>(b, T, jlg, out, J.dst, J.cnt, J.lim);
        }
        bad = bad || br_left(b) != 0;
    };
    if (hi > lo && hi - lo < kMaxSpan) {
        if (act)
            run(span_rsrc(comp, lo, hi - lo), lo);
    } else {
        for (uint64_t m = __ballot(act); m; m &= m - 1) {
            const int l = __builtin_ctzll(m);
            const uint64_t s0 = uni64(__shfl(J.src, l, 64)) & ~15ull;
            const uint64_t s1 = uni64(__shfl(J.src + J.len, l, 64));
            if ((int)lane == l)
                run(span_rsrc(comp, s0, s1 - s0), s0);
        }
    }
    if (bad && jx2) {   // libzstd's X2 decoder may still accept the stream
        const uint16_t *tp =
            in_lds ? &tabs[first] : reinterpret_cast<const uint16_t *>(slots + (uint64_t)jslot * kZSlot);
        const uint64_t s0 = J.src & ~15ull;
        const uint32_t x = x2_rescue(span_rsrc(comp, s0, J.src + J.len - s0), (uint32_t)(J.src - s0), J.len, J.cnt,
                                     tp, jlg);
        bad = !(x & 1);
        if ((x & 0x10000) && J.cnt - 1 < J.lim)
            lit[J.dst + J.cnt - 1] = (uint8_t)(x >> 8);
    }
    hbad[j] = bad ? 1 : 0;
}

__global__ __launch_bounds__(kHufOneT) void zstd_huf_one_kernel(
    const uint8_t *__restrict__ jobs, const uint8_t *__restrict__ comp, const uint8_t *__restrict__ slots,
    uint8_t *__restrict__ lit, uint8_t *__restrict__ hbad, const uint64_t *__restrict__ jr)
{
    __shared__ HufOneLds H;
    if (jr) {   // (the asynchronous decode, as in zstd_huf_kernel)
        const uint64_t b0 = jr[0];
        if (blockIdx.x >= 4 * (jr[1] - b0))
            return;
        jobs += 4 * b0 * sizeof(HufJob);
        hbad += 4 * b0;
    }
    huf_one_body(H, blockIdx.x, threadIdx.x, jobs, comp, slots, lit, hbad);
}

template <uint32_t LANES, uint32_t CELLS, uint32_t GM = 0, bool ONE = false>
__global__ __launch_bounds__(64) void zstd_seq_kernel(
    const FrameDesc *__restrict__ desc, uint32_t n, const uint8_t *__restrict__ comp,
    uint8_t *__restrict__ ops, const uint64_t *__restrict__ blk_base,
    const uint8_t *__restrict__ slots, uint32_t *__restrict__ stop,
    const uint64_t *__restrict__ rec_base, uint64_t *__restrict__ items, uint32_t *__restrict__ nitems,
    int32_t *__restrict__ status, uint64_t *__restrict__ ck, uint32_t *__restrict__ fail_at, uint32_t f0,
    const uint64_t *__restrict__ fit)
{
    __shared__ SeqLds<LANES, CELLS, ONE> SH;
    if (fit && *fit)   // (the asynchronous decode: the batch did not fit its bounds)
        return;
    seq_body<LANES, CELLS, GM, ONE>(SH, blockIdx.x, desc, n, comp, ops, blk_base, slots, stop, rec_base, items,
                                    nitems, status, ck, fail_at, f0);
}

// The one-frame route's replay and Huffman streams in one launch: workgroups
// [0, m) replay frame f0 + b on their first wave (the others leave), the rest
// decode Huffman job b - m with all kHufOneT threads -- no second stream, so
// no event between the frame kernel and them or between them and the
// literal fix-up (~8-11 us each on the request's timeline).  LDS: the union.
// The workgroup finishing last (a counter in `done`, zero between launches:
// the last one resets it) runs the literal fix-up (zstd_lit_fix_kernel's
// work) -- every replay and Huffman job is done by then; nothing waits.
__global__ __launch_bounds__(kHufOneT) void zstd_one_kernel(
    const FrameDesc *__restrict__ desc, uint32_t n, const uint8_t *__restrict__ comp,
    uint8_t *__restrict__ ops, const uint64_t *__restrict__ blk_base,
    const uint8_t *__restrict__ slots, uint32_t *__restrict__ stop,
    const uint64_t *__restrict__ rec_base, uint64_t *__restrict__ items, uint32_t *__restrict__ nitems,
    int32_t *__restrict__ status, uint64_t *__restrict__ ck, uint32_t *__restrict__ fail_at, uint32_t f0,
    uint32_t m, const uint8_t *__restrict__ jobs, uint8_t *__restrict__ lit, uint8_t *__restrict__ hbad,
    uint32_t *__restrict__ done, const uint64_t *__restrict__ fit, const uint64_t *__restrict__ jr)
{
    __shared__ union {
        SeqLds<1, 0, true> s;
        HufOneLds h;
    } U;
    __shared__ uint32_t last;
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    // the workgroups that take part (and count in `done`): the whole grid, or
    // for the asynchronous decode, whose grid covers the call's block
    // capacity, the m replays and the chunk's jobs (blocks [jr[0], jr[1]) in
    // device memory; none at all when the batch did not fit its bounds)
    uint32_t parts = gridDim.x;
    if (jr) {
        if (*fit)
            return;
        const uint64_t b0 = jr[0];
        parts = m + (uint32_t)(4 * (jr[1] - b0));
        if (b >= parts)
            return;
        jobs += 4 * b0 * sizeof(HufJob);
        hbad += 4 * b0;
    }
    if (b < m) {
        // waves 0 and 1: the replay's chain and its vector phase.  Waves 2
        // and 3 leave before any barrier: a wave that has ended no longer
        // counts at s_barrier (CDNA), so seq_body's data-dependent barriers
        // and the two below are met by waves 0 and 1 alone, and no wave
        // reads `last` before thread 0 has written it.
        if (t >= 128)
            return;
        seq_body<1, 0, 0, true, true>(U.s, b, desc, n, comp, ops, blk_base, slots, stop, rec_base, items, nitems,
                                      status, ck, fail_at, f0);
    } else {
        huf_one_body(U.h, b - m, t, jobs, comp, slots, lit, hbad);
    }
    // (thread 0 wrote what the fix-up reads: status, items, stop, hbad)
    __syncthreads();
    if (t == 0) {
        __threadfence();
        last = atomicAdd(done, 1u) == parts - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!last)
        return;
    __threadfence();
    if (t < 64)
        for (uint32_t f = f0 + t; f < n; f += 64)
            lit_fix(f, ops, blk_base, hbad, stop, status, nitems, fail_at);
    if (t == 0)
        *done = 0;
}

__global__ __launch_bounds__(256) void zstd_lit_fix_kernel(
    uint32_t n, const uint8_t *__restrict__ ops, const uint64_t *__restrict__ blk_base,
    const uint8_t *__restrict__ hbad, const uint32_t *__restrict__ stop, int32_t *__restrict__ status,
    uint32_t *__restrict__ nitems, uint32_t *__restrict__ fail_at, uint32_t f0, const uint64_t *__restrict__ fit)
{
    const uint32_t f = f0 + blockIdx.x * 256 + threadIdx.x;   // frames [f0, n)
    if (fit && *fit)   // (the asynchronous decode: the batch did not fit its bounds)
        return;
    if (f < n)
        lit_fix(f, ops, blk_base, hbad, stop, status, nitems, fail_at);
}

}   // namespace

// ZSEEK_SEQ_TIMERS (tuning builds): the one-frame replay's cycles, every 100th launch
void zstd_seq_timers(hipStream_t stream)
{
#ifdef ZSK_TUNING
    static const bool timers = getenv("ZSEEK_SEQ_TIMERS") != nullptr;
    static int calls = 0;
    if (!timers || ++calls % 100 != 0)
        return;
    unsigned long long z[8] = {0};
    (void)hipMemcpyFromSymbolAsync(z, HIP_SYMBOL(g_sdiag), sizeof(z), 0, hipMemcpyDeviceToHost, stream);
    (void)hipStreamSynchronize(stream);
    const double fr = z[4] ? (double)z[4] : 1.0, sq = z[2] ? (double)z[2] : 1.0;
    fprintf(stderr,
            "one-frame sequences: kernel %.0f cycles (%.1f us, %.0f MHz) per frame, loop %.0f cycles "
            "(%.0f per sequence, chain alone %.0f, %.0f sequences per frame)\n",
            z[0] / fr, z[3] / fr / 100.0, z[3] ? z[0] * 100.0 / z[3] : 0.0, z[1] / fr, z[1] / sq, z[5] / sq, sq / fr);
#endif
}

void launch_zstd_huf(const ZstdCall &C, ZstdScratch *s, const ZstdChunk &c, bool one, hipStream_t stream)
{
    // (c.dev: b0 = 0 and b1 the block capacity, so jb / hb are the arrays'
    // starts and nj sizes the grid; the kernels take the true range from c.dev)
    const uint32_t nj = (uint32_t)(4 * (c.b1 - c.b0));
    const uint8_t *jb = s->hjobs + 4 * c.b0 * sizeof(HufJob);
    uint8_t *hb = s->hbad + 4 * c.b0;
    const auto go_one = [&] {
        hipLaunchKernelGGL(zstd_huf_one_kernel, dim3(nj), dim3(kHufOneT), 0, stream, jb, C.comp, s->slots, s->lit, hb,
                           c.dev);
    };
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((nj + 63) / 64), dim3(64), 0, stream, jb, nj, C.comp, s->slots, s->lit, hb,
                           c.dev);
    };
#ifdef ZSK_TUNING
    // diagnostics (tuning builds, ZSEEK_ZSTD_HUF_DIAG): 1 / 3 / 7 / 8
    // counters and elisions (printed)
    static const int diag = getenv("ZSEEK_ZSTD_HUF_DIAG") ? atoi(getenv("ZSEEK_ZSTD_HUF_DIAG")) : 0;
    if (diag) {
        unsigned int z[32] = {};
        (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_hdiag), z, sizeof(z), 0, hipMemcpyHostToDevice, stream);
    }
    switch (one ? -1 : diag) {
    case -1: go_one(); break;
    case 0: go(zstd_huf_kernel<0>); break;
    case 1: go(zstd_huf_kernel<1>); break;
    case 3: go(zstd_huf_kernel<3>); break;
    case 7: go(zstd_huf_kernel<7>); break;
    default: go(zstd_huf_kernel<8>); break;
    }
    if (diag) {
        unsigned int z[32] = {};
        (void)hipMemcpyFromSymbolAsync(z, HIP_SYMBOL(g_hdiag), sizeof(z), 0, hipMemcpyDeviceToHost, stream);
        (void)hipStreamSynchronize(stream);
        fprintf(stderr, "huf diag %d (chunk %u): lgmax", diag, c.c);
        for (int i = 0; i < 16; i++)
            if (z[i])
                fprintf(stderr, " %d:%u", i, z[i]);
        fprintf(stderr, "  global %u lds %u\n", z[16], z[17]);
    }
#else
    if (one)
        go_one();
    else
        go(zstd_huf_kernel<0>);
#endif
}

void launch_zstd_seq(const ZstdCall &C, ZstdScratch *s, const ZstdChunk &c, bool one, hipStream_t stream)
{
    const uint32_t m = c.f1 - c.f0;
    const auto go = [&](auto kernel, uint32_t groups) {
        hipLaunchKernelGGL(kernel, dim3(groups), dim3(64), 0, stream, C.desc, c.f1, C.comp, s->ops, s->blk_base,
                           s->slots, s->stop, s->rec_base, s->items, s->nitems, C.status, s->ck, C.fail_at, c.f0,
                           C.fit);
    };
    if (one) {
        go(zstd_seq_kernel<1, 0, 0, true>, m);
        zstd_seq_timers(stream);
    } else {
        go(zstd_seq_kernel<kSeqLanes, kSeqCells, kSeqGm>, (m + kSeqLanes - 1) / kSeqLanes);
    }
}

void launch_zstd_one(const ZstdCall &C, ZstdScratch *s, const ZstdChunk &c, hipStream_t stream)
{
    const uint32_t m = c.f1 - c.f0, nj = (uint32_t)(4 * (c.b1 - c.b0));
    hipLaunchKernelGGL(zstd_one_kernel, dim3(m + nj), dim3(kHufOneT), 0, stream, C.desc, c.f1, C.comp, s->ops,
                       s->blk_base, s->slots, s->stop, s->rec_base, s->items, s->nitems, C.status, s->ck, C.fail_at,
                       c.f0, m, s->hjobs + 4 * c.b0 * sizeof(HufJob), s->lit, s->hbad + 4 * c.b0,
                       reinterpret_cast<uint32_t *>(s->d_total + ZstdScratch::kDoneWord), C.fit, c.dev);
}

void launch_zstd_lit_fix(const ZstdCall &C, ZstdScratch *s, const ZstdChunk &c, hipStream_t stream)
{
    hipLaunchKernelGGL(zstd_lit_fix_kernel, dim3((c.f1 - c.f0 + 255) / 256), dim3(256), 0, stream, c.f1, s->ops,
                       s->blk_base, s->hbad, s->stop, C.status, s->nitems, C.fail_at, c.f0, C.fit);
}

}   // namespace zsk
