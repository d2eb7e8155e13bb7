// lz4_route.h — which kernels an LZ4 batch gets, as a pure function.
//
// lz4_plan(request, switches) -> the launch sequence launch_lz4_split
// (lz4_split.hip) walks, and what parse_kernel_name / lz4_kernel_name /
// lz4_pick_engine report.  Plain C++17, no HIP: the product and
// tests/native/lz4_route_shim.cpp compile the same text, and
// tests/test_lz4_route.py holds it to a kernel trace recorded from the library
// (tests/golden/lz4_route_trace.json) and to DESIGN.md §3's table.
#ifndef ZSK_LZ4_ROUTE_H
#define ZSK_LZ4_ROUTE_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace zsk {

// Production decoders a batch can be forced through (tests; ROUTE_AUTO is the
// library's own choice).  LEAN / SCAN / CHUNK: the two-phase decoder with that
// parse for every frame.
// BLOCK: every multi-block-capable frame through the block route below (any
// batch size, no job minimum).
// ONE: the one-frame route (batches of <= kOneMaxFrames frames under AUTO):
// every frame takes the chunk parse, reading the frame staged whole in LDS
// (one frame per workgroup); no plan scan, no lean / scan launches.
enum : int { ROUTE_AUTO = 0, ROUTE_WAVE = 1, ROUTE_LEAN = 2, ROUTE_SCAN = 3, ROUTE_CHUNK = 4, ROUTE_BLOCK = 5,
             ROUTE_ONE = 6 };
// Decoder selection (env ZSEEK_HIP_KERNEL = split | wave; default auto).
enum : int { ENGINE_AUTO = 0, ENGINE_SPLIT, ENGINE_WAVE };

// ---- thresholds ----------------------------------------------------------------
constexpr uint32_t kNoSize = 0xFFFFFFFFu;       // a compressed-size bound no frame reaches
constexpr uint32_t kOneMaxFrames = 64;          // the one-frame route's largest batch (AUTO)
constexpr uint32_t kFrameExecMax = 65536;       // decoded bytes a workgroup executes staged whole in LDS
// Frames of at least chunk_parse_min(nframes) compressed bytes go to the
// chunk parse: with >= 32768 frames the lane-per-frame scan has a lane for
// every frame it needs and wins on 64 KiB frames (2.07 vs 4.18 ms parse at
// config 2); smaller batches and bigger frames leave its lanes idle
// (1 MiB frames: 4,096 chains; 256 MiB batches: 4,096 frames).
constexpr uint32_t kLaneBatchMin = 32768;       // frames from which every lane of the lean parse has work
constexpr uint32_t kChunkMinLaneBatch = 49152;  // chunk parse from this many compressed bytes, such batches
constexpr uint32_t kChunkMinSmallBatch = 8192;  // ... and smaller batches
// Frames under this many compressed bytes take the older lz4_scan_kernel
// (its direct item stores beat the lean kernel's line flush on short frames:
// 4 KiB frames 5.68 vs 6.71 ms per launch, config 3)
constexpr uint32_t kLeanMinCsize = 12288;
constexpr uint32_t kBlockRouteMinFrames = 1024;   // the block route under AUTO: batches of [this, kLaneBatchMin)
constexpr uint32_t kBlockRouteMinJobs = 16384;    // ... used on the device from this many planned jobs
constexpr uint32_t kMaxBlockJobs = 64;            // blocks per frame the route takes
constexpr uint32_t kJobsCapMax = 1u << 21;        // job lanes of a batch, at most
constexpr uint32_t kOriginJobsMax = 1024;         // jobs the block-parallel execute's scratch holds (136 KiB each)
constexpr uint32_t kPlanGroups = 256;             // plan workgroups, at most (256 frames each, then strided)

// ---- switches ------------------------------------------------------------------
// The environment's routing switches (A/B runs), read once per process
// (lz4_switches(), lz4_split.hip).
enum : int { PARSE_AUTO = 0, PARSE_SCAN = 1, PARSE_CHUNK = 2 };
struct Lz4Switches {
    int engine = ENGINE_AUTO;      // ZSEEK_HIP_KERNEL=split|wave: wave forces the wave kernel for every frame
    int parse = PARSE_AUTO;        // ZSEEK_PARSE (AUTO batches): chunk = the chunk parse for every frame;
                                   // scan = no chunk parse (lean from kLeanMinCsize, scan below)
    bool block_off = false;        // ZSEEK_BLOCK_ROUTE=0: no automatic block route
    bool one_off = false;          // ZSEEK_ONE_ROUTE=0, or ZSEEK_PARSE set to anything: no automatic one-frame route
    bool one_big_off = false;      // ZSEEK_ONE_BIG=0: the one-frame route's frames of > 64 KiB as round 5
    bool one_blocks_off = false;   // ZSEEK_ONE_BLOCKS=0: ... all through the windowed execute
    bool one_exec_wave = false;    // ZSEEK_ONE_EXEC=wave: the one-frame route executes with the wave kernel
};

// From the seven variables' values (null: unset).
inline Lz4Switches lz4_switches_of(const char *hip_kernel, const char *parse, const char *block_route,
                                   const char *one_route, const char *one_big, const char *one_blocks,
                                   const char *one_exec)
{
    const auto is = [](const char *v, const char *want) { return v && !strcmp(v, want); };
    Lz4Switches w;
    w.engine = is(hip_kernel, "split") ? ENGINE_SPLIT : is(hip_kernel, "wave") ? ENGINE_WAVE : ENGINE_AUTO;
    w.parse = is(parse, "scan") ? PARSE_SCAN : is(parse, "chunk") ? PARSE_CHUNK : PARSE_AUTO;
    w.block_off = is(block_route, "0");
    w.one_off = is(one_route, "0") || parse != nullptr;
    w.one_big_off = is(one_big, "0");
    w.one_blocks_off = is(one_blocks, "0");
    w.one_exec_wave = is(one_exec, "wave");
    return w;
}

inline Lz4Switches lz4_switches_env()
{
    return lz4_switches_of(getenv("ZSEEK_HIP_KERNEL"), getenv("ZSEEK_PARSE"), getenv("ZSEEK_BLOCK_ROUTE"),
                           getenv("ZSEEK_ONE_ROUTE"), getenv("ZSEEK_ONE_BIG"), getenv("ZSEEK_ONE_BLOCKS"),
                           getenv("ZSEEK_ONE_EXEC"));
}

// ---- the routes ----------------------------------------------------------------
inline uint32_t chunk_parse_min(uint32_t nframes, const Lz4Switches &w)
{
    if (w.parse == PARSE_SCAN)
        return kNoSize;
    if (w.parse == PARSE_CHUNK)
        return 0;
    return nframes >= kLaneBatchMin ? kChunkMinLaneBatch : kChunkMinSmallBatch;
}

// Parse routing of the two-phase decoder: frames of >= chunk_min compressed
// bytes take lz4_chunk_kernel, of [lean_min, chunk_min) lz4_lean_pair_kernel,
// shorter ones lz4_scan_kernel.  (ROUTE_WAVE reaches the two-phase decoder in
// tuning builds only, and is routed like AUTO.)
struct ParseRoute {
    uint32_t chunk_min, lean_min;
};
inline ParseRoute parse_route(uint32_t nframes, int route, const Lz4Switches &w)
{
    switch (route) {
    case ROUTE_LEAN: return {kNoSize, 0};
    case ROUTE_SCAN: return {kNoSize, kNoSize};
    case ROUTE_CHUNK:
    case ROUTE_BLOCK:
    case ROUTE_ONE: return {0, 0};
    default: break;
    }
    const uint32_t cmin = chunk_parse_min(nframes, w);
    return {cmin, cmin < kLeanMinCsize ? cmin : kLeanMinCsize};
}

// The block route for a batch: on (AUTO) for >= 1024 frames and < 32768 --
// the batches whose big frames take the chunk parse (config 3: 4,096 frames
// of 1 MiB, 16 blocks each) -- with frames of >= chunk_min compressed bytes,
// used on the device only when >= 16,384 jobs were planned (fewer leave the
// lean parse's lanes idle and the chunk parse wins); ROUTE_BLOCK forces it
// for every frame and any job count.  max_bsid: the largest block size id
// the block plan gives jobs to.
struct BlockRoute {
    bool on;
    uint32_t min_csize, min_jobs, max_bsid;
};
inline BlockRoute block_route(uint32_t nframes, int route, const ParseRoute &r, const Lz4Switches &w)
{
    if (route == ROUTE_BLOCK)
        return {true, 0, 1, 7};
    if (w.block_off || route != ROUTE_AUTO || nframes < kBlockRouteMinFrames || nframes >= kLaneBatchMin ||
        r.chunk_min == kNoSize)
        return {false, 0, 0, 7};
    return {true, r.chunk_min, kBlockRouteMinJobs, 7};
}

// The one-frame route: batches of a few frames -- a cached
// reader's single-frame miss, a request's first batch -- where one frame's
// serial chain is the whole launch: each frame's chunk parse reads it staged
// in LDS, one frame per workgroup.
inline bool one_route(uint32_t nframes, int route, const Lz4Switches &w)
{
    return route == ROUTE_ONE || (route == ROUTE_AUTO && !w.one_off && nframes <= kOneMaxFrames);
}

// ---- request and plan ----------------------------------------------------------
// What a caller of launch_lz4_split knows about its batch.
struct Lz4Request {
    uint32_t nframes = 0;
    int route = ROUTE_AUTO;
    int stages = 15;                  // bitmask 1 plan, 2 parse, 4 execute, 8 hand-offs (tuning builds time subsets)
    int tune = 0;                     // tuning builds: bits 0-7 the lean parse's diag, bits 8-19 the execute's version
    uint32_t stop_last = 0xFFFFFFFFu; // the batch's last frame is executed only this far
    uint32_t max_dsize = 0xFFFFFFFFu; // the batch's largest decoded frame, when the caller knows it
    bool in_order = false;            // the caller laid the frames out in order in d_comp
    bool scan_layout = false;         // item slots by the plan's scan whatever the frames' order (not with in_order)
    bool dsize_bound = false;         // max_dsize is a bound of the frames' sizes, not the largest one's
    bool post = false;                // a HostPost was offered (a lone frame's results straight to the host)
    // a re-plan after a failed reservation: no block route scratch / no
    // scratch for the block-parallel execute's origins
    bool block_denied = false, origin_denied = false;
};

enum : int { LZ4_WAVE_ENGINE = 0, LZ4_ONE = 1, LZ4_TWO_PHASE = 2 };
enum : int { BLOCK_PLAN_NONE = 0, BLOCK_PLAN_INSIDE = 1, BLOCK_PLAN_SEPARATE = 2 };

struct Lz4Plan {
    // LZ4_WAVE_ENGINE: launch_lz4_wave over every frame and nothing else -- the
    // callers in front of launch_lz4_split ask (lz4_pick_engine) and never
    // come; the steps below are then what a tuning build that comes anyway
    // gets (the two-phase decoder, ROUTE_WAVE routed like AUTO)
    int klass = LZ4_TWO_PHASE;
    ParseRoute parse{0, 0};
    BlockRoute block{false, 0, 0, 7};
    uint32_t jlanes = 0;        // job lanes: the block plan's job slots, the job kernels' grids
    uint32_t origin_jobs = 0;   // jobs of origin scratch to reserve (0: none)
    // plan stage
    bool plan = false;          // lz4_plan_direct_kernel on plan_groups workgroups
    uint32_t plan_groups = 0;
    int block_plan = BLOCK_PLAN_NONE;   // inside the plan's one workgroup, or lz4_block_plan_kernel behind it
    bool scan_layout = false;
    // parse stage, in launch order
    bool job_parse = false;     // a workgroup per block job (the one-frame route's big frames)
    bool lean_blocks = false;   // a lane per block job (the block route)
    bool lean = false;          // frames of [lean_min, lean_max) compressed bytes, diag lean_diag
    uint32_t lean_min = 0, lean_max = 0;
    int lean_diag = 0;
    bool scan = false;          // frames under scan_max
    uint32_t scan_max = 0;
    bool chunk = false;         // frames of >= parse.chunk_min; chunk_one: a frame per workgroup
    bool chunk_one = false;
    bool chunk_solo = false;    // no plan launch: the chunk parse lays the slots out and reports their total
    // execute stage, in launch order
    bool exec_frames = false;   // a frame of <= 64 KiB per workgroup (handoff, post_here)
    bool exec_blocks = false;   // accepted big frames, a workgroup per block job
    bool exec_big = false;      // big frames through the window (handoff); big_skip_origin: the jobs
    bool big_skip_origin = false;   // below the origin scratch's capacity are exec_blocks'
    bool exec_wave = false;     // seq_exec_kernel: frames of >= wave_min_dsize, version wave_version,
    uint32_t wave_min_dsize = 0;    // wave_blk: job lists of the block route
    int wave_version = 0;
    bool wave_blk = false;
    bool handoff = false;       // exec_frames / exec_big decode their ST_NOT_RUN frames themselves
    bool post_here = false;     // exec_frames posts the lone frame's results to the host
    // hand-off stage
    bool deferred = false;      // launch_lz4_wave_deferred over the frames still ST_NOT_RUN
};

inline Lz4Plan lz4_plan(const Lz4Request &q, const Lz4Switches &w)
{
    Lz4Plan P;
    const uint32_t n = q.nframes;
    const int version = (q.tune >> 8) & 0xFFF;
    const bool one = one_route(n, q.route, w);
    P.klass = q.route == ROUTE_WAVE || (q.route == ROUTE_AUTO && w.engine == ENGINE_WAVE) ? LZ4_WAVE_ENGINE
              : one                                                                     ? LZ4_ONE
                                                                                        : LZ4_TWO_PHASE;
    P.parse = one ? ParseRoute{0, 0} : parse_route(n, q.route, w);
    const uint64_t jw = (uint64_t)n * kMaxBlockJobs;
    P.jlanes = (uint32_t)(jw < kJobsCapMax ? jw : kJobsCapMax);
    // the one-frame route's frames of > 64 KiB: their blocks
    // of <= 64 KiB get block-plan jobs, parsed a workgroup each, and the
    // windowed execute takes them; not under an execute diagnostic
    const bool big = one && q.max_dsize > kFrameExecMax && !w.one_big_off && version == 0 && !q.block_denied;
    P.block = big ? BlockRoute{true, 0, 1, 4} : one ? BlockRoute{false, 0, 0, 7} : block_route(n, q.route, P.parse, w);
    if (q.block_denied)   // no room: the chunk parse takes the frames as it does without the route
        P.block = BlockRoute{false, 0, 0, 7};
    // the accepted big frames block-parallel (their jobs: at most
    // ceil(max_dsize / 64 KiB) a frame; the device API's unknown sizes: the
    // job lanes, at most kOriginJobsMax -- a frame with a job past the scratch
    // goes through the window), the others through the window
    const bool blocks = big && !w.one_blocks_off && !q.origin_denied;
    if (blocks) {
        const uint64_t by_size = (uint64_t)n * (((uint64_t)q.max_dsize + 65535) / 65536);
        const uint64_t cap = P.jlanes < kOriginJobsMax ? P.jlanes : kOriginJobsMax;
        P.origin_jobs = (uint32_t)(by_size < cap ? by_size : cap);
    }
    // one frame on the one-frame route: the chunk kernel does the plan's work
    // (frames in order: a lone frame, or the caller says so -- the reader's
    // batches are file order)
    const bool solo = one && (n == 1 || q.in_order) && (q.stages & 3) == 3 && !big;
    if ((q.stages & 1) && !solo) {
        P.plan = true;
        P.plan_groups = (n + 255) / 256 < kPlanGroups ? (n + 255) / 256 : kPlanGroups;
        P.block_plan = !P.block.on ? BLOCK_PLAN_NONE : P.plan_groups == 1 ? BLOCK_PLAN_INSIDE : BLOCK_PLAN_SEPARATE;
        P.scan_layout = q.scan_layout;
    }
    // parse: each kernel takes the frames of its compressed-size range and
    // skips the others (launched only when the range is not empty); block
    // route jobs before the chunk parse, which accepts or re-parses their
    // frames
    if (q.stages & 2) {
        P.job_parse = big;
        P.lean_blocks = !big && P.block.on;
        P.lean = P.parse.chunk_min > P.parse.lean_min;
        P.lean_min = P.parse.lean_min;
        P.lean_max = P.parse.chunk_min;
        P.lean_diag = q.tune & 0xFF;
        P.scan = P.parse.lean_min != 0;
        P.scan_max = P.parse.lean_min < P.parse.chunk_min ? P.parse.lean_min : P.parse.chunk_min;
        P.chunk = P.parse.chunk_min != kNoSize;
        P.chunk_one = one;
        P.chunk_solo = solo;
    }
    if (q.stages & 4) {
        // the one-frame route executes a frame of <= 64 KiB per workgroup
        if (one && !w.one_exec_wave && version == 0) {
            // hand-offs of <= 64 KiB frames decoded inside (when the batch has
            // no bigger frame, or its bigger frames go through the window,
            // and the hand-off stage is asked for: no hand-off launch)
            P.handoff = (q.stages & 8) && (q.max_dsize <= kFrameExecMax || big);
            // a lone frame posts its results to the host itself (no download)
            P.post_here = q.post && P.handoff && n == 1 && !big;
            // (a lone big frame: nothing for it -- unless max_dsize is only a
            // bound and the frame may be a small one)
            P.exec_frames = !(big && n == 1) || q.dsize_bound;
            P.exec_blocks = blocks;
            P.exec_big = big;
            P.big_skip_origin = blocks;
            P.exec_wave = !big && q.max_dsize > kFrameExecMax;
            P.wave_min_dsize = kFrameExecMax + 1;
        } else {
            P.exec_wave = true;
            P.wave_version = version;
            P.wave_blk = P.block.on;
        }
    }
    P.deferred = (q.stages & 8) && !P.handoff;
    return P;
}

// ---- names, for tooling ----------------------------------------------------------
// The parse kernel a frame of c_size compressed bytes takes in a batch of
// nframes (what a kernel trace shows).  Frame sizes are not an input: a
// one-frame batch is named for its chunk kernel whatever they are.
inline const char *lz4_parse_kernel_name(uint32_t nframes, uint32_t c_size, int route, const Lz4Switches &w)
{
    Lz4Request q;
    q.nframes = nframes;
    q.route = route;
    q.max_dsize = kFrameExecMax;
    const Lz4Plan P = lz4_plan(q, w);
    // (a forced route other than ROUTE_WAVE is the two-phase decoder whatever the engine switch)
    if (P.klass == LZ4_WAVE_ENGINE && route == ROUTE_AUTO)
        return "lz4_wave_kernel";
    if (P.chunk_one)
        return "lz4_chunk_kernel (one-frame route)";
    // (block route: frames of > 64 KiB decoded; named for the compressed
    // sizes those frames have)
    if (P.block.on && c_size >= P.block.min_csize && c_size >= 65536)
        return "lz4_lean_kernel (block route)";
    if (c_size >= P.parse.chunk_min)
        return "lz4_chunk_kernel";
    return c_size >= P.parse.lean_min ? "lz4_lean_pair_kernel" : "lz4_scan_kernel";
}

// Automatic choice: the two-phase decoder for every batch; the
// wave-per-frame kernel decodes only the frames the parse hands off, unless
// ZSEEK_HIP_KERNEL=wave forces it for every frame.  Never ENGINE_AUTO.
inline int lz4_pick_engine(uint32_t nframes, const Lz4Switches &w)
{
    Lz4Request q;
    q.nframes = nframes;
    return lz4_plan(q, w).klass == LZ4_WAVE_ENGINE ? ENGINE_WAVE : ENGINE_SPLIT;
}

// Name of the dominant kernel an AUTO batch of nframes frames uses (execute
// kernel of the two-phase decoder, or the wave kernel), for matching profiler
// output.
inline const char *lz4_exec_kernel_name(uint32_t nframes, const Lz4Switches &w)
{
    return lz4_pick_engine(nframes, w) == ENGINE_SPLIT ? "seq_exec_kernel" : "lz4_wave_kernel";
}

}   // namespace zsk

#endif
