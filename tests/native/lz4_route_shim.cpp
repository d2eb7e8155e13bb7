// Test-only C shim over libzseek_amd/csrc/lz4_route.h (which kernels an LZ4
// batch gets: pure, no HIP): tests/test_lz4_route.py builds it with g++ and
// calls it via ctypes.  Switches are given as the seven variables' values in
// the order of lz4_switches_of (null: unset).
#include "../../libzseek_amd/csrc/lz4_route.h"

using namespace zsk;

static Lz4Switches sw(const char *const *env)
{
    return lz4_switches_of(env[0], env[1], env[2], env[3], env[4], env[5], env[6]);
}

extern "C" {

// rq: nframes, route, stages, tune, stop_last, max_dsize, in_order,
// scan_layout, post, block_denied, origin_denied.  out: PLAN_FIELDS of the test.
void lr_plan(const uint32_t *rq, const char *const *env, uint32_t *out)
{
    Lz4Request q;
    q.nframes = rq[0];
    q.route = (int)rq[1];
    q.stages = (int)rq[2];
    q.tune = (int)rq[3];
    q.stop_last = rq[4];
    q.max_dsize = rq[5];
    q.in_order = rq[6];
    q.scan_layout = rq[7];
    q.post = rq[8];
    q.block_denied = rq[9];
    q.origin_denied = rq[10];
    const Lz4Plan P = lz4_plan(q, sw(env));
    const uint32_t f[] = {(uint32_t)P.klass, P.parse.chunk_min, P.parse.lean_min, P.block.on, P.block.min_csize,
                          P.block.min_jobs, P.block.max_bsid, P.jlanes, P.origin_jobs, P.plan, P.plan_groups,
                          (uint32_t)P.block_plan, P.scan_layout, P.job_parse, P.lean_blocks, P.lean, P.lean_min,
                          P.lean_max, (uint32_t)P.lean_diag, P.scan, P.scan_max, P.chunk, P.chunk_one, P.chunk_solo,
                          P.exec_frames, P.exec_blocks, P.exec_big, P.big_skip_origin, P.exec_wave, P.wave_min_dsize,
                          (uint32_t)P.wave_version, P.wave_blk, P.handoff, P.post_here, P.deferred};
    for (unsigned i = 0; i < sizeof(f) / sizeof(f[0]); i++)
        out[i] = f[i];
}

const char *lr_parse_kernel_name(uint32_t nframes, uint32_t c_size, int route, const char *const *env)
{
    return lz4_parse_kernel_name(nframes, c_size, route, sw(env));
}

const char *lr_exec_kernel_name(uint32_t nframes, const char *const *env)
{
    return lz4_exec_kernel_name(nframes, sw(env));
}

int lr_pick_engine(uint32_t nframes, const char *const *env)
{
    return lz4_pick_engine(nframes, sw(env));
}

// the named thresholds, in the order of the test's CONSTANTS
void lr_constants(uint32_t *out)
{
    const uint32_t c[] = {kOneMaxFrames,      kFrameExecMax,        kLaneBatchMin,      kChunkMinLaneBatch,
                          kChunkMinSmallBatch, kLeanMinCsize,        kBlockRouteMinFrames, kBlockRouteMinJobs,
                          kMaxBlockJobs,      kJobsCapMax,          kOriginJobsMax,     kPlanGroups};
    for (unsigned i = 0; i < sizeof(c) / sizeof(c[0]); i++)
        out[i] = c[i];
}
}
