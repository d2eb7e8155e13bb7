"""Which kernels an LZ4 batch gets, on the CPU: libzseek_amd/csrc/lz4_route.h's
lz4_plan -- the one function launch_lz4_split walks and parse_kernel_name /
lz4_kernel_name / lz4_pick_engine report from -- through
tests/native/lz4_route_shim.cpp.

  * tests/golden/lz4_route_trace.json: kernel traces of scripts/lz4_route_probe.py
    recorded on an MI355X from the library as it was BEFORE the decision moved
    into lz4_route.h (make_lz4_route_trace.py), under the default environment
    and each routing switch.  For every recorded case the plan of the recorded
    request(s) must list exactly the recorded kernels, in order (STEPS).
  * a restatement of DESIGN.md §3's routing table in Python (model), held to
    lz4_plan over the product of batch-size boundaries, routes, frame sizes,
    stage masks, tuning words, switches and denied reservations;
  * a denied reservation re-plans onto the path without it;
  * the names tooling reads (bench.py reads parse_kernel_name) are the recorded
    library's, string for string."""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import pathlib
import subprocess

import pytest

from conftest import GOLDEN

ROOT = pathlib.Path(__file__).resolve().parents[1]
SHIM = str(ROOT / "tests/native/lz4_route_shim.cpp")
TRACE = json.load(open(os.path.join(GOLDEN, "lz4_route_trace.json")))

SWITCHES = ["ZSEEK_HIP_KERNEL", "ZSEEK_PARSE", "ZSEEK_BLOCK_ROUTE", "ZSEEK_ONE_ROUTE", "ZSEEK_ONE_BIG",
            "ZSEEK_ONE_BLOCKS", "ZSEEK_ONE_EXEC"]
REQUEST_FIELDS = ["nframes", "route", "stages", "tune", "stop_last", "max_dsize", "in_order", "scan_layout", "post",
                  "block_denied", "origin_denied"]
PLAN_FIELDS = ["klass", "chunk_min", "lean_min", "block_on", "block_min_csize", "block_min_jobs", "block_max_bsid",
               "jlanes", "origin_jobs", "plan", "plan_groups", "block_plan", "scan_layout", "job_parse",
               "lean_blocks", "lean", "lean_lo", "lean_hi", "lean_diag", "scan", "scan_max", "chunk", "chunk_one",
               "chunk_solo", "exec_frames", "exec_blocks", "exec_big", "big_skip_origin", "exec_wave",
               "wave_min_dsize", "wave_version", "wave_blk", "handoff", "post_here", "deferred"]
CONSTANTS = {"kOneMaxFrames": 64, "kFrameExecMax": 65536, "kLaneBatchMin": 32768, "kChunkMinLaneBatch": 49152,
             "kChunkMinSmallBatch": 8192, "kLeanMinCsize": 12288, "kBlockRouteMinFrames": 1024,
             "kBlockRouteMinJobs": 16384, "kMaxBlockJobs": 64, "kJobsCapMax": 1 << 21, "kOriginJobsMax": 1024,
             "kPlanGroups": 256}
AUTO, WAVE, LEAN, SCAN, CHUNK, BLOCK, ONE = range(7)
WAVE_ENGINE, ONE_FRAME, TWO_PHASE = 0, 1, 2
INSIDE, SEPARATE = 1, 2
NO = 0xFFFFFFFF

# The launcher's steps in launch order: (name, taken when, the kernel it
# launches).  No step is optional: every launcher behind a step returns
# without a launch only for zero frames or zero job lanes (launch_lz4_* and
# launch_seq_exec_* begin `if (nframes == 0) return 0` / `if (jobs == 0)`),
# launch_lz4_split itself returns before planning for zero frames, and job
# lanes are 64 per frame -- so a step the plan takes is exactly one launch.
# (lean: production builds launch the pair kernel whatever the diag word.)
STEPS = [
    ("plan", lambda p: p["plan"], "lz4_plan_direct_kernel"),
    ("block plan", lambda p: p["plan"] and p["block_plan"] == SEPARATE, "lz4_block_plan_kernel"),
    ("job parse", lambda p: p["job_parse"], "lz4_job_parse_kernel"),
    ("lean blocks", lambda p: p["lean_blocks"], "lz4_lean_kernel"),
    ("lean", lambda p: p["lean"], "lz4_lean_pair_kernel"),
    ("scan", lambda p: p["scan"], "lz4_scan_kernel"),
    ("chunk", lambda p: p["chunk"], "lz4_chunk_kernel"),
    ("execute frames", lambda p: p["exec_frames"], "seq_exec_frame_kernel"),
    ("execute blocks", lambda p: p["exec_blocks"], "seq_exec_blocks_kernel"),
    ("execute big", lambda p: p["exec_big"], "seq_exec_big_kernel"),
    ("execute wave", lambda p: p["exec_wave"], "seq_exec_kernel"),
    ("hand-off", lambda p: p["deferred"], "lz4_wave_kernel"),
]


def launches(p) -> list:
    """the kernels a plan's steps launch; the wave engine: its kernel alone"""
    if p["klass"] == WAVE_ENGINE:
        return ["lz4_wave_kernel"]
    return [kernel for _, taken, kernel in STEPS if taken(p)]


@pytest.fixture(scope="module")
def lr(tmp_path_factory):
    so = tmp_path_factory.mktemp("lz4_route") / "liblz4_route.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-o", str(so), SHIM],
                   check=True)
    L = C.CDLL(str(so))
    L.lr_plan.restype = None
    L.lr_parse_kernel_name.restype = C.c_char_p
    L.lr_exec_kernel_name.restype = C.c_char_p
    return L


_ENVS = {}


def c_env(env: dict):
    key = tuple(sorted(env.items()))
    if key not in _ENVS:
        _ENVS[key] = (C.c_char_p * 7)(*[env[k].encode() if k in env else None for k in SWITCHES])
    return _ENVS[key]


def plan(lr, rq: dict, env) -> dict:
    q = (C.c_uint32 * len(REQUEST_FIELDS))(*[int(rq.get(k, 0)) for k in REQUEST_FIELDS])
    out = (C.c_uint32 * len(PLAN_FIELDS))()
    lr.lr_plan(q, env if not isinstance(env, dict) else c_env(env), out)
    return dict(zip(PLAN_FIELDS, out))


def test_constants(lr):
    out = (C.c_uint32 * len(CONSTANTS))()
    lr.lr_constants(out)
    assert dict(zip(CONSTANTS, out)) == CONSTANTS


# ---------------------------------------------------------------------------
# the recording
# ---------------------------------------------------------------------------
def test_recording_covers_what_it_should():
    s = TRACE["settings"]
    assert list(s) == ["default", "one_route_0", "one_big_0", "one_blocks_0", "one_exec_wave", "parse_scan",
                       "parse_chunk", "block_route_0", "hip_kernel_wave"]
    names = set(s["default"]["cases"])
    assert all(set(v["cases"]) == names for v in s.values())
    for engine in ("auto", "wave", "lean", "scan", "chunk", "block", "one"):
        for n in (1, 2, 64, 65, 255, 256, 257, 1023, 1024, 32767, 32768):
            assert f"api/{engine}/{n}" in names
    for name in ("4k_cache0", "2_frames", "65_frames_pread", "65_frames_preadv", "1m_frame", "1m_two_frames",
                 "preadv_scattered"):
        assert f"host/{name}" in names and f"image/{name}" in names
    assert {"host/4k_cache1", "image/indirect_4", "image/indirect_65"} <= names
    # every step's kernel was seen somewhere, and nothing but the steps' kernels
    seen = {k for v in s.values() for c in v["cases"].values() for k in c["kernels"]}
    assert seen == {kernel for _, _, kernel in STEPS}


@pytest.mark.parametrize("setting", list(TRACE["settings"]))
def test_plan_lists_the_recorded_kernels(lr, setting):
    rec = TRACE["settings"][setting]
    env = c_env(rec["env"])
    for name, case in rec["cases"].items():
        want = [k for rq in case["requests"] for k in launches(plan(lr, rq, env))]
        assert want == case["kernels"], (setting, name)


@pytest.mark.parametrize("setting", list(TRACE["settings"]))
def test_names_are_the_recorded_library_s(lr, setting):
    rec = TRACE["settings"][setting]
    env = c_env(rec["env"])
    assert len(rec["names"]) == 110
    for n, c_size, parse_name, exec_name in rec["names"]:
        assert lr.lr_parse_kernel_name(n, c_size, AUTO, env).decode() == parse_name, (n, c_size)
        assert lr.lr_exec_kernel_name(n, env).decode() == exec_name, n
        assert lr.lr_pick_engine(n, env) == (2 if exec_name == "lz4_wave_kernel" else 1)


def test_parse_kernel_name_ignores_frame_sizes_on_the_one_frame_route(lr):
    """no max_dsize input: a one-frame batch is named for the chunk kernel
    whatever its frames' sizes (bench.py reads the string)"""
    for c_size in (1, 65536, 1 << 20, NO):
        assert lr.lr_parse_kernel_name(1, c_size, AUTO, c_env({})) == b"lz4_chunk_kernel (one-frame route)"
        assert lr.lr_parse_kernel_name(1000, c_size, ONE, c_env({})) == b"lz4_chunk_kernel (one-frame route)"


# ---------------------------------------------------------------------------
# DESIGN.md §3's table, restated
# ---------------------------------------------------------------------------
def model(q: dict, env: dict) -> dict:
    n, route, stages = q["nframes"], q["route"], q["stages"]
    diag, version = q["tune"] & 0xFF, (q["tune"] >> 8) & 0xFFF
    dmax = q["max_dsize"]
    p = dict.fromkeys(PLAN_FIELDS, 0)
    # class
    wave_engine = route == WAVE or (route == AUTO and env.get("ZSEEK_HIP_KERNEL") == "wave")
    one = route == ONE or (route == AUTO and n <= 64 and env.get("ZSEEK_ONE_ROUTE") != "0" and "ZSEEK_PARSE" not in env)
    p["klass"] = WAVE_ENGINE if wave_engine else ONE_FRAME if one else TWO_PHASE
    # parse bounds
    if one or route in (CHUNK, BLOCK):
        cmin = lmin = 0
    elif route == LEAN:
        cmin, lmin = NO, 0
    elif route == SCAN:
        cmin = lmin = NO
    else:
        cmin = {"scan": NO, "chunk": 0}.get(env.get("ZSEEK_PARSE"), 49152 if n >= 32768 else 8192)
        lmin = min(cmin, 12288)
    p["chunk_min"], p["lean_min"] = cmin, lmin
    # block jobs
    big = (one and dmax > 65536 and env.get("ZSEEK_ONE_BIG") != "0" and version == 0 and not q["block_denied"])
    block = (0, 0, 0, 7)
    if big:
        block = (1, 0, 1, 4)
    elif not one and not q["block_denied"]:
        if route == BLOCK:
            block = (1, 0, 1, 7)
        elif route == AUTO and env.get("ZSEEK_BLOCK_ROUTE") != "0" and 1024 <= n < 32768 and cmin != NO:
            block = (1, cmin, 16384, 7)
    p["block_on"], p["block_min_csize"], p["block_min_jobs"], p["block_max_bsid"] = block
    p["jlanes"] = min(64 * n, 1 << 21)
    blocks = big and env.get("ZSEEK_ONE_BLOCKS") != "0" and not q["origin_denied"]
    if blocks:
        p["origin_jobs"] = min(n * -(-dmax // 65536), p["jlanes"], 1024)
    # plan
    solo = one and (n == 1 or q["in_order"]) and stages & 3 == 3 and not big
    if stages & 1 and not solo:
        p["plan"], p["plan_groups"] = 1, min(-(-n // 256), 256)
        p["block_plan"] = 0 if not block[0] else INSIDE if p["plan_groups"] == 1 else SEPARATE
        p["scan_layout"] = int(q["scan_layout"])
    # parse
    if stages & 2:
        p["job_parse"], p["lean_blocks"] = int(big), int(bool(block[0]) and not big)
        p["lean"], p["lean_lo"], p["lean_hi"], p["lean_diag"] = int(cmin > lmin), lmin, cmin, diag
        p["scan"], p["scan_max"] = int(lmin != 0), min(lmin, cmin)
        p["chunk"], p["chunk_one"], p["chunk_solo"] = int(cmin != NO), int(one), int(solo)
    # execute
    if stages & 4:
        if one and env.get("ZSEEK_ONE_EXEC") != "wave" and version == 0:
            p["handoff"] = int(bool(stages & 8) and (dmax <= 65536 or big))
            p["post_here"] = int(q["post"] and p["handoff"] and n == 1 and not big)
            p["exec_frames"] = int(not (big and n == 1))
            p["exec_blocks"] = p["big_skip_origin"] = int(blocks)
            p["exec_big"] = int(big)
            p["exec_wave"], p["wave_min_dsize"] = int(not big and dmax > 65536), 65537
        else:
            p["exec_wave"], p["wave_version"], p["wave_blk"] = 1, version, block[0]
    p["deferred"] = int(bool(stages & 8) and not p["handoff"])
    return p


NFRAMES = [1, 2, 64, 65, 255, 256, 257, 1023, 1024, 32767, 32768]
ENVS = [{}, {"ZSEEK_ONE_ROUTE": "0"}, {"ZSEEK_ONE_BIG": "0"}, {"ZSEEK_ONE_BLOCKS": "0"}, {"ZSEEK_ONE_EXEC": "wave"},
        {"ZSEEK_PARSE": "scan"}, {"ZSEEK_PARSE": "chunk"}, {"ZSEEK_BLOCK_ROUTE": "0"}, {"ZSEEK_HIP_KERNEL": "wave"},
        {"ZSEEK_HIP_KERNEL": "split"}, {"ZSEEK_PARSE": "other"}, {"ZSEEK_ONE_ROUTE": "1"}]
TUNES = [0, 0x80, 0x400 << 8]   # production, a lean parse diag value, an execute version


def requests(denied=((0, 0), (1, 0), (0, 1), (1, 1))):
    for n, route, dmax, in_order, stages, tune, (bd, od) in itertools.product(
            NFRAMES, range(7), (1, 65536, 65537, NO), (0, 1), (1, 3, 4, 15), TUNES, denied):
        yield {"nframes": n, "route": route, "stages": stages, "tune": tune, "stop_last": NO, "max_dsize": dmax,
               "in_order": in_order, "scan_layout": int(not in_order), "post": int(n == 1), "block_denied": bd,
               "origin_denied": od}


def test_plan_is_the_design_table(lr):
    for env in ENVS:
        ce = c_env(env)
        for q in requests():
            assert plan(lr, q, ce) == model(q, env), (env, q)


def test_a_denied_reservation_replans_without_it(lr):
    """no block scratch: exactly the plan of the same request on the
    chunk-parse path -- the one-frame route as with ZSEEK_ONE_BIG=0, AUTO as
    with ZSEEK_BLOCK_ROUTE=0, ROUTE_BLOCK as ROUTE_CHUNK -- with no job parse
    and no blocks or big execute; no origin scratch: the plan with
    ZSEEK_ONE_BLOCKS=0"""
    for env in ENVS:
        for q in requests(denied=((0, 0),)):
            p = plan(lr, q, env)
            without = dict(env, ZSEEK_ONE_BIG="0", ZSEEK_BLOCK_ROUTE="0")
            as_chunk = dict(q, route=CHUNK) if q["route"] == BLOCK else q
            got = plan(lr, dict(q, block_denied=1), env)
            assert got == plan(lr, as_chunk, without), (env, q)
            assert got["klass"] == p["klass"]
            assert not (got["block_on"] or got["job_parse"] or got["lean_blocks"] or got["exec_blocks"] or
                        got["exec_big"] or got["origin_jobs"] or got["block_plan"])
            assert plan(lr, dict(q, origin_denied=1), env) == plan(lr, q, dict(env, ZSEEK_ONE_BLOCKS="0")), (env, q)
