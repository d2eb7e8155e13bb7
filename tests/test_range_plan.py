"""The host planner of a vectored read (zsk_preadv), on the CPU:
libzseek_amd/csrc/range_plan.h's pure functions -- the touched frames, their
runs of adjacent frames (one pread each), the batches, the (range, frame)
segments the gather kernel moves, and the per-range results from the frames'
statuses -- plus the entry points' argument checks, which need no device.
reader_vec.cpp calls exactly these."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

from conftest import golden_file

ROOT = pathlib.Path(__file__).resolve().parents[1]
F = 65536
D_OFF = [i * F for i in range(33)]   # 32 frames of 64 KiB
SIZE = D_OFF[-1]


@pytest.fixture(scope="module")
def rp(tmp_path_factory):
    so = tmp_path_factory.mktemp("range_plan") / "librange_plan.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/range_plan_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.rp_plan.restype = C.c_void_p
    L.rp_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint64]
    L.rp_free.restype = None
    L.rp_free.argtypes = [C.c_void_p]
    L.rp_count.restype = C.c_size_t
    L.rp_count.argtypes = [C.c_void_p, C.c_int]
    for fn in (L.rp_frames, L.rp_runs, L.rp_batches, L.rp_segs):
        fn.restype = None
        fn.argtypes = [C.c_void_p, C.c_void_p]
    L.rp_results.restype = C.c_size_t
    L.rp_results.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return L


class Plan:
    """plan_ranges' output as Python lists; ranges: (offset, count, dst_off)."""

    def __init__(self, rp, ranges, d_off=D_OFF, batch_bytes=64 << 20):
        self.rp = rp
        self.rg = np.ascontiguousarray(np.array(ranges, np.uint64).reshape(-1, 3))
        self.d = np.ascontiguousarray(d_off, np.uint64)
        self.h = rp.rp_plan(self.rg.ctypes.data, len(self.rg), self.d.ctypes.data, len(self.d) - 1, batch_bytes)

        def grab(fn, what, width):
            a = np.zeros((rp.rp_count(self.h, what), width), np.uint64)
            fn(self.h, a.ctypes.data)
            return a.astype(np.int64).tolist()

        self.frames = [x[0] for x in grab(rp.rp_frames, 0, 1)]
        self.runs = [tuple(x) for x in grab(rp.rp_runs, 1, 2)]
        keys = ("t0", "t1", "r0", "r1", "s0", "s1", "d_bytes", "out_bytes")
        self.batches = [dict(zip(keys, x)) for x in grab(rp.rp_batches, 2, 8)]
        keys = ("src_off", "dst_off", "len", "frame", "range", "cum")
        self.segs = [dict(zip(keys, x)) for x in grab(rp.rp_segs, 3, 6)]

    def results(self, status):
        st = np.ascontiguousarray(status, np.int32)
        assert len(st) == len(self.frames)
        res = np.zeros(len(self.rg), np.int64)
        ok = self.rp.rp_results(self.h, self.rg.ctypes.data, len(self.rg), self.d.ctypes.data, len(self.d) - 1,
                                st.ctypes.data, res.ctypes.data)
        return res.tolist(), ok

    def close(self):
        self.rp.rp_free(self.h)


def test_frames_deduplicated_and_sorted(rp):
    p = Plan(rp, [(9 * F + 5, 10, 0), (2 * F, 100, 10), (9 * F + 100, 50, 110), (2 * F + 7, 1, 160),
                  (30 * F, 3 * F, 161), (2 * F, 100, 161 + 2 * F)])
    assert p.frames == [2, 9, 30, 31]
    p.close()


def test_runs_split_where_frames_are_not_adjacent(rp):
    p = Plan(rp, [(15 * F, 1, 0), (7 * F + 1, F, 1), (0, 2 * F, 1 + F)])
    assert p.frames == [0, 1, 7, 8, 15]
    assert p.runs == [(0, 2), (7, 9), (15, 16)]                 # three preads, an untouched frame never read
    assert len(p.batches) == 1 and (p.batches[0]["r0"], p.batches[0]["r1"]) == (0, 3)
    p.close()


def test_segments_tile_each_range_exactly(rp):
    rng = np.random.default_rng(7)
    ranges, at = [], 3
    for _ in range(200):
        off = int(rng.integers(0, SIZE))
        cnt = int(rng.integers(1, 4 * F))
        ranges.append((off, cnt, at))
        at += cnt + 5
    p = Plan(rp, ranges, batch_bytes=4 * F)
    by_range = {}
    for b in p.batches:
        packed = np.cumsum([0] + [D_OFF[f + 1] - D_OFF[f] for f in p.frames[b["t0"]:b["t1"]]])
        cum = 0
        for s in p.segs[b["s0"]:b["s1"]]:
            f = p.frames[b["t0"] + s["frame"]]
            in_frame = s["src_off"] - int(packed[s["frame"]])
            assert 0 <= in_frame and in_frame + s["len"] <= D_OFF[f + 1] - D_OFF[f]
            assert s["cum"] == cum                               # the batch's length prefix sum
            cum += s["len"]
            by_range.setdefault(s["range"], []).append((D_OFF[f] + in_frame, s["dst_off"], s["len"]))
        assert cum == b["out_bytes"]
    for r, (off, cnt, dst) in enumerate(ranges):
        want = min(cnt, SIZE - off)
        pieces = sorted(by_range[r])
        assert pieces[0][0] == off and pieces[0][1] == dst
        for (a, da, la), (b_, db, _) in zip(pieces, pieces[1:]):
            assert a + la == b_ and da + la == db                # no gap, no overlap, source and destination
        assert sum(x[2] for x in pieces) == want
        assert len(pieces) == (off + want - 1) // F - off // F + 1   # one segment per frame touched
    p.close()


def test_range_across_three_frames_yields_three_segments(rp):
    p = Plan(rp, [(4 * F - 10, F + 20, 1000)])
    assert p.frames == [3, 4, 5] and p.runs == [(3, 6)]
    assert [(s["src_off"], s["dst_off"], s["len"], s["frame"]) for s in p.segs] == [
        (F - 10, 1000, 10, 0), (F, 1010, F, 1), (2 * F, 1010 + F, 10, 2)]
    p.close()


def test_empty_ranges_yield_nothing(rp):
    p = Plan(rp, [(5, 0, 0), (SIZE, 10, 0), (SIZE + 99, 10, 0), (2**63, 2**63, 0)])
    assert p.frames == [] and p.runs == [] and p.batches == [] and p.segs == []
    res, ok = p.results([])
    assert res == [0, 0, 0, 0] and ok == 4
    p.close()
    p = Plan(rp, [(SIZE - 1, 2**64 - 1, 0)])                     # count past EOF (and past 2^64)
    assert p.frames == [31] and [(s["src_off"], s["len"]) for s in p.segs] == [(F - 1, 1)]
    assert p.results([0]) == ([1], 1)
    p.close()


def test_batch_split_honours_batch_bytes(rp):
    p = Plan(rp, [(0, SIZE, 0), (5 * F + 1, 10, SIZE)], batch_bytes=3 * F)
    assert p.frames == list(range(32))
    assert [(b["t0"], b["t1"]) for b in p.batches] == [(i, min(i + 3, 32)) for i in range(0, 32, 3)]
    assert all(b["d_bytes"] <= 3 * F for b in p.batches)
    # a run never crosses a batch: the whole-file run is cut at every batch end
    assert p.runs == [(i, min(i + 3, 32)) for i in range(0, 32, 3)]
    # the small range's segment sits in the batch of frame 5, at the frame's packed offset
    small = [s for s in p.segs if s["range"] == 1]
    assert len(small) == 1 and small[0]["frame"] == 2 and small[0]["src_off"] == 2 * F + 1
    b = p.batches[1]
    assert small[0] in p.segs[b["s0"]:b["s1"]]
    p.close()
    # frames bigger than batch_bytes: one per batch
    p = Plan(rp, [(0, 3 * F, 0)], batch_bytes=4096)
    assert [(b["t0"], b["t1"]) for b in p.batches] == [(0, 1), (1, 2), (2, 3)]
    p.close()


def test_results_from_statuses(rp):
    ranges = [(2 * F + 5, 100, 0),            # inside frame 2
              (1 * F + 7, 3 * F, 100),        # frames 1..4, frame 2 in the middle
              (2 * F, 10, 100 + 3 * F),       # starts at frame 2's first byte
              (0, 2 * F, 200 + 3 * F),        # frames 0, 1: ends where frame 2 starts
              (6 * F - 1, 2 * F, 200 + 5 * F),   # frames 5, 6, 7: the bad frame 7 is in a later batch
              (7 * F + 1, 5, 200 + 7 * F)]
    p = Plan(rp, ranges, batch_bytes=4 * F)
    assert p.frames == list(range(8)) and len(p.batches) == 2
    good = [0] * 8
    assert p.results(good) == ([100, 3 * F, 10, 2 * F, 2 * F, 5], 6)
    bad = list(good)
    bad[2] = 17
    bad[7] = 0x7FFF
    res, ok = p.results(bad)
    assert res == [-1,              # a bad first frame
                   F - 7,           # a bad middle frame: the bytes before it
                   -1, 2 * F,
                   F + 1,           # the bytes of frames 5 and 6, across the batch boundary
                   -1]
    assert ok == 1
    p.close()


# ---------------------------------------------------------------------------
# the entry points' argument checks (no device needed)
# ---------------------------------------------------------------------------
def test_preadv_null_reader(zs):
    L = zs.lib()
    err = C.create_string_buffer(80)
    rg = np.zeros(2, zs.RANGE_DTYPE)
    rg["count"] = 4
    buf = C.create_string_buffer(16)
    for fn in (L.zsk_preadv, L.zsk_preadv_device):
        err.value = b""
        rg["result"] = 7
        assert fn(None, buf, rg.ctypes.data, 2, None, err) == -1
        assert err.value == b"invalid reader"
        assert rg["result"].tolist() == [-1, -1]


def test_preadv_no_ranges_and_null_ranges(zs):
    with zs.Reader(golden_file("lz4_64k_direct"), 0) as r:
        buf = np.zeros(16, np.uint8)
        assert r.preadv_raw(buf.ctypes.data, np.zeros(0, zs.RANGE_DTYPE)) == 0
        assert zs.lib().zsk_preadv(r.handle, buf.ctypes.data, None, 3, None, r._err) == -1
        assert r.error == "invalid ranges"
        assert r.preadv([]) == ([], 0)
        # ranges that touch no frame need no device either
        size = r.stats()["decompressed_size"]
        got, n_ok = r.preadv([(0, 0), (size, 10), (size + 5, 1)])
        assert got == [b"", b"", b""] and n_ok == 3


def test_gather_segments_nothing_to_do(zs):
    assert zs.lib().zsk_gather_segments(None, 0, None, None, None, None) == 0
