"""The device-side per-range results of zsk_preadv_device_async, on the CPU:
libzseek_amd/csrc/range_result.h's shared functions driven the way
range_result_kernel drives them -- 64 "lanes" per range, chunk by chunk, a
ballot's lowest set bit, early exit -- against range_plan.h's range_results,
which is the yardstick (the synchronous call's arithmetic), over plans and
status vectors chosen for the walk's edges.  Plus the new entry point's
declaration / export and the argument checks that need no device."""
from __future__ import annotations

import ctypes as C
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest

from conftest import golden_file

ROOT = pathlib.Path(__file__).resolve().parents[1]
F = 65536
D_OFF = [i * F for i in range(33)]   # test_range_plan.py's layout: 32 frames of 64 KiB
SIZE = D_OFF[-1]
# a zero-size frame (frame 3) among 64 KiB frames
D_ZERO = [0, F, 2 * F, 3 * F, 3 * F, 4 * F, 5 * F, 6 * F]
# 200 frames of 4 KiB with two zero-size ones: ranges of 64, 65 and 129 touched frames
K = 4096
D_LONG = np.cumsum([0] + [0 if i in (70, 150) else K for i in range(200)]).tolist()
ST_NOT_RUN = 0x7FFF


@pytest.fixture(scope="module")
def rr(tmp_path_factory):
    so = tmp_path_factory.mktemp("range_result") / "librange_result.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/range_result_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.rr_plan.restype = C.c_void_p
    L.rr_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint64]
    L.rr_free.restype = None
    L.rr_free.argtypes = [C.c_void_p]
    for fn in (L.rr_touched, L.rr_batches):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_void_p]
    L.rr_table.restype = None
    L.rr_table.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    for fn in (L.rr_lanes, L.rr_host):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return L


class Plan:
    """A plan over (offset, count) ranges; both result paths on a status vector."""

    def __init__(self, rr, ranges, d_off=D_OFF, batch_bytes=64 << 20):
        self.rr = rr
        self.rg = np.ascontiguousarray(np.array([(o, c, 0) for o, c in ranges], np.uint64).reshape(-1, 3))
        self.d = np.ascontiguousarray(d_off, np.uint64)
        self.args = (self.rg.ctypes.data, len(self.rg), self.d.ctypes.data, len(self.d) - 1)
        self.h = rr.rr_plan(*self.args, batch_bytes)
        self.touched = rr.rr_touched(self.h)
        self.nbatches = rr.rr_batches(self.h)

    def table(self):
        rows = np.zeros((len(self.rg), 4), np.uint64)
        t_doff = np.zeros(self.touched, np.uint64)
        self.rr.rr_table(self.h, *self.args, rows.ctypes.data, t_doff.ctypes.data)
        return rows.astype(np.int64).tolist(), t_doff.astype(np.int64).tolist()

    def both(self, status):
        st = np.ascontiguousarray(status, np.int32)
        assert len(st) == self.touched
        out = []
        for fn in (self.rr.rr_lanes, self.rr.rr_host):
            res = np.full(len(self.rg), 12345, np.int64)
            ok = fn(self.h, *self.args, st.ctypes.data, res.ctypes.data)
            out.append((res.tolist(), ok))
        return out

    def check(self, status):
        lanes, host = self.both(status)
        assert lanes == host
        return host

    def close(self):
        self.rr.rr_free(self.h)


def _mixed_ranges(d_off):
    """Empty ranges, ranges at / past EOF, duplicates, one range over the whole
    file, frame-boundary ends, spans."""
    size = d_off[-1]
    f = d_off[1] - d_off[0]
    return [(5, 0), (size, 10), (size + 99, 10), (2**63, 2**63),
            (0, size), (0, size),                       # the whole file, twice
            (size - 1, 2**64 - 1),                      # count past EOF
            (f + 7, 3 * f), (f + 7, 3 * f),             # a duplicate span
            (2 * f, 10), (0, 2 * f), (2 * f + 5, 100), (size - f, f), (size - 3, 100)]


@pytest.mark.parametrize("d_off,batch_bytes", [(D_OFF, 64 << 20), (D_OFF, 3 * F), (D_ZERO, 64 << 20),
                                               (D_ZERO, F), (D_LONG, 64 << 20), (D_LONG, 5 * K)])
def test_lanes_match_range_results(rr, d_off, batch_bytes):
    p = Plan(rr, _mixed_ranges(d_off), d_off, batch_bytes)
    if batch_bytes < d_off[-1]:
        assert p.nbatches > 1                            # several batches
    t = p.touched
    assert t == len(d_off) - 1                           # the whole-file range touches every frame
    res, ok = p.check([0] * t)
    size = d_off[-1]
    assert res == [0 if c == 0 or o >= size else min(c, size - o) for o, c in _mixed_ranges(d_off)]
    assert ok == len(res)
    # ST_NOT_RUN tails: the batches from some frame on were never queued
    for cut in (0, 1, t // 2, t - 1):
        p.check([0] * cut + [ST_NOT_RUN] * (t - cut))
    # 200 random status vectors (sparse and dense failures)
    rng = np.random.default_rng(20)
    for i in range(200):
        density = (0.0, 0.02, 0.3, 1.0)[i % 4] if i >= 4 else 0.02
        st = np.where(rng.random(t) < density, rng.integers(1, 0x8000, t), 0)
        if i % 7 == 0:
            st[int(rng.integers(0, t)):] = ST_NOT_RUN
        p.check(st)
    p.close()


def test_table_rows(rr):
    p = Plan(rr, [(2 * F + 5, 100), (SIZE - 3, 100), (7, 0), (SIZE, 1), (9 * F, F + 1)])
    rows, t_doff = p.table()
    assert t_doff == [2 * F, 9 * F, 10 * F, 31 * F]
    # offset, full, rt0, rtn
    assert rows == [[2 * F + 5, 100, 0, 1], [SIZE - 3, 3, 3, 1], [7, 0, 0, 0], [SIZE, 0, 0, 0], [9 * F, F + 1, 1, 2]]
    p.close()


def test_one_bad_frame_at_each_position_of_three(rr):
    ranges = [(4 * F - 10, F + 20), (0, F)]              # frames 3, 4, 5 and an untouched-by-failure range
    p = Plan(rr, ranges)
    assert p.touched == 4
    want = {1: [-1, F], 2: [10, F], 3: [10 + F, F]}      # touched index of the bad frame -> results
    for bad, res in want.items():
        st = [0] * 4
        st[bad] = 17
        assert p.check(st) == (res, 1)
    assert p.check([0, 0, 0, 0]) == ([F + 20, F], 2)
    assert p.check([5, 0, 0, 0]) == ([F + 20, -1], 1)
    p.close()


@pytest.mark.parametrize("nt", [64, 65, 129])
def test_chunk_edges(rr, nt):
    """A range of exactly nt touched frames (64: one full chunk; 65: one lane
    into the second; 129: one lane into the third), a bad frame at every
    position that matters: lanes 0, 62, 63 of a chunk and lane 0 of the next."""
    first, last = 3, 3 + nt - 1                          # frames 3 .. 66 / 67 / 131 (frame 70 has no bytes)
    assert D_LONG[last + 1] > D_LONG[last]
    off, end = D_LONG[first] + 9, D_LONG[last] + 1
    p = Plan(rr, [(off, end - off), (0, D_LONG[first])], D_LONG)
    rows, t_doff = p.table()
    assert rows[0][3] == nt and rows[0][2] == first
    t = p.touched
    assert p.check([0] * t) == ([end - off, D_LONG[first]], 2)
    for k in sorted({0, 1, 62, 63, 64, 65, 127, 128, nt - 1} & set(range(nt))):
        st = [0] * t
        st[first + k] = 3
        want = -1 if k == 0 else D_LONG[first + k] - off
        assert p.check(st) == ([want, D_LONG[first]], 1), k
        # a later failure does not matter, an earlier one does
        st[first + nt - 1] = 9
        assert p.check(st)[0][0] == want
    # lane 63 and lane 64 both bad: the first wins
    st = [0] * t
    if nt > 64:
        st[first + 63] = st[first + 64] = 1
        assert p.check(st)[0][0] == D_LONG[first + 63] - off
    p.close()


def test_whole_file_range_long_layout(rr):
    p = Plan(rr, [(0, D_LONG[-1])], D_LONG, batch_bytes=7 * K)
    assert p.touched == 200 and p.nbatches > 20
    for bad in (0, 63, 64, 70, 127, 128, 191, 192, 199):
        st = [0] * 200
        st[bad] = ST_NOT_RUN
        assert p.check(st) == ([-1 if bad == 0 else D_LONG[bad]], 0)
    p.close()


# ---------------------------------------------------------------------------
# the entry point: declared, listed, exported; the argument checks that need
# no device
# ---------------------------------------------------------------------------
def test_async_entry_declared_listed_exported(zs):
    text = open(os.path.join(ROOT, "include", "zseek_hip.h")).read()
    assert re.search(r"ZSEEK_EXPORT\s+ssize_t\s+zsk_preadv_device_async\s*\(", text)
    assert "zsk_preadv_device_async" in zs.EXPORTED
    assert hasattr(zs.lib(), "zsk_preadv_device_async")
    out = subprocess.run(["nm", "-D", "--defined-only", zs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "zsk_preadv_device_async" and ln.split()[-2] == "T" for ln in out.splitlines())


def test_async_null_reader(zs):
    err = C.create_string_buffer(80)
    rg = np.zeros(2, zs.RANGE_DTYPE)
    rg["count"] = 4
    rg["result"] = 7
    assert zs.lib().zsk_preadv_device_async(None, None, rg.ctypes.data, 2, None, None, None, err) == -1
    assert err.value == b"invalid reader"
    assert rg["result"].tolist() == [7, 7]               # the array is const


def test_async_no_ranges(zs):
    with zs.Reader(golden_file("lz4_64k_direct"), 0) as r:
        err = C.create_string_buffer(80)
        assert zs.lib().zsk_preadv_device_async(r.handle, None, None, 0, None, None, None, err) == 0
        assert err.value == b""
