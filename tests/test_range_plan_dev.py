"""The device plan of zsk_preadv_device_indirect, on the CPU:
libzseek_amd/csrc/range_plan_dev.h's shared functions driven the way the
kernels of range_plan_dev.hip drive them -- a thread per range, the compact
workgroup's 1,024 shares and scans -- against range_plan.h's plan_ranges,
range_result.h's build_range_table and range_plan.h's range_results, which are
the yardstick (the host-planned call's arithmetic).  Plus the new entry point's
declaration / export and the argument check that needs no device."""
from __future__ import annotations

import ctypes as C
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
F = 65536
D_OFF = [i * F for i in range(33)]   # test_range_plan.py's layout: 32 frames of 64 KiB
# a zero-size frame (frame 3) among 64 KiB frames
D_ZERO = [0, F, 2 * F, 3 * F, 3 * F, 4 * F, 5 * F, 6 * F]
# 200 frames of 4 KiB with two zero-size ones
K = 4096
D_LONG = np.cumsum([0] + [0 if i in (70, 150) else K for i in range(200)]).tolist()
LAYOUTS = {"D_OFF": D_OFF, "D_ZERO": D_ZERO, "D_LONG": D_LONG}
BIAS = 130                           # the image's offset from its 256-aligned base
OVERFLOW, SPAN = -2, -3
BUF = 2**64 - 1                      # a destination buffer nothing here ends outside of
ST_NOT_RUN = 0x7FFF


@pytest.fixture(scope="module")
def pd(tmp_path_factory):
    so = tmp_path_factory.mktemp("range_plan_dev") / "librange_plan_dev.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/range_plan_dev_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.pd_run.restype = C.c_void_p
    L.pd_run.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64,
                         C.c_uint64, C.c_uint64]
    L.ref_plan.restype = C.c_void_p
    L.ref_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    for fn in (L.pd_free, L.ref_free):
        fn.restype = None
        fn.argtypes = [C.c_void_p]
    for fn in (L.pd_seg_cap, L.ref_touched, L.ref_nsegs, L.ref_batches):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_void_p]
    for fn, k in ((L.pd_head, 2), (L.pd_rows, 2), (L.pd_frames, 2), (L.pd_segs, 2), (L.pd_results, 3), (L.ref_get, 5)):
        fn.restype = None
        fn.argtypes = [C.c_void_p] * k
    L.ref_results.restype = C.c_size_t
    L.ref_results.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return L


def _c_off(d_off):
    """Compressed prefix sums of a layout: frame f takes 100 + 7 f bytes (15 when it decodes to nothing)."""
    sizes = [(100 + 7 * f) if d_off[f + 1] > d_off[f] else 15 for f in range(len(d_off) - 1)]
    return np.cumsum([0] + sizes).tolist()


def _dst(ranges, gap=3):
    """(offset, count) -> (offset, count, dst_off): disjoint destinations in
    order, a few bytes apart.  (A count near 2^64 fits only a destination that
    covers nearly everything: it takes no room here -- the plan never looks at
    how destinations relate, that is the caller's contract.)"""
    out, at = [], 5
    for o, c in ranges:
        out.append((o, c, at))
        at += c + gap if c < 2**62 else 0
    return out, at


class Run:
    """The lanes' plan for (offset, count, dst_off) ranges."""

    def __init__(self, pd, ranges, d_off, max_frames, buf_size, c_off=None, ck=False):
        self.pd, self.ranges, self.n = pd, ranges, len(ranges)
        self.d_off_list = list(d_off)
        self.nframes = len(d_off) - 1
        self.d = np.ascontiguousarray(d_off, np.uint64)
        self.c = np.ascontiguousarray(c_off if c_off is not None else _c_off(d_off), np.uint64)
        self.ck = np.arange(1000, 1000 + self.nframes, dtype=np.uint32) if ck else None
        self.max_frames = max_frames
        rg4 = np.ascontiguousarray([(o, c, d, 424242) for o, c, d in ranges], np.uint64).reshape(-1, 4)
        self.h = pd.pd_run(rg4.ctypes.data, self.n, self.c.ctypes.data, self.d.ctypes.data,
                           self.ck.ctypes.data if ck else None, self.nframes, BIAS, buf_size, max_frames)
        assert (rg4[:, 3] == 424242).all()                   # the list is const
        head = np.zeros(4, np.int64)
        pd.pd_head(self.h, head.ctypes.data)
        self.touched, self.bytes, self.span, self.flag = head.tolist()
        assert pd.pd_seg_cap(self.h) == self.n               # one segment per range
        rows = np.zeros((self.n, 4), np.uint64)
        pd.pd_rows(self.h, rows.ctypes.data)
        self.rows = rows.astype(np.int64).tolist()
        fr = np.zeros((max_frames, 6), np.uint64)
        pd.pd_frames(self.h, fr.ctypes.data)
        self.frames = fr.tolist()                            # c_off, d_off, c_size, d_size, t_doff, ck
        sg = np.zeros((self.n, 4), np.uint64)
        pd.pd_segs(self.h, sg.ctypes.data)
        self.segs = sg.tolist()                              # src_off, dst_off, len, frame

    def results(self, status):
        st = np.ascontiguousarray(status, np.int32)
        assert len(st) == self.max_frames
        res = np.full(self.n + 1, 12345, np.int64)
        self.pd.pd_results(self.h, st.ctypes.data, res.ctypes.data)
        return res.tolist()

    def close(self):
        self.pd.pd_free(self.h)


class Ref:
    """The yardstick: plan_ranges (one batch), build_range_table, range_results."""

    def __init__(self, pd, ranges, d_off):
        self.pd = pd
        self.rg = np.ascontiguousarray(ranges, np.uint64).reshape(-1, 3)
        self.d = np.ascontiguousarray(d_off, np.uint64)
        self.args = (self.rg.ctypes.data, len(self.rg), self.d.ctypes.data, len(self.d) - 1)
        self.h = pd.ref_plan(*self.args)
        t, s = pd.ref_touched(self.h), pd.ref_nsegs(self.h)
        assert pd.ref_batches(self.h) <= 1
        frames, rows = np.zeros(t, np.uint64), np.zeros((len(self.rg), 4), np.uint64)
        t_doff, segs = np.zeros(t, np.uint64), np.zeros((s, 5), np.uint64)
        pd.ref_get(self.h, frames.ctypes.data, rows.ctypes.data, t_doff.ctypes.data, segs.ctypes.data)
        self.frames, self.t_doff = frames.tolist(), t_doff.tolist()
        self.rows = rows.astype(np.int64).tolist()
        self.segs = segs.tolist()                            # src_off, dst_off, len, frame, range

    def results(self, status):
        st = np.ascontiguousarray(status, np.int32)
        res = np.full(len(self.rg), 12345, np.int64)
        ok = self.pd.ref_results(self.h, *self.args, st.ctypes.data, res.ctypes.data)
        return res.tolist() + [ok]

    def close(self):
        self.pd.ref_free(self.h)


def _mixed(d_off):
    """Empty ranges, ranges at / past EOF, a count that wraps, duplicates,
    frame-boundary ends, spans (over a zero-size frame where the layout has
    one), the whole file."""
    size = d_off[-1]
    f = d_off[1] - d_off[0]
    rg = [(size - 1, 2**64 - size + 5),                # offset + count wraps (to 4): the range ends at EOF
          (5, 0), (size, 10), (size + 99, 10), (2**63, 100),
          (f + 7, 3 * f), (f + 7, 3 * f),              # a duplicate span
          (2 * f - 10, 10), (0, 2 * f),                # ending exactly at a frame boundary
          (2 * f + 5, 100), (size - f, f), (size - 3, 100),
          (d_off[-2] - 1, 2),                          # one byte each side of the last boundary
          (0, size)]
    return rg


def _compare(run: Run, ref: Ref):
    """A clean plan against the yardstick: the touched list, rows, packed
    offsets, checksum words, padding, and per range the segment set -- the
    yardstick's (range, frame) segments of a range, in frame order, are
    adjacent in the staging and in the destination, start at the range's first
    touched frame, and joined they are the range's one segment here."""
    assert run.flag == 0
    T = len(ref.frames)
    assert run.touched == T
    c, d = run.c.tolist(), run.d_off_list
    packed = np.cumsum([0] + [d[f + 1] - d[f] for f in ref.frames]).tolist()
    assert run.bytes == packed[-1]
    assert run.span == (c[ref.frames[-1] + 1] - c[ref.frames[0]] if T else 0)
    for t, f in enumerate(ref.frames):
        want_ck = 1000 + f if run.ck is not None else 0
        assert run.frames[t] == [c[f] + BIAS, packed[t], c[f + 1] - c[f], d[f + 1] - d[f], d[f], want_ck], (t, f)
    for t in range(T, run.max_frames):                    # padding: nothing to decode, c_off inside the checked span
        assert run.frames[t][:4] == [(c[ref.frames[0]] if T else 0) + BIAS, 0, 0, 0], t
    assert run.rows == ref.rows                           # offset, full, rt0, rtn
    assert ref.t_doff == [run.frames[t][4] for t in range(T)]
    for r, row in enumerate(run.rows):
        parts = sorted((s for s in ref.segs if s[4] == r), key=lambda s: s[3])
        seg = run.segs[r]
        if not parts:
            assert seg[2] == 0 and row[1] == 0
            continue
        assert parts[0][3] == row[2] == seg[3]            # gated by the range's first touched frame
        for a, b in zip(parts, parts[1:]):
            assert b[0] == a[0] + a[2] and b[1] == a[1] + a[2]
            assert b[3] > a[3]
        assert seg[:3] == [parts[0][0], parts[0][1], sum(s[2] for s in parts)] and seg[2] == row[1]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("ck", [False, True], ids=["plain", "checksums"])
def test_plan_matches_plan_ranges(pd, layout, ck):
    d_off = LAYOUTS[layout]
    ranges, end = _dst(_mixed(d_off))
    ref = Ref(pd, ranges, d_off)
    T = len(ref.frames)
    assert T == len(d_off) - 1                            # the whole-file range touches every frame
    run = Run(pd, ranges, d_off, T + 5, BUF, ck=ck)       # five padding descriptors
    _compare(run, ref)
    # results on status vectors: clean, one failure at every touched frame, tails never run
    pad = [ST_NOT_RUN] * 5                                # what padding frames report: never looked at
    for st in [[0] * T] + [[0] * k + [9] + [0] * (T - k - 1) for k in range(T)] + \
              [[0] * k + [ST_NOT_RUN] * (T - k) for k in (0, 1, T // 2)]:
        assert run.results(st + pad) == ref.results(st)
    size = d_off[-1]
    assert run.results([0] * T + pad)[:-1] == [0 if c == 0 or o >= size else min(c, size - o) for o, c, _ in ranges]
    run.close()
    ref.close()


def test_zero_size_frame_inside_a_range(pd):
    ranges, _ = _dst([(2 * F + 9, 2 * F), (3 * F, 1), (3 * F - 1, 1)])
    ref = Ref(pd, ranges, D_ZERO)
    assert ref.frames == [2, 3, 4, 5] and ref.rows[0][2:] == [0, 4]      # frame 3 (no bytes) is touched
    run = Run(pd, ranges, D_ZERO, 4, BUF)
    _compare(run, ref)
    assert run.frames[1][1:4] == [F, 15, 0] and run.frames[2][1] == F    # it takes no room in the staging
    assert run.segs[0] == [9, ranges[0][2], 2 * F, 0]
    assert run.rows[1][2:] == [2, 1] and run.rows[2][2:] == [0, 1]      # 3 F is frame 4's byte, not frame 3's
    run.close()
    ref.close()


def test_overlapping_ranges_never_run_out_of_segments(pd):
    """305 ranges over 200 frames, the whole file among them: (range, frame)
    segments would number several hundred more than nranges + max_frames; one
    per range always fits."""
    rng = np.random.default_rng(7)
    size = D_LONG[-1]
    rg = [(int(rng.integers(0, size)), int(rng.integers(1, 3 * K))) for _ in range(300)]
    rg += [(0, size), (D_LONG[70], 1), (D_LONG[150] - 1, 2), (D_LONG[64], 64 * K), (D_LONG[3] + 9, 129 * K)]
    ranges, _ = _dst([rg[i] for i in rng.permutation(len(rg))])
    ref = Ref(pd, ranges, D_LONG)
    assert len(ref.frames) == 200 and len(ref.segs) > len(ranges) + 200
    run = Run(pd, ranges, D_LONG, 200, BUF, ck=True)
    _compare(run, ref)
    for density in (0.0, 0.02, 0.3, 1.0):
        st = np.where(rng.random(200) < density, 17, 0).tolist()
        assert run.results(st) == ref.results(st)
    run.close()
    ref.close()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_max_frames_edge(pd, layout):
    d_off = LAYOUTS[layout]
    ranges, _ = _dst(_mixed(d_off)[:-1])                  # (without the whole-file range)
    ref = Ref(pd, ranges, d_off)
    T = len(ref.frames)
    assert 1 < T <= len(d_off) - 1
    run = Run(pd, ranges, d_off, T, BUF)                  # exactly T: clean, no padding
    _compare(run, ref)
    run.close()
    run = Run(pd, ranges, d_off, T - 1, BUF)              # one short
    assert (run.flag, run.touched) == (OVERFLOW, T)
    assert all(fr[:4] == [BIAS, 0, 0, 0] for fr in run.frames)           # nothing to decode
    assert all(s[2] == 0 for s in run.segs)                              # nothing to move
    assert all(r[3] == 0 for r in run.rows)                              # no status is looked at
    assert run.results([ST_NOT_RUN] * (T - 1)) == [-1] * len(ranges) + [OVERFLOW]
    run.close()
    ref.close()


def test_segment_capacity_edge(pd):
    """Every one of the nranges slots in use: n copies of a range over the
    same four frames (4 n (range, frame) overlaps) with max_frames 4."""
    for n in (1, 2, 64):
        ranges, _ = _dst([(F + 1, 3 * F)] * n)
        ref = Ref(pd, ranges, D_OFF)
        assert len(ref.segs) == 4 * n
        run = Run(pd, ranges, D_OFF, 4, BUF)
        _compare(run, ref)
        assert all(s[2] == 3 * F and s[0] == 1 and s[3] == 0 for s in run.segs)
        assert len({s[1] for s in run.segs}) == n
        run.close()
        ref.close()


def test_destination_bounds(pd):
    rg = [(10, 100), (F - 5, 10), (3 * F, 50), (7, 0)]
    ranges, end = _dst(rg)
    last = ranges[2]
    buf_size = last[2] + last[1]                          # the third range ends exactly at buf_size
    ranges[3] = (7, 0, buf_size + 999)                    # an empty range has no destination to check
    ref = Ref(pd, ranges, D_OFF)
    run = Run(pd, ranges, D_OFF, 8, buf_size)
    _compare(run, ref)
    assert run.results([0] * 8) == [100, 10, 50, 0, 4]
    run.close()
    ref.close()
    run = Run(pd, ranges, D_OFF, 8, buf_size - 1)         # ... and one byte past it
    assert run.flag == 0
    assert run.rows[2][2:] == [0, 0] and run.touched == 2  # it touches nothing
    assert all(s[2] == 0 or s[1] + s[2] <= buf_size - 1 for s in run.segs)
    assert [s[1:3] for s in run.segs] == [[ranges[0][2], 100], [ranges[1][2], 10], [0, 0], [0, 0]]
    assert run.results([0] * 8) == [100, 10, -1, 0, 3]
    assert run.results([0, 5, 0] + [0] * 5) == [100, 5, -1, 0, 2]
    run.close()
    # dst_off + count wraps; dst_off past the buffer; a range at EOF with a bad destination
    size = D_OFF[-1]
    ranges = [(0, 16, 2**64 - 8), (0, 4, buf_size + 1), (size + 5, 9, buf_size), (1, 1, buf_size - 1)]
    run = Run(pd, ranges, D_OFF, 2, buf_size)
    assert run.touched == 1 and [s[1:3] for s in run.segs if s[2]] == [[buf_size - 1, 1]]
    assert run.results([0, 0]) == [-1, -1, -1, 1, 1]
    run.close()


def test_span_flag(pd):
    """Frames 2 GiB apart in the image: refused for a read that touches both
    ends, fine for reads that stay on one side."""
    d_off = [i * F for i in range(9)]
    sizes = [1000, 1000, 1000, 0x7FFFFF00 - 3000, 1000, 1000, 1000, 1000]
    c_off = np.cumsum([0] + sizes).tolist()
    near, _ = _dst([(0, 10), (2 * F + 1, 10)])
    run = Run(pd, near, d_off, 4, BUF, c_off=c_off)
    assert run.flag == 0 and run.touched == 2 and run.span == 3000
    run.close()
    far, _ = _dst([(0, 10), (3 * F + 1, 10)])              # frames 0 .. 3: exactly the limit
    run = Run(pd, far, d_off, 4, BUF, c_off=c_off)
    assert run.flag == SPAN and run.span == 0x7FFFFF00
    assert all(fr[:4] == [BIAS, 0, 0, 0] for fr in run.frames) and all(s[2] == 0 for s in run.segs)
    assert run.results([ST_NOT_RUN] * 4) == [-1, -1, SPAN]
    run.close()
    far, _ = _dst([(F, 10), (3 * F + 1, 10)])              # frames 1 .. 3: 1000 bytes under it
    run = Run(pd, far, d_off, 4, BUF, c_off=c_off)
    assert run.flag == 0
    run.close()
    over, _ = _dst([(4 * F, 10), (7 * F + 1, 10)])         # beyond 2 GiB into the image, but close together
    run = Run(pd, over, d_off, 4, BUF, c_off=c_off)
    assert run.flag == 0 and run.frames[0][0] == c_off[4] + BIAS
    run.close()


def test_whole_words_and_word_edges(pd):
    """Runs that start / end on bitmap word edges (32 frames a word) and cover
    whole words, on 200 frames."""
    for a, b in [(0, 31), (0, 32), (31, 32), (32, 63), (31, 64), (5, 199), (0, 199), (64, 127), (63, 128), (199, 199)]:
        assert D_LONG[b + 1] > D_LONG[b] and D_LONG[a + 1] > D_LONG[a]
        ranges, _ = _dst([(D_LONG[a], D_LONG[b] + 1 - D_LONG[a]), (D_LONG[a] + 1, 1)])
        ref = Ref(pd, ranges, D_LONG)
        assert ref.frames == list(range(a, b + 1))
        run = Run(pd, ranges, D_LONG, b - a + 2, BUF)
        _compare(run, ref)
        run.close()
        ref.close()


# ---------------------------------------------------------------------------
# the entry point: declared, listed, exported; the argument check that needs
# no device
# ---------------------------------------------------------------------------
def test_indirect_entry_declared_listed_exported(zs):
    text = open(os.path.join(ROOT, "include", "zseek_hip.h")).read()
    assert re.search(r"ZSEEK_EXPORT\s+ssize_t\s+zsk_preadv_device_indirect\s*\(", text)
    assert re.search(r"#define\s+ZSK_PLAN_OVERFLOW\s+\(-2\)", text) and re.search(r"#define\s+ZSK_PLAN_SPAN\s+\(-3\)", text)
    assert (zs.PLAN_OVERFLOW, zs.PLAN_SPAN) == (OVERFLOW, SPAN)
    assert "zsk_preadv_device_indirect" in zs.EXPORTED
    assert hasattr(zs.lib(), "zsk_preadv_device_indirect")
    assert hasattr(zs.Reader, "preadv_device_indirect")
    out = subprocess.run(["nm", "-D", "--defined-only", zs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "zsk_preadv_device_indirect" and ln.split()[-2] == "T" for ln in out.splitlines())


def test_indirect_null_reader(zs):
    err = C.create_string_buffer(80)
    assert zs.lib().zsk_preadv_device_indirect(None, None, 0, None, 2, 4, None, None, err) == -1
    assert err.value == b"invalid reader"
