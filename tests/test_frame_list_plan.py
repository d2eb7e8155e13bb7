"""The device plan of zsk_read_frames_indirect, on the CPU:
libzseek_amd/csrc/frame_list_plan.h's shared functions driven the way the
kernels of frame_list_plan.hip drive them -- a thread per slot, the scan
workgroup's 1,024 shares -- against the call's arithmetic written out in numpy
here (sizes, their scan, the region rules, the span).  Plus the entry point's
declaration / export and the refusals that need no device."""
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
D_OFF = [i * F for i in range(33)]   # 32 frames of 64 KiB
# a zero-size frame (frame 3) among 64 KiB frames
D_ZERO = [0, F, 2 * F, 3 * F, 3 * F, 4 * F, 5 * F, 6 * F]
# 200 frames of 4 KiB with two zero-size ones
K = 4096
D_LONG = np.cumsum([0] + [0 if i in (70, 150) else K for i in range(200)]).tolist()
LAYOUTS = {"D_OFF": D_OFF, "D_ZERO": D_ZERO, "D_LONG": D_LONG}
BIAS = 130                           # the image's offset from its 256-aligned base
SPAN = -3
SPAN_LIMIT = 0x7FFFFF00
BUF = 2**63                          # a destination buffer nothing here ends outside of
ST_NOT_RUN = 0x7FFF
NIDX = [0, 1, 2, 1023, 1024, 1025, 3077]   # shares of the scan with and without a remainder


@pytest.fixture(scope="module")
def fl(tmp_path_factory):
    so = tmp_path_factory.mktemp("frame_list_plan") / "libframe_list_plan.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/frame_list_plan_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.fl_run.restype = C.c_void_p
    L.fl_run.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                         C.c_size_t, C.c_uint64]
    L.fl_free.restype = None
    L.fl_free.argtypes = [C.c_void_p]
    L.fl_get.restype = None
    L.fl_get.argtypes = [C.c_void_p] * 7
    L.fl_results.restype = None
    L.fl_results.argtypes = [C.c_void_p] * 3
    L.fl_layout.restype = None
    L.fl_layout.argtypes = [C.c_uint64, C.c_int, C.c_void_p]
    L.fl_span_limit.restype = C.c_uint64
    L.fl_span_limit.argtypes = []
    return L


def _c_off(d_off):
    """Compressed prefix sums of a layout: frame f takes 100 + 7 f bytes (15 when it decodes to nothing)."""
    sizes = [(100 + 7 * f) if d_off[f + 1] > d_off[f] else 15 for f in range(len(d_off) - 1)]
    return np.cumsum([0] + sizes).tolist()


class Model:
    """The call's arithmetic (the issue's rules) in numpy: what d_offsets, the
    descriptors, the checksum words and d_result must be."""

    def __init__(self, idx, d_off, c_off, stride, buf_size, ck):
        idx = np.asarray(idx, np.int64)
        n, nframes = len(idx), len(d_off) - 1
        d, c = np.asarray(d_off, np.uint64), np.asarray(c_off, np.uint64)
        valid = (idx >= 0) & (idx < nframes)
        f = np.where(valid, idx, 0)
        size = np.where(valid, (d[f + 1] - d[f]).astype(np.int64), 0)
        packed = np.concatenate([[0], np.cumsum(size)]).astype(np.uint64)
        self.total = int(packed[-1])
        self.off = packed.tolist()
        if stride:
            self.offsets = [i * stride for i in range(n + 1)]
        else:
            self.offsets = self.off
        touched = valid & (size > 0)
        if touched.any():
            self.c_lo = int(c[f[touched]].min())
            self.span = int(c[f[touched] + 1].max()) - self.c_lo
        else:
            self.c_lo = self.span = 0
        self.flag = SPAN if self.span >= SPAN_LIMIT else 0
        self.want, self.desc, self.ck = [], [], []
        pad = [(0 if self.flag else self.c_lo) + BIAS, 0, 0, 0]
        for i in range(n):
            s, at = int(size[i]), self.offsets[i]
            if not valid[i] or self.flag:
                w = -1
            elif s == 0:
                w = 0
            elif at + s > buf_size or (stride and s > stride):
                w = -1
            else:
                w = s
            self.want.append(w)
            fi = int(f[i])
            self.desc.append([int(c[fi]) + BIAS, at, int(c[fi + 1] - c[fi]), s] if w > 0 else pad)
            self.ck.append((1000 + fi if w > 0 else 0) if ck else None)

    def results(self, status):
        res = [w if w <= 0 or status[i] == 0 else -1 for i, w in enumerate(self.want)]
        return res + [self.flag if self.flag else sum(r >= 0 for r in res)]


class Run:
    """The lanes' plan for an index list."""

    def __init__(self, fl, idx, d_off, stride=0, buf_size=BUF, c_off=None, ck=False):
        self.fl, self.n = fl, len(idx)
        n = self.n
        self.idx = np.ascontiguousarray(idx, np.int64)
        keep = self.idx.copy()
        nframes = len(d_off) - 1
        d = np.ascontiguousarray(d_off, np.uint64)
        c = np.ascontiguousarray(c_off if c_off is not None else _c_off(d_off), np.uint64)
        cks = np.arange(1000, 1000 + nframes, dtype=np.uint32) if ck else None
        self.h = fl.fl_run(self.idx.ctypes.data, n, stride, buf_size, c.ctypes.data, d.ctypes.data,
                           cks.ctypes.data if ck else None, nframes, BIAS)
        assert (self.idx == keep).all()                      # the list is const
        head, off, offsets = np.zeros(4, np.int64), np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        want, desc, ckw = np.zeros(n, np.int64), np.zeros((n, 4), np.uint64), np.zeros(n, np.uint32)
        fl.fl_get(self.h, head.ctypes.data, off.ctypes.data, offsets.ctypes.data, want.ctypes.data,
                  desc.ctypes.data, ckw.ctypes.data if ck else None)
        self.total, self.c_lo, self.span, self.flag = head.tolist()
        self.off, self.offsets, self.want = off.tolist(), offsets.tolist(), want.tolist()
        self.desc = desc.tolist()
        self.ck = ckw.tolist() if ck else [None] * n
        self.model = Model(idx, d_off, c.tolist(), stride, buf_size, ck)

    def check(self):
        m = self.model
        assert (self.total, self.c_lo, self.span, self.flag) == (m.total, m.c_lo, m.span, m.flag)
        assert self.off == m.off
        assert self.offsets == m.offsets
        assert self.want == m.want
        assert self.desc == m.desc
        assert self.ck == m.ck
        return self

    def results(self, status):
        st = np.ascontiguousarray(status, np.int32)
        assert len(st) == self.n
        res = np.full(self.n + 1, 12345, np.int64)
        self.fl.fl_results(self.h, st.ctypes.data, res.ctypes.data)
        assert res.tolist() == self.model.results(list(status))
        return res.tolist()

    def close(self):
        self.fl.fl_free(self.h)


def _lists(n, nframes, rng):
    """Ascending, reversed and shuffled lists of n slots over the file's frames, and one of a single index."""
    asc = [i % nframes for i in range(n)]
    asc.sort()
    return {"ascending": asc, "reversed": asc[::-1], "shuffled": rng.permutation(asc).tolist(),
            "same": [nframes // 2] * n}


def _statuses(n, rng):
    yield [0] * n
    yield [ST_NOT_RUN] * n
    yield np.where(rng.random(n) < 0.3, 17, 0).tolist()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", NIDX)
def test_plan_matches_model(fl, layout, n):
    d_off = LAYOUTS[layout]
    nframes = len(d_off) - 1
    rng = np.random.default_rng(n + 1)
    size = max(b - a for a, b in zip(d_off, d_off[1:]))
    for order, idx in _lists(n, nframes, rng).items():
        for stride, ck in ((0, False), (0, True), (size, True), (size + 1, False)):
            run = Run(fl, idx, d_off, stride=stride, ck=ck).check()
            assert run.flag == 0
            if not stride:                                    # every valid slot fits the endless buffer
                sizes = [d_off[f + 1] - d_off[f] for f in idx]
                assert run.want == sizes and run.offsets == np.cumsum([0] + sizes).tolist(), order
            for st in _statuses(n, rng):
                run.results(st)
            run.close()


def test_empty_list(fl):
    run = Run(fl, [], D_OFF).check()
    assert run.offsets == [0] and run.results([]) == [0]
    run.close()
    run = Run(fl, [], D_OFF, stride=100).check()
    assert run.offsets == [0] and run.results([]) == [0]
    run.close()


def test_delivered_sizes_and_count(fl):
    idx = [5, 3, 3, 0, 6]                                    # frame 3 of D_ZERO decodes to nothing
    run = Run(fl, idx, D_ZERO, ck=True).check()
    assert run.want == [F, 0, 0, F, F] and run.offsets == [0, F, F, F, 2 * F, 3 * F]
    assert run.results([0] * 5) == [F, 0, 0, F, F, 5]
    assert run.results([0, 9, 9, 9, 0]) == [F, 0, 0, -1, F, 4]   # an empty frame's status is never looked at
    # an empty frame is delivered wherever its offset lies; its descriptor is padding
    assert run.desc[1] == run.desc[2] == [min(_c_off(D_ZERO)[f] for f in (5, 0, 6)) + BIAS, 0, 0, 0]
    run.close()
    run = Run(fl, idx, D_ZERO, buf_size=0).check()
    assert run.results([0] * 5) == [-1, 0, 0, -1, -1, 2] and run.offsets[-1] == 3 * F
    run.close()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_invalid_indices(fl, layout):
    d_off = LAYOUTS[layout]
    nframes = len(d_off) - 1
    bad = [-1, nframes, 2**40, -2**63]
    idx = [0, bad[0], 1, bad[1], bad[2], nframes - 1, bad[3], 2]
    for stride in (0, F):
        run = Run(fl, idx, d_off, stride=stride, ck=True).check()
        res = run.results([0] * len(idx))
        assert [res[i] for i in (1, 3, 4, 6)] == [-1] * 4 and res[-1] == 4
        if not stride:                                        # an invalid slot takes no room
            assert run.offsets[2] == run.offsets[1] and run.offsets[5] == run.offsets[3]
        run.close()
    run = Run(fl, bad * 300, d_off).check()                   # nothing valid at all: nothing touched
    assert (run.total, run.c_lo, run.span, run.flag) == (0, 0, 0, 0)
    assert run.results([ST_NOT_RUN] * 1200) == [-1] * 1200 + [0]
    assert all(dd == [BIAS, 0, 0, 0] for dd in run.desc)
    run.close()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_buffer_cut_at_every_slot_boundary(fl, layout):
    d_off = LAYOUTS[layout]
    nframes = len(d_off) - 1
    rng = np.random.default_rng(11)
    idx = rng.permutation([i % nframes for i in range(37)] + [-1, nframes]).tolist()
    full = Run(fl, idx, d_off).check()
    offs = full.offsets
    full.close()
    for b in sorted(set(offs)):
        for buf_size in (b - 1, b, b + 1):
            if buf_size < 0:
                continue
            run = Run(fl, idx, d_off, buf_size=buf_size, ck=True).check()
            assert run.offsets == offs                        # the total whatever buf_size is
            for i, w in enumerate(run.want):                  # delivered exactly when the region is inside
                s = offs[i + 1] - offs[i]
                assert (w == s and (s == 0 or offs[i + 1] <= buf_size)) or (w == -1 and (
                    not 0 <= idx[i] < nframes or offs[i + 1] > buf_size)), (buf_size, i)
                assert w <= 0 or run.desc[i][1] + run.desc[i][3] <= buf_size
            run.results([0] * len(idx))
            run.close()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_strides(fl, layout):
    d_off = LAYOUTS[layout]
    nframes = len(d_off) - 1
    size = max(b - a for a, b in zip(d_off, d_off[1:]))
    rng = np.random.default_rng(5)
    idx = rng.permutation([i % nframes for i in range(70)] + [nframes + 7]).tolist()
    n = len(idx)
    for stride in (1, size - 1, size, size + 1, 3 * size):
        for buf_size in (n * stride, n * stride - 1, (n - 1) * stride + size - 1, 5 * stride):
            run = Run(fl, idx, d_off, stride=stride, buf_size=buf_size, ck=True).check()
            assert run.offsets == [i * stride for i in range(n + 1)]
            for i, w in enumerate(run.want):
                if w > 0:                                     # inside its row and inside the buffer
                    assert w <= stride and run.desc[i][1] == i * stride and i * stride + w <= buf_size
            if stride < size:                                 # a frame is never truncated to its row
                assert all(w <= 0 for w in run.want)
            run.results([0] * n)
            run.close()


def test_span_flag(fl):
    """Frames 2 GiB apart in the image: refused for a list that touches both
    ends, fine one byte under the limit and for lists that stay on one side."""
    assert fl.fl_span_limit() == SPAN_LIMIT
    d_off = [i * F for i in range(9)]
    d_off[6] = d_off[5]                                       # frame 5 decodes to nothing
    sizes = [1000, 1000, 1000, SPAN_LIMIT - 3001, 1, 1000, 1000, 1000]
    c_off = np.cumsum([0] + sizes).tolist()
    run = Run(fl, [3, 0, 2], d_off, c_off=c_off, ck=True).check()      # frames 0 .. 3: one byte under
    assert run.flag == 0 and run.span == SPAN_LIMIT - 1
    run.results([0, 0, 0])
    run.close()
    for stride in (0, F):
        run = Run(fl, [4, 2, 0, 5, -1], d_off, c_off=c_off, stride=stride, ck=True).check()   # frames 0 .. 4: exactly the limit
        assert run.flag == SPAN and run.span == SPAN_LIMIT
        assert all(dd == [BIAS, 0, 0, 0] for dd in run.desc) and run.ck == [0] * 5
        assert run.results([ST_NOT_RUN] * 5) == [-1] * 5 + [SPAN]
        assert run.offsets[-1] == (5 * F if stride else 3 * F)                                # d_offsets as always
        run.close()
    # an empty or invalid slot touches nothing: frame 5 (empty) beyond the limit does not count
    run = Run(fl, [0, 5, 9, 1], d_off, c_off=c_off).check()
    assert run.flag == 0 and run.span == 2000
    run.close()
    # a slot that does not fit the buffer still counts (the span is taken before the fit is known)
    run = Run(fl, [0, 4], d_off, c_off=c_off, buf_size=F).check()
    assert run.flag == SPAN
    run.close()
    run = Run(fl, [7, 4, 6], d_off, c_off=c_off).check()               # beyond 2 GiB into the image, but close together
    assert run.flag == 0 and run.c_lo == c_off[4] and run.desc[1][0] == c_off[4] + BIAS
    run.close()


def test_layout_is_aligned_and_disjoint(fl):
    for n in (1, 2, 3, 1025):
        for ck in (0, 1):
            out = np.zeros(6, np.uint64)
            fl.fl_layout(n, ck, out.ctypes.data)
            head, off, want, desc, ckw, total = out.tolist()
            assert all(v % 16 == 0 for v in out.tolist())
            assert head == 0 and off >= 32 and want >= off + 8 * (n + 1) and desc >= want + 8 * n
            assert ckw >= desc + 24 * n and total >= ckw + (4 * n if ck else 0)


# ---------------------------------------------------------------------------
# the entry point: declared, listed, exported; the refusals that need no device
# ---------------------------------------------------------------------------
def test_entry_declared_listed_exported(zs):
    text = open(os.path.join(ROOT, "include", "zseek_hip.h")).read()
    m = re.search(r"ZSEEK_EXPORT\s+ssize_t\s+zsk_read_frames_indirect\s*\(([^;]*)\);", text)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zseek_reader_t *reader", "const int64_t *d_idx", "size_t nidx", "size_t stride", "void *d_buf",
                    "size_t buf_size", "uint64_t *d_offsets", "int64_t *d_result", "void *stream",
                    "char errbuf[ZSEEK_ERRBUF_SIZE]"]
    assert "decoded once per occurrence" in text              # the header says what duplicates cost
    assert "zsk_read_frames_indirect" in zs.EXPORTED
    assert hasattr(zs.lib(), "zsk_read_frames_indirect")
    assert hasattr(zs.Reader, "read_frames_indirect") and hasattr(zs.Reader, "read_frames")
    vers = open(os.path.join(ROOT, "libzseek_amd", "csrc", "libzseek.map")).read()
    assert re.search(r"^\s*zsk_read_frames_indirect;", vers, re.M)
    out = subprocess.run(["nm", "-D", "--defined-only", zs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "zsk_read_frames_indirect" and ln.split()[-2] == "T" for ln in out.splitlines())


def test_null_reader(zs):
    err = C.create_string_buffer(80)
    assert zs.lib().zsk_read_frames_indirect(None, None, 2, 0, None, 0, None, None, None, err) == -1
    assert err.value == b"invalid reader"


def test_host_image_is_refused(zs):
    """A reader over a host file has no resident seek table: refused before
    any device is touched."""
    from conftest import golden_file
    with zs.Reader(golden_file("lz4_4k_direct")) as r:
        with pytest.raises(zs.ZseekError, match="frame-list read: needs a device image"):
            r.read_frames_indirect(0, 0, 0, 0, 0, 0)
        assert r.gpu_stats()["batches"] == 0
