"""The builds from device-listed pieces where no GPU is needed
(zsk_lz4_build_image_pieces / zsk_zstd_build_image_pieces):

- the per-piece rule of libzseek_amd/csrc/image_pieces.h, through
  tests/native/image_pieces_shim.cpp, against a plain restatement: offsets are
  the running sum of the sizes, the first invalid piece is found, what follows
  it is refused, and the running offset and the flag chain across batches;
- zsk_*_pieces_bound covers the sum of the compressors' bounds plus the table
  for any list, and stays within a stated slack of zsk_*_image_bound on
  fixed-frame lists;
- the new entries are declared, listed and exported, and refuse cleanly without
  a device."""
from __future__ import annotations

import ctypes as C
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, gpu_available

MIB = 1 << 20
S = [1, 7, 4096, 65536, 65537, 3, 200_001]
NONE = 0xFFFFFFFF
NEW = ["zsk_lz4_pieces_bound", "zsk_zstd_pieces_bound", "zsk_lz4_build_image_pieces", "zsk_zstd_build_image_pieces"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = pathlib.Path(tmp_path_factory.mktemp("image_pieces")) / "libimage_pieces.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    os.path.join(ROOT, "tests", "native", "image_pieces_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.ipieces_valid.restype = C.c_int
    L.ipieces_valid.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64]
    L.ipieces_plan.restype = C.c_uint64
    L.ipieces_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.POINTER(C.c_int)]
    for fn in (L.ipieces_lz4_bound, L.ipieces_zstd_bound):
        fn.restype = C.c_uint64
        fn.argtypes = [C.c_uint64, C.c_uint64, C.c_int]
    L.ipieces_code.restype = C.c_int64
    L.ipieces_code.argtypes = [C.c_int]
    return L


def plan(shim, sizes, per, max_piece, src_len):
    """-> (src_off[n], size[n], first_bad per batch, final offset, final flag)"""
    z = np.asarray(sizes, np.uint32)
    n = z.size
    off, size = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    fb = np.zeros(max(1, -(-n // per)), np.uint32)
    bad = C.c_int(-1)
    end = shim.ipieces_plan(z.ctypes.data, n, per, max_piece, src_len, off.ctypes.data, size.ctypes.data,
                            fb.ctypes.data, C.byref(bad))
    return off, size, [int(x) for x in fb[: -(-n // per)]], int(end), bool(bad.value)


def restate(sizes, max_piece, src_len):
    """The rule in plain Python: (first invalid index or None, offsets)."""
    at, offs = 0, []
    for i, s in enumerate(sizes):
        if s == 0 or s > max_piece or at + s > src_len:
            return i, offs
        offs.append(at)
        at += s
    return None, offs


def check(shim, sizes, max_piece, src_len):
    want_bad, offs = restate(sizes, max_piece, src_len)
    for per in (len(sizes), 1, 2, 3):
        off, size, fb, end, bad = plan(shim, sizes, per, max_piece, src_len)
        k = len(sizes) if want_bad is None else want_bad
        assert [int(x) for x in off[:k]] == offs and [int(x) for x in size[:k]] == list(sizes[:k])
        # what follows the first invalid piece is the refused piece: nothing, at offset 0
        assert not off[k:].any() and not size[k:].any()
        assert bad == (want_bad is not None)
        assert end == sum(sizes[:k])
        for b, first in enumerate(fb):
            lo = b * per
            if want_bad is None or want_bad >= lo + per:
                assert first == NONE
            else:
                assert first == max(want_bad - lo, 0)    # (sticky: a later batch is refused from 0)
    return want_bad


def test_offsets_are_the_running_sum(shim):
    top = max(S)
    assert check(shim, S, top, sum(S)) is None                       # the edges: a size of exactly
    off, size, fb, end, bad = plan(shim, S, len(S), top, sum(S))     # max_piece, a sum of exactly src_len
    assert [int(x) for x in off] == [int(x) for x in np.concatenate(([0], np.cumsum(S)[:-1]))]
    assert end == sum(S) and not bad
    assert check(shim, S, top, sum(S) + 1000) is None                # a sum below src_len is valid
    assert check(shim, [4 * MIB] * 3, 4 * MIB, 12 * MIB) is None


def test_first_invalid_piece(shim):
    top = max(S)
    for at in (0, 3, len(S) - 1):
        z = list(S)
        z[at] = 0
        assert check(shim, z, top, sum(S)) == at
        z[at] = top + 1
        assert check(shim, z, top, sum(S) + top) == at
    assert check(shim, S, top, sum(S) - 1) == len(S) - 1             # the sum is src_len + 1
    assert check(shim, S, top - 1, sum(S)) == len(S) - 1
    assert check(shim, S, top, 0) == 0
    assert check(shim, [0xFFFFFFFF] * 5, 0xFFFFFFFF, (1 << 34) - 4) == 4
    rng = np.random.default_rng(11)
    for _ in range(200):
        z = [int(x) for x in rng.integers(0, 40, int(rng.integers(1, 30)))]
        check(shim, z, int(rng.integers(1, 45)), int(rng.integers(0, sum(z) + 10)))


def test_valid_edges(shim):
    v = shim.ipieces_valid
    assert v(1, 0, 1, 1) and not v(0, 0, 1, 1) and not v(2, 0, 1, 2) and not v(1, 1, 1, 1)
    assert v(100, 900, 100, 1000) and not v(100, 901, 100, 1000) and not v(101, 0, 100, 1000)
    assert not v(1, 2000, 100, 1000)                                 # an offset past the source
    assert v(0xFFFFFFFF, 1, 1 << 32, 1 << 32) and not v(0xFFFFFFFF, 2, 1 << 32, 1 << 32)
    assert shim.ipieces_code(0) == -1 and shim.ipieces_code(1) == -2


# -- the bounds -----------------------------------------------------------------------------
def lz4_slot(n: int) -> int:
    """ZSK_LZ4_COMPRESS_BOUND (include/zseek_hip.h)."""
    return (n + 4 * (n >> 16) + 24 + 15) & ~15


def zstd_slot(n: int) -> int:
    """ZSK_ZSTD_COMPRESS_BOUND."""
    return (9 + 3 * (((n + 131071) >> 17) if n else 1) + n + 4 + 15) & ~15


def bound_lists():
    rng = np.random.default_rng(2024)
    yield [1] * 1000
    yield [65535, 65536, 131071] * 5
    yield [131072] * 9
    yield [4 * MIB]
    yield S
    yield []
    for _ in range(300):
        n = int(rng.integers(1, 60))
        top = int(rng.choice([2, 300, 65537, 131073, 4 * MIB]))
        yield [int(x) for x in rng.integers(1, top + 1, n)]


def test_bounds_cover_any_list(zs, shim):
    count = 0
    for z in bound_lists():
        for ck in (False, True):
            table = 17 + (12 if ck else 8) * len(z)
            for slack in (0, 1, 70_000):                              # (sizes may sum to less than src_len)
                src_len = sum(z) + slack
                got = zs.lz4_pieces_bound(src_len, len(z), ck)
                assert got == shim.ipieces_lz4_bound(src_len, len(z), ck)
                assert got >= sum(lz4_slot(s) for s in z) + table, z
                got = zs.zstd_pieces_bound(src_len, len(z), ck)
                assert got == shim.ipieces_zstd_bound(src_len, len(z), ck)
                assert got >= sum(zstd_slot(s) for s in z) + table, z
        count += 1
    assert count > 300


@pytest.mark.parametrize("length,frame_size", [
    (0, 65536), (1, 65536), (65536, 65536), (65537, 65536), (3 * 65536 + 100, 65536), (200_000, 4096),
    (2 * MIB + 5, MIB), (4 * MIB + 1, 4 * MIB), (1 << 30, 65536), ((1 << 30) + 12345, MIB), (999_999, 1000), (7, 3)])
def test_bounds_on_fixed_frames(zs, length, frame_size):
    """On a fixed-frame list the bound exceeds zsk_*_image_bound by at most
    the rounding (under 16 bytes a piece) and one block word a piece."""
    n = -(-length // frame_size)
    for ck in (False, True):
        d = zs.lz4_pieces_bound(length, n, ck) - zs.lz4_image_bound(length, frame_size, ck)
        assert 0 <= d <= 19 * n
        d = zs.zstd_pieces_bound(length, n, ck) - zs.zstd_image_bound(length, frame_size, ck)
        assert 0 <= d <= 18 * n
    assert zs.lz4_pieces_bound(0, 0) == zs.zstd_pieces_bound(0, 0) == 17


# -- the interface --------------------------------------------------------------------------
def test_entries_declared_listed_exported(zs):
    text = open(os.path.join(ROOT, "include", "zseek_hip.h")).read()
    mapped = open(os.path.join(ROOT, "libzseek_amd", "csrc", "libzseek.map")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", zs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"ZSEEK_EXPORT\s+\w+\s+%s\s*\(" % name, text), name
        assert re.search(r"^\s*%s;" % name, mapped, re.M), name
        assert name in zs.EXPORTED and hasattr(zs.lib(), name)
        assert any(ln.split()[-1] == name and ln.split()[-2] == "T" for ln in out.splitlines()), name
    assert re.search(r"#define\s+ZSK_IMAGE_FAILED\s+\(-1\)", text)
    assert re.search(r"#define\s+ZSK_IMAGE_BAD_PIECES\s+\(-2\)", text)
    assert (zs.IMAGE_FAILED, zs.IMAGE_BAD_PIECES) == (-1, -2)
    import libzseek_amd
    for name in ("lz4_build_image_pieces", "zstd_build_image_pieces", "lz4_pieces_bound", "zstd_pieces_bound",
                 "IMAGE_FAILED", "IMAGE_BAD_PIECES"):
        assert hasattr(libzseek_amd, name)


def test_refusals_without_a_device(zs):
    """The argument checks come first, whatever the machine; then, with host
    memory for every pointer, the device check: no device at all where there is
    none."""
    L = zs.lib()
    err = C.create_string_buffer(zs.ERRBUF)
    src = np.zeros(100_000, np.uint8)
    sizes = np.array([50_000, 50_000], np.uint32)
    res = np.full(3, 77, np.int64)
    dst = np.full(zs.lz4_pieces_bound(src.size, 2) + 64, 0xA5, np.uint8)

    def lz4(**kw):
        a = {"src": src.ctypes.data, "n": src.size, "sizes": sizes.ctypes.data, "k": 2, "max_piece": 65536,
             "level": 0, "cap": dst.size, "res": res.ctypes.data, **kw}
        r = L.zsk_lz4_build_image_pieces(a["src"], a["n"], a["sizes"], a["k"], a["max_piece"], a["level"], 0, 0,
                                         dst.ctypes.data, a["cap"], a["res"], None, err)
        return r, err.value.decode()

    def zstd(**kw):
        a = {"sizes": sizes.ctypes.data, "k": 2, "max_piece": 65536, "res": res.ctypes.data, **kw}
        r = L.zsk_zstd_build_image_pieces(src.ctypes.data, src.size, a["sizes"], a["k"], a["max_piece"], 0, 0,
                                          dst.ctypes.data, dst.size, a["res"], None, err)
        return r, err.value.decode()

    for call in (lz4, zstd):
        assert call(res=None) == (-1, "build image: NULL result")
        assert call(max_piece=0) == (-1, "build image: invalid piece size")
        assert call(max_piece=4 * MIB + 1) == (-1, "build image: invalid piece size")
        assert call(k=(1 << 27) + 1) == (-1, "build image: Frame index is too large")
        assert call(sizes=None, k=3) == (-1, "build image: invalid piece count")
        assert call(sizes=None, k=1) == (-1, "build image: invalid piece count")
        r, text = call()
        assert r == -1
        if gpu_available():
            assert text in ("no HIP device available", "build image: not device memory of one device")
        else:
            assert text == "no HIP device available"
    assert lz4(level=3) == (-1, "build image: HC levels are not supported")
    assert (dst == 0xA5).all() and (res == 77).all()
