"""The layout of a batch's pinned upload (libzseek_amd/csrc/batch_layout.h),
on the CPU: the offsets reader.cpp's submit, reader_vec.cpp's submit_gather and
the pre-growing of an asynchronous call's slots all take from it, against the
expressions each of the three used to write out for itself, restated here."""
from __future__ import annotations

import ctypes as C
import itertools
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
DESC = 24      # sizeof(FrameDesc)
SEG = 24       # sizeof(GatherSeg)
COUNTS = (0, 1, 3)
CSIZES = (0, 1, 255, 256, 257, 65536 + 1)


@pytest.fixture(scope="module")
def bl(tmp_path_factory):
    so = tmp_path_factory.mktemp("batch_layout") / "libbatch_layout.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/batch_layout_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.bl_contiguous.restype = None
    L.bl_contiguous.argtypes = [C.c_uint64, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.bl_pack_at.restype = C.c_uint64
    L.bl_pack_at.argtypes = [C.c_uint64]
    L.bl_vectored.restype = None
    L.bl_vectored.argtypes = [C.c_uint64, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    return L


def _call(fn, *args):
    out = (C.c_uint64 * 5)()
    fn(*args, out)
    return dict(zip(("doff", "poff", "goff", "coff", "up"), out))


def _parent_doff(csz, image):
    return 0 if image else (csz + 256 + 255) & ~255


def _check_order(L, csz, image):
    # the compressed span and its 256 bytes of slack end before the descriptors
    # (an image: neither is uploaded); every region ends where the next starts
    # or before, none reaches past the upload's end
    if not image:
        assert csz + 256 <= L["doff"] < csz + 256 + 256
    assert L["doff"] % 256 == 0
    assert L["doff"] <= L["poff"] <= L["goff"] <= L["coff"] <= L["up"]


@pytest.mark.parametrize("image", [False, True])
@pytest.mark.parametrize("plan", [False, True])
def test_contiguous(bl, image, plan):
    for csz, n in itertools.product(CSIZES, COUNTS):
        L = _call(bl.bl_contiguous, csz, n, image, plan)
        # submit, before: doff; poff = doff + n * sizeof(FrameDesc);
        # up = poff + (zplan ? 16 * (n + 1) : 0)
        doff = _parent_doff(csz, image)
        poff = doff + n * DESC
        up = poff + (16 * (n + 1) if plan else 0)
        assert (L["doff"], L["poff"], L["up"]) == (doff, poff, up), (csz, n)
        # no segment regions
        assert L["goff"] == L["coff"] == L["up"]
        assert L["poff"] - L["doff"] == n * DESC
        assert L["up"] - L["poff"] == (16 * (n + 1) if plan else 0)
        _check_order(L, csz, image)


@pytest.mark.parametrize("image", [False, True])
@pytest.mark.parametrize("plan", [False, True])
def test_vectored(bl, image, plan):
    for csz, n, nseg in itertools.product(CSIZES, COUNTS, COUNTS):
        L = _call(bl.bl_vectored, csz, n, nseg, image, plan)
        # submit_gather, before: doff; poff = doff + n * sizeof(FrameDesc);
        # goff = poff + (zplan ? 16 * (n + 1) : 0);
        # coff = goff + nseg * sizeof(GatherSeg); up = coff + (nseg + 1) * 8
        doff = _parent_doff(csz, image)
        poff = doff + n * DESC
        goff = poff + (16 * (n + 1) if plan else 0)
        coff = goff + nseg * SEG
        up = coff + (nseg + 1) * 8
        assert L == dict(doff=doff, poff=poff, goff=goff, coff=coff, up=up), (csz, n, nseg)
        # each region holds exactly its items: no overlap, no gap
        assert L["poff"] - L["doff"] == n * DESC
        assert L["goff"] - L["poff"] == (16 * (n + 1) if plan else 0)
        assert L["coff"] - L["goff"] == nseg * SEG
        assert L["up"] - L["coff"] == (nseg + 1) * 8
        _check_order(L, csz, image)
        if not plan:
            # grow_idle_for_async, before (LZ4 alone, no plan): one sum
            assert L["up"] == doff + n * DESC + nseg * SEG + (nseg + 1) * 8


def test_pack_at(bl):
    """Where a vectored batch's compacted segments start in its decoded staging:
    submit_gather's pack_at, before."""
    for dsz in (0, 1, 255, 256, 257, 65536 + 1, (1 << 32) + 5):
        at = bl.bl_pack_at(dsz)
        assert at == (dsz + 255) & ~255
        assert dsz <= at < dsz + 256 and at % 256 == 0


def test_vectored_extends_contiguous(bl):
    """The two forms agree on everything before the segments."""
    for csz, n, image, plan in itertools.product(CSIZES, COUNTS, (0, 1), (0, 1)):
        a = _call(bl.bl_contiguous, csz, n, image, plan)
        b = _call(bl.bl_vectored, csz, n, 3, image, plan)
        assert (a["doff"], a["poff"], a["goff"]) == (b["doff"], b["poff"], b["goff"])
