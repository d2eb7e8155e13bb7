"""tests/native/zstd_census_shim.cpp for the tests of the zstd census: the plan
walk per seek-table entry, the census as its maxima, the bounds a
device-planned read derives from it (libzseek_amd/csrc/zstd_plan.h,
zstd_caps.h), on the CPU; and the crafted files both test files read."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess
import tempfile

import zstd_craft as zc

ROOT = pathlib.Path(__file__).resolve().parents[1]
SHIM = str(ROOT / "tests/native/zstd_census_shim.cpp")
FIELDS = ("frames", "max_items", "max_blocks", "max_sequences", "max_dsize", "max_csize")
# test_zstd_caps.py's list: accepted hand-built entries of many tiny blocks
NOFIT = ("b_1000_empty_raw", "b_1000_empty_then_seqs", "h_40frames", "h_40frames_skips")

_keep = []


def load(so_dir=None) -> C.CDLL:
    if so_dir is None:
        _keep.append(tempfile.TemporaryDirectory())
        so_dir = _keep[-1].name
    so = pathlib.Path(so_dir) / "libzstd_census.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so), SHIM],
                   check=True)
    L = C.CDLL(str(so))
    L.zcensus_bounds.restype = None
    L.zcensus_bounds.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
    L.zcensus_item_capacity.restype = C.c_uint64
    L.zcensus_item_capacity.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64]
    L.zcensus_bounds_default.restype = None
    L.zcensus_bounds_default.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p]
    L.zcensus_frame_plan.restype = None
    L.zcensus_frame_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def plan(L, entry: bytes):
    """(bound, blocks, sequences) of the entry, from a buffer of exactly its length"""
    buf = (C.c_uint8 * len(entry)).from_buffer_copy(entry) if entry else None
    out = (C.c_uint64 * 3)()
    L.zcensus_frame_plan(buf, len(entry), out)
    return int(out[0]), int(out[1]), int(out[2])


def seek_table(img: bytes):
    """(entries, decoded sizes) of a seekable file, from its footer"""
    assert img[-4:] == (0x8F92EAB1).to_bytes(4, "little")
    n, flags = int.from_bytes(img[-9:-5], "little"), img[-5]
    step = 12 if flags & 0x80 else 8
    at = len(img) - 9 - step * n
    entries, dsizes, c = [], [], 0
    for _ in range(n):
        cs, ds = int.from_bytes(img[at: at + 4], "little"), int.from_bytes(img[at + 4: at + 8], "little")
        entries.append(img[c: c + cs])
        dsizes.append(ds)
        c, at = c + cs, at + step
    return entries, dsizes


def census(L, img: bytes) -> dict:
    """zsk_zstd_census_t of the file: the maxima of the walk over its entries"""
    entries, dsizes = seek_table(img)
    plans = [plan(L, e) for e in entries]
    vals = (len(entries), max((p[0] for p in plans), default=0), max((p[1] for p in plans), default=0),
            max((p[2] for p in plans), default=0), max(dsizes, default=0), max(map(len, entries), default=0))
    return dict(zip(FIELDS, vals))


def bounds(L, max_frames: int, cen: dict):
    """(out_bytes, max_blocks, max_sequences) of zstd_census_bounds"""
    out = (C.c_uint64 * 3)()
    L.zcensus_bounds(max_frames, cen["max_blocks"], cen["max_sequences"], cen["max_dsize"], out)
    return int(out[0]), int(out[1]), int(out[2])


def defaults(L, nframes: int, out_bytes: int):
    """(max_blocks, max_sequences) of zstd_bounds_default"""
    out = (C.c_uint64 * 2)()
    L.zcensus_bounds_default(nframes, out_bytes, out)
    return int(out[0]), int(out[1])


def nofit_file():
    """(image, payload): the NOFIT entries, twice over, as a seekable file"""
    cases = [zc.CASE[n] for n in NOFIT] * 2
    return zc.seekable([c[1] for c in cases], [c[2] for c in cases]), b"".join(c[3] for c in cases)


def random_file(seed: int = 77, n: int = 48):
    """(image, payload): zstd_craft.random_valid entries as a seekable file"""
    ents = zc.random_valid(seed, n)
    return zc.seekable([e for e, _ in ents], [len(x) for _, x in ents]), b"".join(x for _, x in ents)
