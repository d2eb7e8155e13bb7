"""tests/native/zstd_caps_shim.cpp for the tests of the asynchronous zstd
decode: the plan walk with its sequence count, the item capacity and the
default bounds (libzseek_amd/csrc/zstd_plan.h, zstd_caps.h), on the CPU."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess
import tempfile

ROOT = pathlib.Path(__file__).resolve().parents[1]
SHIM = str(ROOT / "tests/native/zstd_caps_shim.cpp")

_keep = []


def load(so_dir=None) -> C.CDLL:
    if so_dir is None:
        _keep.append(tempfile.TemporaryDirectory())
        so_dir = _keep[-1].name
    so = pathlib.Path(so_dir) / "libzstd_caps.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so), SHIM],
                   check=True)
    L = C.CDLL(str(so))
    L.zcaps_item_capacity.restype = C.c_uint64
    L.zcaps_item_capacity.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64]
    L.zcaps_bounds_default.restype = None
    L.zcaps_bounds_default.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p]
    L.zcaps_frame_plan.restype = None
    L.zcaps_frame_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def plan(L, entry: bytes):
    """(bound, blocks, cks, sequences) of the entry, from a buffer of exactly its length"""
    buf = (C.c_uint8 * len(entry)).from_buffer_copy(entry) if entry else None
    out = (C.c_uint64 * 4)()
    L.zcaps_frame_plan(buf, len(entry), out)
    return int(out[0]), int(out[1]), bool(out[2]), int(out[3])


def totals(L, entries):
    """(item bounds, blocks, sequences) of a batch, summed"""
    p = [plan(L, e) for e in entries]
    return sum(x[0] for x in p), sum(x[1] for x in p), sum(x[3] for x in p)


def defaults(L, nframes: int, out_bytes: int):
    """(max_blocks, max_sequences) of zstd_bounds_default"""
    out = (C.c_uint64 * 2)()
    L.zcaps_bounds_default(nframes, out_bytes, out)
    return int(out[0]), int(out[1])


def fits(L, entries, out_bytes: int, max_blocks: int, max_sequences: int) -> bool:
    """the device's fit check for entries packed back to back into out_bytes"""
    items, blocks, _ = totals(L, entries)
    return blocks <= max_blocks and items <= L.zcaps_item_capacity(len(entries), max_blocks, max_sequences)


def exact_bounds(L, entries, dsizes) -> dict:
    """the tightest bounds the batch decodes with (zstd_decode_frames_async's dict)"""
    _, blocks, seqs = totals(L, entries)
    return {"out_bytes": int(sum(dsizes)), "max_blocks": blocks, "max_sequences": seqs}
