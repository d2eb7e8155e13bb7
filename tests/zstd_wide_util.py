"""What tests/test_zstd_enc_wide.py, tests/test_gpu_zstd_compress_wide.py and
tests/golden/make_zstd_enc_wide.py share: the CPU shim of the wide match search
(tests/native/zstd_enc_wide_shim.cpp, which holds the full and the subset
entries too) and the inputs at its edges."""
from __future__ import annotations

import ctypes as C
import hashlib
import pathlib
import subprocess

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
ZB = 1 << 17            # kZBlock
WIDE_MIN = 1 << 14      # kWideMinFrame: frames above it take the wide search
EDGE_LENGTHS = (0, 1, WIDE_MIN, WIDE_MIN + 1, ZB - 1, ZB, ZB + 1, 2 * ZB + 5, 1 << 22)


def load_shim(so_dir) -> C.CDLL:
    so = pathlib.Path(so_dir) / "libzstd_enc_wide.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/zstd_enc_wide_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    for fn in (L.zenc_zblock, L.zenc_wide_min_frame, L.zenc_wide_hash_log):
        fn.restype = C.c_uint32
    L.zenc_frame_bound.restype = C.c_uint64
    L.zenc_frame_bound.argtypes = [C.c_uint64]
    for fn in (L.zenc_compress, L.zenc_full_compress, L.zenc_wide_compress):
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64]
    L.zenc_wide_sequences.restype = C.c_uint32
    L.zenc_wide_sequences.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.zenc_full_frame.restype = C.c_int64
    L.zenc_full_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64,
                                  C.c_void_p]
    return L


def _src(content) -> np.ndarray:
    a = np.frombuffer(content, np.uint8) if isinstance(content, (bytes, bytearray)) else np.ascontiguousarray(content)
    return a if a.size else np.zeros(1, np.uint8)


def compress(L, content, checksum=0, how="wide") -> bytes:
    """content (bytes or a uint8 array) through zenc_wide_compress ("full", "subset": the others)."""
    n = len(content)
    src = _src(content)
    cap = L.zenc_frame_bound(n)
    out = np.empty(cap, np.uint8)
    fn = {"wide": L.zenc_wide_compress, "full": L.zenc_full_compress, "subset": L.zenc_compress}[how]
    r = fn(src.ctypes.data, n, int(checksum), out.ctypes.data, cap)
    assert 0 < r <= cap, (how, n, r)
    return out[:r].tobytes()


def sequences(L, content):
    """-> per block the (ll, ml, off) triples the wide search finds."""
    n = len(content)
    src = _src(content)
    nseq = np.zeros(max(1, -(-n // ZB)), np.uint32)
    total = L.zenc_wide_sequences(src.ctypes.data, n, None, nseq.ctypes.data)
    seq3 = np.zeros((max(total, 1), 3), np.uint32)
    assert L.zenc_wide_sequences(src.ctypes.data, n, seq3.ctypes.data, nseq.ctypes.data) == total
    cuts = np.cumsum(np.concatenate(([0], nseq)))
    return [[tuple(int(x) for x in t) for t in seq3[a:b]] for a, b in zip(cuts, cuts[1:])]


def offset_values(L, content, per):
    """The frame of `per` (sequences(...)) through zenc_full_frame -> (frame, per block the offset
    values chosen), as test_zstd_enc_full.py's full_frame."""
    n = len(content)
    src = _src(content)
    flat = [t for blk in per for t in blk]
    seq3 = np.ascontiguousarray(flat, np.uint32).reshape(-1, 3)
    nseq = np.ascontiguousarray([len(blk) for blk in per], np.uint32)
    cap = L.zenc_frame_bound(n)
    out = np.empty(cap, np.uint8)
    ofv = np.zeros(max(len(flat), 1), np.uint32)
    r = L.zenc_full_frame(src.ctypes.data, n, seq3.ctypes.data if flat else None, nseq.ctypes.data, 0,
                          out.ctypes.data, cap, ofv.ctypes.data)
    assert 0 < r <= cap, r
    cuts = np.cumsum([0] + [len(blk) for blk in per])
    return out[:r].tobytes(), [ofv[a:b].tolist() for a, b in zip(cuts, cuts[1:])]


def noise(n: int, seed: int) -> np.ndarray:
    """n bytes that no compressor shortens: SHA-256 in counter mode, the same on every machine."""
    out = bytearray()
    i = 0
    while len(out) < n:
        out += hashlib.sha256(b"zstd_enc_wide %d %d" % (seed, i)).digest()
        i += 1
    return np.frombuffer(bytes(out[:n]), np.uint8).copy()


def edge_inputs(oracle):
    """-> [(name, content array, checksum flag)]: every edge length as text-like data
    (oracle.synth), as noise and as the text with every byte's top bit flipped."""
    text = oracle.synth((1 << 22) + 4096, 5)
    rnd = noise(1 << 22, 6)
    out = []
    for i, n in enumerate(EDGE_LENGTHS):
        at = 1 + (i * 977) % 4096                    # (not the same prefix every time)
        out.append(("text_%d" % n, text[at: at + n].copy(), i & 1))
        out.append(("noise_%d" % n, rnd[:n].copy(), 1 - (i & 1)))
        out.append(("xor80_%d" % n, text[at: at + n] ^ np.uint8(0x80), i & 1))
    return out


STRADDLE_LEN, STRADDLE_AT = 1000, ZB - 500         # case b: the source's length and where it starts


def cross_block_inputs():
    """The cross-block contents -> {name: content array}.
      a  block 1 is a copy of block 0, 128 KiB of noise
      b  1000 bytes of noise that lie across the boundary of blocks 0 and 1, again in block 2; the
         rest of block 1 is a 7-byte pattern, one long match whose positions do not enter the table
      c  noise in block 0, 30 blocks of one repeated byte, block 0 again as block 31 (4 MiB)
      d  H H | one repeated byte | G G | H and 77 bytes more of it: H and G half blocks of noise, so
         blocks 0 and 2 each end on a match at offset 64 KiB, and block 3 repeats block 0"""
    a0 = noise(ZB, 21)
    b = noise(2 * ZB + 300 + STRADDLE_LEN + 200, 22)
    b[ZB + 500: 2 * ZB] = np.resize(np.frombuffer(b"pattern", np.uint8), ZB - 500)
    b[2 * ZB + 300: 2 * ZB + 300 + STRADDLE_LEN] = b[STRADDLE_AT: STRADDLE_AT + STRADDLE_LEN]
    c0 = noise(ZB, 23)
    h, g = noise(ZB // 2, 24), noise(ZB // 2, 25)
    d = np.concatenate([h, h, np.full(ZB, 0x5A, np.uint8), g, g, h, h[:77]])
    return {"a": np.concatenate([a0, a0]), "b": b,
            "c": np.concatenate([c0, np.full(30 * ZB, 0x33, np.uint8), c0]), "d": d}
