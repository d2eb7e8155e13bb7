"""Records tests/golden/zstd_enc_subset.json: the SHA-256 of the frames that the
subset entry of the zstd compressor's format layer (zenc_compress of
tests/native/zstd_enc_shim.cpp over libzseek_amd/csrc/zstd_enc_dev.h) writes
for a dozen inputs.  Run at the commit whose subset bytes are the record -- the
one before the full format was added -- and never again unless the subset is
changed on purpose:

    python tests/golden/make_zstd_enc_subset.py

tests/test_zstd_enc_full.py recomputes the hashes with the same shim against
the header as it is now: the subset's functions must give what they gave.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import pathlib
import subprocess
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
OUT = pathlib.Path(__file__).with_name("zstd_enc_subset.json")

WORDS = [b"the", b"frame", b"of", b"a", b"seekable", b"file", b"holds", b"its", b"bytes", b"and", b"table",
         b"offset", b"literal", b"match", b"sequence", b"block", b"wave", b"lane", b"kernel", b"stream", b"\n",
         b"compressed", b"size", b"checksum", b"reader", b"writer", b"is", b"in", b"to", b"0x1F", b"42", b"zstd"]


def _lcg(n: int, seed: int) -> np.ndarray:
    """n values of a 32-bit linear congruential generator (its high 16 bits)"""
    out = np.empty(n, np.uint32)
    x = seed & 0xFFFFFFFF
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = x >> 16
    return out


def text(n: int, seed: int) -> bytes:
    r = _lcg(n // 3 + 8, seed)
    return b" ".join(WORDS[int(v) % len(WORDS)] for v in r)[:n]


def high(n: int, seed: int) -> bytes:
    return (160 + _lcg(n, seed) % 64).astype(np.uint8).tobytes()


def periodic(n: int, seed: int) -> bytes:
    p = (_lcg(270, seed) % 256).astype(np.uint8).tobytes()
    return (p * (n // 270 + 1))[:n]


def inputs():
    """-> [(name, content, checksum flag)]"""
    zb = 1 << 17
    out = []
    for i, n in enumerate((0, 1, 255, 4096, zb + 1, 300 << 10)):
        out.append(("text_%d" % n, text(n, 11 + i), i & 1))
    for i, n in enumerate((4096, 300 << 10)):
        out.append(("high_%d" % n, high(n, 23 + i), 1 - (i & 1)))
    for i, n in enumerate((255, 4096, zb + 1, 300 << 10)):
        out.append(("periodic_%d" % n, periodic(n, 37 + i), i & 1))
    return out


def load_shim(so_dir) -> C.CDLL:
    so = pathlib.Path(so_dir) / "libzstd_enc_subset.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/zstd_enc_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.zenc_frame_bound.restype = C.c_uint64
    L.zenc_frame_bound.argtypes = [C.c_uint64]
    L.zenc_compress.restype = C.c_int64
    L.zenc_compress.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64]
    return L


def hashes(L) -> dict:
    rec = {}
    for name, content, ck in inputs():
        src = np.frombuffer(content, np.uint8) if content else np.zeros(1, np.uint8)
        cap = L.zenc_frame_bound(len(content))
        out = np.empty(cap, np.uint8)
        n = L.zenc_compress(src.ctypes.data, len(content), ck, out.ctypes.data, cap)
        assert 0 < n <= cap, (name, n)
        rec[name] = {"input_sha256": hashlib.sha256(content).hexdigest(), "checksum": ck, "size": int(n),
                     "sha256": hashlib.sha256(out[:n].tobytes()).hexdigest()}
    return rec


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        rec = hashes(load_shim(d))
    OUT.write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT, len(rec), "entries")
