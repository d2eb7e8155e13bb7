"""The lean LZ4 parse's ring arithmetic on the CPU: libzseek_amd/csrc/lean_ring.h
-- the text lz4_lean.hip's kernels compile -- through
tests/native/lean_ring_shim.cpp, for ring lengths 256 (a power of two: masks),
288 and 320 (one add and one conditional subtract).

Exhaustive, inside the shim: every start position (the three unwrapped ones
the chain may hold included) times every advance up to the fast step's
longest, 273 + 3, against `%`; a coordinate's position after a jump against
`%`; every 4-byte read inside every window of R stream bytes against a plain
byte-array ring with its 16-byte mirror; and slots of one to four 32-byte
pieces placed from every 32-aligned coordinate over three laps, position
carried from piece to piece, bytes and mirror against the plain ring."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("lean_ring") / "liblean_ring.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/lean_ring_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.lean_ring_check.restype = C.c_int
    L.lean_ring_check.argtypes = [C.c_uint32, C.c_void_p]
    return L


@pytest.mark.parametrize("R", [256, 288, 320])
def test_ring_arithmetic(shim, R):
    out = (C.c_uint32 * 4)()
    line = shim.lean_ring_check(R, out)
    assert line == 0, f"lean_ring_shim.cpp:{line} failed with {list(out)}"


def test_unknown_length_is_refused(shim):
    out = (C.c_uint32 * 4)()
    assert shim.lean_ring_check(384, out) == -1
