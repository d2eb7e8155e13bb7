"""The writer's host XXH64 (libzseek_amd/csrc/xxh64_host.h, written from the
specification) against the oracle's: one-shot over every length around the
32-byte stripe and the 8- / 4- / 1-byte tail steps, and the streaming state
(the multi-worker zstd path hashes a frame over several writes) split at
every position."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def xs(tmp_path_factory):
    so = tmp_path_factory.mktemp("xxh64") / "libxxh64_shim.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/xxh64_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.xs_oneshot.restype = C.c_uint64
    L.xs_oneshot.argtypes = [C.c_char_p, C.c_size_t]
    L.xs_stream.restype = C.c_uint64
    L.xs_stream.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t]
    return L


def _stream(xs, b: bytes, cuts) -> int:
    arr = (C.c_size_t * max(len(cuts), 1))(*cuts)
    return xs.xs_stream(b, len(b), arr, len(cuts))


def test_oneshot_matches_oracle(xs, oracle):
    rng = np.random.default_rng(11)
    for n in list(range(0, 201)) + [4095, 65536, 65537]:
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert xs.xs_oneshot(b, n) == oracle.xxh64(b), n


def test_empty_input_known_answer(xs):
    assert xs.xs_oneshot(b"", 0) == 0xEF46DB3751D8E999


def test_streaming_split_everywhere(xs, oracle):
    b = np.random.default_rng(12).integers(0, 256, 300, dtype=np.uint8).tobytes()
    want = oracle.xxh64(b)
    for cut in range(0, 301):
        assert _stream(xs, b, [cut]) == want, cut
    assert _stream(xs, b, [1] * 300) == want
    # updates that straddle, fill and leave a partial stripe
    assert _stream(xs, b, [31, 1, 32, 33, 64, 7]) == want
