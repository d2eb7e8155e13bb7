"""The zstd decoder's plan walk on the CPU: libzseek_amd/csrc/zstd_plan.h's
zstd_frame_plan, the one function that sizes an entry's item slots and block
slots for both the device plan (zstd_plan_kernel) and the host plan
(zstd_host_plan).  Inputs: every hand-built entry of tests/zstd_craft.py
(tests/golden/zstd_craft.json names the same table) and every corrupted frame
of tests/golden/zstd_x2.*.  For the entries the table accepts, the bound is
held to the builder's record of their frames and blocks (zstd_craft.RECORDS)
and to the item slots the replay fills (zstd_craft.items); every entry, whole
or cut short, must be
walked without a read past its end -- the last under AddressSanitizer, in a
stand-alone program built from the same shim."""
from __future__ import annotations

import ctypes as C
import json
import os
import pathlib
import struct
import subprocess

import pytest

import zstd_craft as zc
from conftest import GOLDEN

ROOT = pathlib.Path(__file__).resolve().parents[1]
SHIM = str(ROOT / "tests/native/zstd_plan_shim.cpp")
BOUND_MAX = (1 << 30) + (1 << 18)   # no entry here may be given more: the walk stops once past 2^30


def x2_entries():
    meta = json.load(open(os.path.join(GOLDEN, "zstd_x2.json")))
    blob = open(os.path.join(GOLDEN, "zstd_x2.bin"), "rb").read()
    out = [("x2_%d" % i, blob[c["off"]: c["off"] + c["len"]]) for i, c in enumerate(meta["cases"])]
    return out + [("x2_neighbour_%d" % i, bytes.fromhex(h)) for i, h in enumerate(meta["neighbour_frames_hex"])]


ENTRIES = [(c[0], c[1]) for c in zc.CASES] + x2_entries()


@pytest.fixture(scope="module")
def zp(tmp_path_factory):
    so = tmp_path_factory.mktemp("zstd_plan") / "libzstd_plan.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so), SHIM],
                   check=True)
    L = C.CDLL(str(so))
    L.zp_frame_plan.restype = None
    L.zp_frame_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def plan(zp, entry: bytes):
    """(bound, blocks, cks) of the entry, from a fresh buffer of exactly its length"""
    buf = (C.c_uint8 * len(entry)).from_buffer_copy(entry) if entry else None
    out = (C.c_uint32 * 3)()
    zp.zp_frame_plan(buf, len(entry), out)
    return out[0], out[1], bool(out[2])


def test_inputs():
    """every accepted entry has the builder's record, and the entries this
    walk is about are among them: skippable frames, concatenated frames,
    checksummed frames between others"""
    ok = [c[0] for c in zc.CASES if c[4] == 0]
    assert len(zc.CASES) == 578 and len(ENTRIES) == 578 + 42
    assert len(ok) == 451 and set(ok) == set(zc.RECORDS)
    assert sum(len(zc.RECORDS[n][0]) > 1 for n in ok) >= 10
    assert sum(zc.RECORDS[n][1] for n in ok) == 6
    for n in ("h_3frames_skips", "h_40frames_skips", "h_skippable_only", "h_checksummed_x3",
              "h_plain_then_checksummed", "h_checksummed_then_skippables", "b_1000_empty_raw"):
        assert n in zc.RECORDS


def test_accepted_entries_match_the_builders_record(zp):
    """blocks = the block headers the builder wrote; bound = ceil4(8 + per
    block 4 + 2 nseq + ceil(2 nseq / 63)) and covers the items the replay
    emits; cks = some frame of the entry was built with the checksum flag"""
    for name, entry, _dsize, _exp, code in zc.CASES:
        if code != 0:
            continue
        frames, want_cks = zc.RECORDS[name]
        bound, blocks, cks = plan(zp, entry)
        assert cks == want_cks, name
        assert blocks == sum(len(fr) for fr in frames), name
        want = 8
        for fr in frames:
            for b in fr:
                nseq = 0 if isinstance(b, (bytes, bytearray)) else len(b[1])
                want += 4 + 2 * nseq + (2 * nseq + 62) // 63
        assert bound == (want + 3) & ~3, name
        emitted = zc.items(frames)
        if emitted:
            slot, ext, pad = emitted[-1]
            assert bound >= slot + ((2 + pad) if ext else 1), name


def test_every_entry_whole_and_cut(zp):
    for name, entry in ENTRIES:
        assert plan(zp, entry)[0] <= BOUND_MAX, name
        for n in {0, 1, 8, 9, len(entry) - 1}:
            if 0 <= n <= len(entry):
                assert plan(zp, entry[:n])[0] <= BOUND_MAX, (name, n)


def test_no_read_past_the_entry_under_asan(zp, tmp_path):
    """the same walks from heap buffers of exactly each length, in a
    stand-alone program under AddressSanitizer and UBSan (CPU only); its
    answers for the whole entries are the shim's"""
    prog, dump = tmp_path / "zstd_plan_asan", tmp_path / "entries.bin"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DZSTD_PLAN_MAIN", "-o", str(prog), SHIM], check=True)
    dump.write_bytes(b"".join(struct.pack("<I", len(e)) + e for _, e in ENTRIES))
    r = subprocess.run([str(prog), str(dump)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.split("\n") if line]
    assert got == [tuple(int(x) for x in plan(zp, e)) for _, e in ENTRIES]
