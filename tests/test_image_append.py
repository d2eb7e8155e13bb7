"""The appends to a seekable image in device memory where no GPU is needed
(zsk_lz4_append_image_pieces / zsk_zstd_append_image_pieces):

- the acceptance and room rules of libzseek_amd/csrc/image_append.h, through
  tests/native/image_append_shim.cpp, against a plain restatement, over valid
  files and one mutation each;
- zsk_*_append_bound covers the old frames, the sum of the compressors' bounds
  over any list and the new table; it is monotone in the old size and equals
  zsk_*_pieces_bound on the empty file;
- the new entries are declared, listed, exported and bound, and refuse cleanly
  without a device, the argument checks first."""
from __future__ import annotations

import ctypes as C
import os
import pathlib
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, gpu_available

MIB = 1 << 20
NEW = ["zsk_lz4_append_bound", "zsk_zstd_append_bound", "zsk_lz4_append_image_pieces", "zsk_zstd_append_image_pieces"]
BAD_IMAGE, NO_ROOM = -3, -4
SKIPPABLE, SEEK = 0x184D2A5E, 0x8F92EAB1
MAGIC = {False: 0x184D2204, True: 0xFD2FB528}      # by "is zstd"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = pathlib.Path(tmp_path_factory.mktemp("image_append")) / "libimage_append.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    os.path.join(ROOT, "tests", "native", "image_append_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.iappend_window.restype = C.c_int
    L.iappend_window.argtypes = [C.c_int64, C.c_uint64, C.c_uint64, C.c_int]
    L.iappend_check.restype = C.c_int64
    L.iappend_check.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_uint64, C.c_int, C.c_int,
                                C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    for fn in (L.iappend_lz4_bound, L.iappend_zstd_bound):
        fn.restype = C.c_uint64
        fn.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    L.iappend_table_bytes.restype = C.c_uint64
    L.iappend_table_bytes.argtypes = [C.c_uint64, C.c_int]
    L.iappend_drop_mask.restype = C.c_uint64
    return L


# -- the acceptance rule ---------------------------------------------------------------------
def table_bytes(frames: int, ck: bool) -> int:
    return 8 + (12 if ck else 8) * frames + 9


def make_file(frames: int, ck: bool, zstd: bool) -> bytearray:
    """A well-formed file: `frames` frames of 9 + i bytes, the first one
    starting with the codec's magic, and their table."""
    csize = [9 + i for i in range(frames)]
    body = bytearray(b"\x5A" * sum(csize))
    if frames:
        body[0:4] = struct.pack("<I", MAGIC[zstd])
    ent = b"".join(struct.pack("<II", c, 100 + c) + (struct.pack("<I", 7 * c) if ck else b"") for c in csize)
    return body + struct.pack("<II", SKIPPABLE, len(ent) + 9) + ent + struct.pack("<IBI", frames, 0x80 if ck else 0,
                                                                                  SEEK)


def restate(img: bytes, capacity: int, size: int, count: int, prev_frames: int, ck: bool, zstd: bool) -> bool:
    """The rule in plain Python, in the order the issue states it."""
    tb = table_bytes(prev_frames, ck)
    if count != prev_frames:
        return False
    if not tb <= size <= capacity:
        return False
    n, desc, magic = struct.unpack("<IBI", img[size - 9: size])
    if magic != SEEK or desc & 0x7C or n != prev_frames or bool(desc & 0x80) != ck:
        return False
    at = size - tb
    m, field = struct.unpack("<II", img[at: at + 8])
    if m != SKIPPABLE or field != tb - 8:
        return False
    ew = 12 if ck else 8
    if sum(struct.unpack("<I", img[at + 8 + ew * i: at + 12 + ew * i])[0] for i in range(prev_frames)) != at:
        return False
    if prev_frames and struct.unpack("<I", img[:4])[0] != MAGIC[zstd]:
        return False
    return True


def verdict(shim, img, capacity, size, count, prev_frames, ck, zstd, src_len=0, npieces=0):
    buf = np.frombuffer(bytes(img) + b"\xA5" * max(0, capacity - len(img)), np.uint8)
    assert buf.size >= capacity                      # (the shim reads image[0, capacity) at most)
    at = C.c_uint64(0)
    got = shim.iappend_check(buf.ctypes.data, capacity, size, count, prev_frames, int(ck), int(zstd), src_len, npieces,
                             C.byref(at))
    return int(got), int(at.value)


def cases():
    """-> (name, image, capacity, size, count, prev_frames, ck, zstd)"""
    for frames in (0, 1, 7):
        for ck in (False, True):
            for zstd in (False, True):
                img = make_file(frames, ck, zstd)
                n, cap = len(img), len(img) + 100
                tag = "%d%s%s" % (frames, "c" if ck else "", "z" if zstd else "")
                yield "valid " + tag, img, cap, n, frames, frames, ck, zstd
                yield "valid, capacity = size " + tag, img, n, n, frames, frames, ck, zstd
                for size in (n - 1, n + 1, 0, -1, -2, cap + 1, 1 << 62, table_bytes(frames, ck) - 1):
                    yield "size %d %s" % (size, tag), img, cap, size, frames, frames, ck, zstd
                yield "count + 1 " + tag, img, cap, n, frames + 1, frames, ck, zstd
                yield "count -1 " + tag, img, cap, n, -1, frames, ck, zstd
                yield "frames stated + 1 " + tag, img, cap, n, frames + 1, frames + 1, ck, zstd
                yield "checksum flag flipped " + tag, img, cap, n, frames, frames, not ck, zstd
                for bit in (0x04, 0x08, 0x10, 0x20, 0x40):
                    m = bytearray(img)
                    m[n - 5] |= bit
                    yield "reserved bit %#x %s" % (bit, tag), m, cap, n, frames, frames, ck, zstd
                m = bytearray(img)
                m[n - 5] ^= 0x80
                yield "checksum bit flipped in the file " + tag, m, cap, n, frames, frames, ck, zstd
                for k in (n - 4, n - 1):                             # the footer's magic
                    m = bytearray(img)
                    m[k] ^= 1
                    yield "footer magic %d %s" % (k, tag), m, cap, n, frames, frames, ck, zstd
                m = bytearray(img)
                m[n - 9] ^= 1                                        # the footer's frame count
                yield "footer count " + tag, m, cap, n, frames, frames, ck, zstd
                at = n - table_bytes(frames, ck)
                for k in (at, at + 3):                               # the header's magic
                    m = bytearray(img)
                    m[k] ^= 0x10
                    yield "header magic %d %s" % (k, tag), m, cap, n, frames, frames, ck, zstd
                m = bytearray(img)
                m[at + 4] ^= 1                                       # the header's size field
                yield "header size field " + tag, m, cap, n, frames, frames, ck, zstd
                if frames:
                    ew = 12 if ck else 8
                    for f in (0, frames - 1):
                        for d in (1, -1):
                            m = bytearray(img)
                            c = struct.unpack("<I", m[at + 8 + ew * f: at + 12 + ew * f])[0]
                            m[at + 8 + ew * f: at + 12 + ew * f] = struct.pack("<I", c + d)
                            yield "cSize[%d] %+d %s" % (f, d, tag), m, cap, n, frames, frames, ck, zstd
                    m = bytearray(img)
                    m[0:4] = struct.pack("<I", MAGIC[not zstd])
                    yield "the other codec's magic " + tag, m, cap, n, frames, frames, ck, zstd
                    yield "the other codec stated " + tag, img, cap, n, frames, frames, ck, not zstd
                    # frames stated on a file that is only its 17-byte empty table
                    empty = make_file(0, ck, zstd)
                    yield "frames on a 17-byte file " + tag, empty, cap, 17, frames, frames, ck, zstd


def test_acceptance_rule(shim):
    seen = {True: 0, False: 0}
    for name, img, cap, size, count, prev_frames, ck, zstd in cases():
        want = restate(bytes(img) + b"\xA5" * (cap - len(img)), cap, size, count, prev_frames, ck, zstd)
        got, at = verdict(shim, img, cap, size, count, prev_frames, ck, zstd)
        assert got == (0 if want else BAD_IMAGE), name
        assert want == name.startswith("valid"), name
        if want:
            assert at == size - table_bytes(prev_frames, ck), name
        seen[want] += 1
    assert seen[True] == 24 and seen[False] > 300


def test_unused_descriptor_bits_are_ignored(shim):
    """(as read_seek_table: only 0x7c is reserved)"""
    img = make_file(3, True, False)
    img[len(img) - 5] |= 0x03
    assert verdict(shim, img, len(img), len(img), 3, 3, True, False)[0] == 0


def test_window(shim):
    w = shim.iappend_window
    for frames in (0, 1, 1000):
        for ck in (0, 1):
            tb = table_bytes(frames, bool(ck))
            assert shim.iappend_table_bytes(frames, ck) == tb
            assert w(tb, tb, frames, ck) and w(tb, tb + 5, frames, ck) and w(tb + 5, tb + 5, frames, ck)
            assert not w(tb - 1, tb + 5, frames, ck) and not w(tb + 6, tb + 5, frames, ck)
            assert not w(tb, tb - 1, frames, ck)
            for size in (0, -1, -2, -3, -4, -(1 << 63), (1 << 63) - 1, 1 << 62):
                assert not w(size, 1 << 40, frames, ck)
    assert shim.iappend_drop_mask() == 2 | 4 | 8


def lz4_slot(n: int) -> int:
    """ZSK_LZ4_COMPRESS_BOUND (include/zseek_hip.h)."""
    return (n + 4 * (n >> 16) + 24 + 15) & ~15


def zstd_slot(n: int) -> int:
    """ZSK_ZSTD_COMPRESS_BOUND."""
    return (9 + 3 * (((n + 131071) >> 17) if n else 1) + n + 4 + 15) & ~15


def test_room_rule(zs, shim):
    """An accepted file answers NO_ROOM exactly when the bound at its actual
    size exceeds the capacity."""
    for zstd in (False, True):
        bound = zs.zstd_append_bound if zstd else zs.lz4_append_bound
        for frames, ck in ((0, False), (7, True)):
            img = make_file(frames, ck, zstd)
            n = len(img)
            for src_len, k in ((0, 0), (1, 1), (300_000, 5)):
                need = bound(n, frames, src_len, k, ck)
                assert verdict(shim, img, need, n, frames, frames, ck, zstd, src_len, k)[0] == 0
                assert verdict(shim, img, need + 1, n, frames, frames, ck, zstd, src_len, k)[0] == 0
                if need - 1 >= n:
                    assert verdict(shim, img, need - 1, n, frames, frames, ck, zstd, src_len, k)[0] == NO_ROOM
                # BAD_IMAGE comes before NO_ROOM
                assert verdict(shim, img, need - 1, n, frames + 1, frames, ck, zstd, src_len, k)[0] == BAD_IMAGE


# -- the bounds -----------------------------------------------------------------------------
def test_bounds_cover_any_list(zs, shim):
    rng = np.random.default_rng(4096)
    for _ in range(1000):
        k = int(rng.integers(0, 65))
        z = [int(x) for x in rng.integers(1, 300_001, k)]
        ck = bool(rng.integers(0, 2))
        prev_frames = int(rng.integers(0, 5000))
        old_data = int(rng.integers(0, 1 << 33))
        prev_size = old_data + table_bytes(prev_frames, ck)
        src_len = sum(z) + int(rng.choice([0, 1, 70_000]))
        table = table_bytes(prev_frames + k, ck)
        for name, slot in (("lz4", lz4_slot), ("zstd", zstd_slot)):
            got = getattr(zs, name + "_append_bound")(prev_size, prev_frames, src_len, k, ck)
            assert got == getattr(shim, "iappend_%s_bound" % name)(prev_size, prev_frames, src_len, k, int(ck))
            assert got >= old_data + sum(slot(s) for s in z) + table, (name, z)
            # the stated formula
            pieces = getattr(zs, name + "_pieces_bound")
            assert got == old_data + pieces(src_len, k, ck) - table_bytes(k, ck) + table
            # monotone in the old size
            step = int(rng.integers(1, 1 << 20))
            assert getattr(zs, name + "_append_bound")(prev_size + step, prev_frames, src_len, k, ck) == got + step
            assert getattr(zs, name + "_append_bound")(table_bytes(prev_frames, ck), prev_frames, src_len, k, ck) <= got
            # on the empty file: the builder's bound
            assert getattr(zs, name + "_append_bound")(17, 0, src_len, k, ck) == pieces(src_len, k, ck)
            # a size that cannot hold the table
            assert getattr(zs, name + "_append_bound")(table_bytes(prev_frames, ck) - 1, prev_frames, src_len, k, ck) == 0
    assert zs.lz4_append_bound(0, 0, 0, 0) == 0 and zs.lz4_append_bound(17, 0, 0, 0) == 17
    assert zs.zstd_append_bound(16, 0, 5, 1) == 0 and zs.zstd_append_bound(17, 0, 0, 0) == 17


# -- the interface --------------------------------------------------------------------------
def test_entries_declared_listed_exported(zs):
    text = open(os.path.join(ROOT, "include", "zseek_hip.h")).read()
    mapped = open(os.path.join(ROOT, "libzseek_amd", "csrc", "libzseek.map")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", zs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"ZSEEK_EXPORT\s+\w+\s+%s\s*\(" % name, text), name
        assert re.search(r"^\s*%s;" % name, mapped, re.M), name
        assert name in zs.EXPORTED and hasattr(zs.lib(), name)
        assert getattr(zs.lib(), name).argtypes, name
        assert any(ln.split()[-1] == name and ln.split()[-2] == "T" for ln in out.splitlines()), name
    assert re.search(r"#define\s+ZSK_IMAGE_BAD_IMAGE\s+\(-3\)", text)
    assert re.search(r"#define\s+ZSK_IMAGE_NO_ROOM\s+\(-4\)", text)
    assert (zs.IMAGE_BAD_IMAGE, zs.IMAGE_NO_ROOM) == (BAD_IMAGE, NO_ROOM)
    import libzseek_amd
    for name in ("lz4_append_image_pieces", "zstd_append_image_pieces", "lz4_append_bound", "zstd_append_bound",
                 "IMAGE_BAD_IMAGE", "IMAGE_NO_ROOM"):
        assert hasattr(libzseek_amd, name)


def test_refusals_without_a_device(zs):
    """Every argument check comes first, whatever the machine; then, with host
    memory for every pointer, the device check: no device at all where there is
    none."""
    L = zs.lib()
    err = C.create_string_buffer(zs.ERRBUF)
    src = np.zeros(100_000, np.uint8)
    sizes = np.array([50_000, 50_000], np.uint32)
    res = np.full(3, 77, np.int64)
    prev = np.array([17 + 3 * 8, 3], np.int64)
    need = {False: zs.lz4_append_bound(17 + 3 * 8, 3, src.size, 2), True: zs.zstd_append_bound(17 + 3 * 8, 3, src.size, 2)}
    dst = np.full(max(need.values()) + 64, 0xA5, np.uint8)

    def call(zstd, **kw):
        a = {"sizes": sizes.ctypes.data, "k": 2, "max_piece": 65536, "level": 0, "cap": dst.size,
             "res": res.ctypes.data, "prev": prev.ctypes.data, "frames": 3, "flags": 0, **kw}
        if zstd:
            r = L.zsk_zstd_append_image_pieces(src.ctypes.data, src.size, a["sizes"], a["k"], a["max_piece"],
                                               a["flags"], 0, dst.ctypes.data, a["cap"], a["prev"], a["frames"],
                                               a["res"], None, err)
        else:
            r = L.zsk_lz4_append_image_pieces(src.ctypes.data, src.size, a["sizes"], a["k"], a["max_piece"],
                                              a["level"], a["flags"], 0, dst.ctypes.data, a["cap"], a["prev"],
                                              a["frames"], a["res"], None, err)
        return r, err.value.decode()

    for zstd in (False, True):
        assert call(zstd, res=None) == (-1, "append image: NULL result")
        assert call(zstd, prev=None) == (-1, "append image: NULL prev")
        assert call(zstd, sizes=None) == (-1, "append image: needs a piece list")
        assert call(zstd, sizes=None, k=0) == (-1, "append image: needs a piece list")
        assert call(zstd, max_piece=0) == (-1, "append image: invalid piece size")
        assert call(zstd, max_piece=4 * MIB + 1) == (-1, "append image: invalid piece size")
        assert call(zstd, k=(1 << 27) - 2) == (-1, "append image: Frame index is too large")
        assert call(zstd, frames=(1 << 27) - 1) == (-1, "append image: Frame index is too large")
        assert call(zstd, frames=(1 << 27) + 1, k=0) == (-1, "append image: Frame index is too large")
        for kw in ({"res": res.ctypes.data + 4}, {"prev": prev.ctypes.data + 4}, {"sizes": sizes.ctypes.data + 2}):
            assert call(zstd, **kw) == (-1, "append image: misaligned sizes, prev or result")
        # the smallest file that could be there: its table alone
        assert call(zstd, cap=need[zstd] - 1) == (-1, "append image: buffer too small")
        assert call(zstd, cap=need[zstd] + 19, flags=1) == (-1, "append image: buffer too small")
        # nothing wrong with the arguments: now the device is asked for
        for kw in ({}, {"cap": need[zstd]}, {"k": 0}, {"frames": (1 << 27) - 2, "cap": 1 << 40}):
            r, text = call(zstd, **kw)
            assert r == -1
            if gpu_available():
                assert text in ("no HIP device available", "append image: not device memory of one device")
            else:
                assert text == "no HIP device available"
    assert call(False, level=3) == (-1, "append image: HC levels are not supported")
    assert (dst == 0xA5).all() and (res == 77).all()
