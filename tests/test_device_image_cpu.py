"""The device-image entry points where no GPU is needed: the capacity formula
of zsk_lz4_image_bound, and clean refusals of zsk_reader_open_device /
zsk_lz4_build_image for memory that is not device memory (or on a machine with
no HIP device at all)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import golden_file

MIB = 1 << 20
NO_DEVICE = "no HIP device available"


def _slot(n: int) -> int:
    """ZSK_LZ4_COMPRESS_BOUND (include/zseek_hip.h)."""
    return (n + 4 * (n >> 16) + 24 + 15) & ~15


def _bound(length: int, frame_size: int, checksums: bool) -> int:
    """Every frame at its compressor bound, then the seek table: an 8-byte
    skippable header, 8 (12 with checksums) bytes per frame, a 9-byte footer."""
    full, tail = divmod(length, frame_size)
    frames = full + (1 if tail else 0)
    return full * _slot(frame_size) + (_slot(tail) if tail else 0) + 8 + (12 if checksums else 8) * frames + 9


@pytest.mark.parametrize("length,frame_size", [
    (0, 65536), (1, 65536), (65536, 65536), (65537, 65536), (3 * 65536 + 100, 65536), (200_000, 4096),
    (2 * MIB + 5, MIB), (4 * MIB + 1, 4 * MIB), (1 << 30, 65536), ((1 << 30) + 12345, MIB), (999_999, 1000),
    (7, 3), ((1 << 40) + 1, 4 * MIB)])
def test_image_bound_formula(zs, length, frame_size):
    for ck in (False, True):
        assert zs.lz4_image_bound(length, frame_size, ck) == _bound(length, frame_size, ck)
    assert zs.lz4_image_bound(length, frame_size, True) - zs.lz4_image_bound(length, frame_size, False) == \
        4 * -(-length // frame_size)


def test_image_bound_covers_the_writer(zs):
    """The bound is at least the file the host writer produces, also for
    incompressible input (stored blocks)."""
    data = np.random.default_rng(3).integers(0, 256, 300_000, dtype=np.uint8).tobytes()
    for fs in (4096, 65536, 100_000):
        for ck in (False, True):
            w = zs.Writer(zs.ZSEEK_LZ4, fs)
            assert w.set_checksums(ck)
            for o in range(0, len(data), fs):
                w.write(data[o: o + fs])
            assert len(w.close()) <= zs.lz4_image_bound(len(data), fs, ck)
    assert zs.lz4_image_bound(0, 65536) == 17
    assert zs.lz4_image_bound(100, 0) == 0


def test_open_device_refuses_host_memory(zs):
    img = np.frombuffer(golden_file("lz4_64k_direct"), np.uint8).copy()
    for ptr in (img.ctypes.data, None):
        with pytest.raises(zs.ZseekError) as e:
            zs.Reader.open_device(ptr, img.size, 1)
        assert str(e.value) in (NO_DEVICE, "open device image: not device memory")


def test_build_image_refuses_host_memory(zs):
    src = np.zeros(100_000, np.uint8)
    dst = np.full(zs.lz4_image_bound(src.size, 65536) + 64, 0xA5, np.uint8)
    err = C.create_string_buffer(80)
    L = zs.lib()
    assert L.zsk_lz4_build_image(src.ctypes.data, src.size, 65536, 0, 0, 0, dst.ctypes.data, dst.size, err) == -1
    assert err.value.decode() in (NO_DEVICE, "build image: not device memory of one device")
    assert (dst == 0xA5).all()
    # argument checks come first, whatever the machine
    for fs, level in ((0, 0), (4 * MIB + 1, 0), (65536, 3)):
        assert L.zsk_lz4_build_image(src.ctypes.data, src.size, fs, level, 0, 0, dst.ctypes.data, dst.size, err) == -1
        assert err.value.decode().startswith("build image: ")
    assert L.zsk_lz4_build_image(None, 0, 65536, 0, 0, 0, None, 0, err) == -1
    assert (dst == 0xA5).all()
