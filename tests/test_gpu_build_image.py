"""zsk_lz4_build_image (csrc/image_build.hip): a complete seekable LZ4 file
built in device memory.

The yardstick is the writer: the same library's host writer (liblz4 itself,
GPU mode off) fed the same bytes through zsk_write_device, and, where the
compiled reference exists, the reference writer's file.  The round trip reads
the built image back through zsk_reader_open_device and compares with the
source bytes."""
from __future__ import annotations

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 64
MIB = 1 << 20
PAIRS = [(0, 65536), (1, 65536), (65536, 65536), (65537, 65536), (3 * 65536 + 100, 65536), (200_000, 4096),
         (2 * MIB + 5, MIB), (4 * MIB + 1, 4 * MIB)]

_SRC = {}


def _source(zs, gpu):
    """4 MiB + 1 of the synthetic with spans of random bytes spliced in (whole
    4 KiB and 64 KiB frames of them are stored, not compressed), once; the
    tests take prefixes.  -> (host bytes, device tensor)."""
    import torch
    if not _SRC:
        data = zs.synth_buffer(4 * MIB + 1).copy()
        rng = np.random.default_rng(77)
        for a, n in ((20_000, 10_000), (100_000, 40_000), (3 * 65536, 65536 + 5000), (MIB + 300_000, 200_000)):
            data[a: a + n] = rng.integers(0, 256, n, dtype=np.uint8)
        _SRC["host"] = data
        _SRC["dev"] = torch.from_numpy(data).to(gpu)
        torch.cuda.synchronize()
    return _SRC["host"], _SRC["dev"]


def _writer_file(zs, d_src, length, frame_size, level, checksums) -> bytes:
    """The sequence zsk_lz4_build_image is defined by."""
    w = zs.Writer(zs.ZSEEK_LZ4, frame_size, level)
    assert w.set_checksums(checksums)
    w.write_device(d_src.data_ptr(), length, frame_size)
    return w.close()


def _build(zs, gpu, d_src, length, frame_size, level=0, checksums=False, batch_bytes=0, at=0, capacity=None):
    """-> (return value, errbuf, the whole tensor on the host, capacity): the
    image buffer starts `at` bytes past a 64-byte guard zone and is followed by
    another."""
    import ctypes as C

    import torch
    if capacity is None:
        capacity = zs.lz4_image_bound(length, frame_size, checksums)
    t = torch.full((GUARD + at + capacity + GUARD,), SENT, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    err = C.create_string_buffer(80)
    n = zs.lib().zsk_lz4_build_image(d_src.data_ptr(), length, frame_size, level, 1 if checksums else 0,
                                     batch_bytes, t.data_ptr() + GUARD + at, capacity, err)
    return n, err.value.decode(), t.cpu().numpy(), capacity


def _image(res, at=0) -> bytes:
    n, err, host, cap = res
    assert n >= 0, err
    assert n <= cap
    assert (host[: GUARD + at] == SENT).all() and (host[GUARD + at + cap:] == SENT).all()   # guards
    return bytes(host[GUARD + at: GUARD + at + n])


@pytest.mark.parametrize("length,frame_size", PAIRS)
@pytest.mark.parametrize("level", [0, -2])
@pytest.mark.parametrize("checksums", [False, True])
def test_byte_identity(gpu, zs, request, length, frame_size, level, checksums):
    from oracle.oracle import REF_SO
    host, dev = _source(zs, gpu)
    want = _writer_file(zs, dev, length, frame_size, level, checksums)
    got = _image(_build(zs, gpu, dev, length, frame_size, level, checksums))
    assert len(got) == len(want)
    assert got == want
    if not checksums and os.path.exists(REF_SO):
        ref = request.getfixturevalue("ref")      # (the compiled reference, where it was built)
        assert got == ref.compress(bytes(host[:length]), zs.ZSEEK_LZ4, frame_size, frame_size, level)
    # what the file says about itself
    if length:
        with zs.Reader(got, 0) as r:
            _, d_off = r.frames()
            assert len(d_off) - 1 == -(-length // frame_size)
            assert int(d_off[-1]) == length


@pytest.mark.parametrize("length,frame_size", [(11 * 65536 + 777, 65536), (200_000, 4096), (2 * MIB + 5, MIB)])
@pytest.mark.parametrize("checksums", [False, True])
def test_batch_chaining(gpu, zs, length, frame_size, checksums):
    """Batches of 2, 3 and 1 frames: the running file offset and the global
    frame index carry over; the bytes are the default's (one batch)."""
    host, dev = _source(zs, gpu)
    want = _image(_build(zs, gpu, dev, length, frame_size, 0, checksums))
    assert want == _writer_file(zs, dev, length, frame_size, 0, checksums)
    for frames in (2, 3, 1):
        got = _image(_build(zs, gpu, dev, length, frame_size, 0, checksums, batch_bytes=frames * frame_size))
        assert got == want, frames


@pytest.mark.parametrize("at", [0, 1, 3])
def test_bounds(gpu, zs, at):
    """capacity == bound succeeds (at odd offsets of a tensor too); one byte
    less fails before anything is written; the guard zone past capacity is
    never touched."""
    host, dev = _source(zs, gpu)
    length, frame_size = 5 * 65536 + 4321, 65536
    want = _writer_file(zs, dev, length, frame_size, 0, True)
    assert _image(_build(zs, gpu, dev, length, frame_size, 0, True, at=at), at) == want
    bound = zs.lz4_image_bound(length, frame_size, True)
    n, err, t, cap = _build(zs, gpu, dev, length, frame_size, 0, True, at=at, capacity=bound - 1)
    assert n == -1 and err == "build image: buffer too small"
    assert (t == SENT).all()


def test_refusals(gpu, zs):
    import ctypes as C
    host, dev = _source(zs, gpu)
    for kw in ({"frame_size": 0}, {"frame_size": 4 * MIB + 1}, {"level": 3}):
        a = {"frame_size": 65536, "level": 0, **kw}
        n, err, t, cap = _build(zs, gpu, dev, 100_000, a["frame_size"], a["level"], capacity=200_000)
        assert n == -1 and err.startswith("build image: "), (kw, err)
        assert (t == SENT).all()
    # a host pointer as the source, then as the image
    import torch
    err = C.create_string_buffer(80)
    img = torch.full((200_000,), SENT, dtype=torch.uint8, device=gpu)
    L = zs.lib()
    assert L.zsk_lz4_build_image(host.ctypes.data, 100_000, 65536, 0, 0, 0, img.data_ptr(), img.numel(), err) == -1
    assert err.value == b"build image: not device memory of one device"
    buf = np.zeros(200_000, np.uint8)
    assert L.zsk_lz4_build_image(dev.data_ptr(), 100_000, 65536, 0, 0, 0, buf.ctypes.data, buf.size, err) == -1
    assert err.value == b"build image: not device memory of one device"
    assert (img.cpu().numpy() == SENT).all() and not buf.any()


def test_round_trip_on_the_device(gpu, zs):
    """Built with checksums, opened where it is with verification on, read at
    random and whole: the source's bytes, and nothing uploaded."""
    import torch
    host, dev = _source(zs, gpu)
    length = 3 * MIB + 100
    image = zs.lz4_build_image(dev[:length], 65536, checksums=True)
    assert image.is_cuda and image.numel() < zs.lz4_image_bound(length, 65536, True)
    with zs.Reader.open_device(image.data_ptr(), image.numel(), 0) as r:
        r.set_verify_checksums(True)
        assert r.stats()["frames"] == 49 and r.stats()["decompressed_size"] == length
        rng = np.random.default_rng(5)
        rg = np.zeros(300, zs.RANGE_DTYPE)
        at = 0
        for i in range(300):
            off = int(rng.integers(0, length))
            cnt = int(rng.integers(1, min(length - off, 150_000) + 1))
            rg[i] = (off, cnt, at, -7)
            at += cnt + 16
        out = torch.full((at,), SENT, dtype=torch.uint8, device=gpu)
        res, n_ok = r.preadv_device(out.data_ptr(), rg)
        assert n_ok == 300
        got = out.cpu().numpy()
        for q in res:
            o, c, d = int(q["offset"]), int(q["count"]), int(q["dst_off"])
            assert int(q["result"]) == c
            assert np.array_equal(got[d: d + c], host[o: o + c]), (o, c)
            assert (got[d + c: d + c + 16] == SENT).all()
        whole = torch.full((length + 32,), SENT, dtype=torch.uint8, device=gpu)
        assert r.pread_device(whole.data_ptr(), length + 32, 0) == length
        assert torch.equal(whole[:length], dev[:length]) and bool((whole[length:] == SENT).all())
        assert r.gpu_stats()["bytes_uploaded"] == 0
