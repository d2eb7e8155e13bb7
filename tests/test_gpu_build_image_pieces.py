"""zsk_lz4_build_image_pieces / zsk_zstd_build_image_pieces
(csrc/image_build.hip): seekable files built on the caller's stream, one frame
per piece of a list that is in device memory.

Yardsticks: for LZ4 the same library's host writer (liblz4 itself) with
min_frame_size 1 and one write per piece; for the fixed-frame form the writer
through zsk_write_device, the definition of zsk_lz4_build_image; for zstd the
frames zsk_zstd_compress_frames_ex writes for the pieces (pinned to their CPU
restatements by their own tests), libzstd and the oracle as decoders; and,
where the compiled reference exists, its reader.  Every image sits in a tensor
between two 64-byte guards of 0xA5, 0, 1 or 3 bytes past the first."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import zstd_util

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 64
MIB = 1 << 20
S = [1, 7, 4096, 65536, 65537, 3, 200_001]
TOP = max(S)
ATS = (0, 1, 3)
CK, CONTENT, FULL, WIDE = 1, 2, 4, 8     # ZSK_IMAGE_*

_SRC = {}
_WANT = {}


def _source(zs, gpu):
    """400,000 bytes of the synthetic with spans of random bytes spliced in
    (as test_gpu_build_image.py's source), once.  -> (host bytes, device tensor)."""
    import torch
    if not _SRC:
        data = zs.synth_buffer(400_000).copy()
        rng = np.random.default_rng(77)
        for a, n in ((20_000, 10_000), (100_000, 40_000), (3 * 65536, 65536 + 5000)):
            data[a: a + n] = rng.integers(0, 256, n, dtype=np.uint8)
        _SRC["host"] = data
        _SRC["dev"] = torch.from_numpy(data).to(gpu)
        torch.cuda.synchronize()
    return _SRC["host"], _SRC["dev"]


def _pieces_file(zs, host, sizes, level, checksums) -> bytes:
    """The sequence the LZ4 build from pieces is defined by (computed once per case)."""
    key = (tuple(sizes), level, checksums)
    if key not in _WANT:
        w = zs.Writer(zs.ZSEEK_LZ4, 1, level)
        assert w.set_checksums(checksums)
        at = 0
        for n in sizes:
            w.write(host[at: at + n])
            at += n
        _WANT[key] = w.close()
    return _WANT[key]


def _sizes(gpu, sizes):
    import torch
    return torch.from_numpy(np.asarray(sizes, np.uint32).view(np.int32).copy()).to(gpu)


def _queue(zs, gpu, zstd, d_src, src_len, d_sizes, npieces, max_piece, level=0, flags=0, batch_bytes=0, at=0,
           capacity=None, stream=0, result="new", src_ptr=None, sizes_ptr=None, image_ptr=None):
    """One call.  -> (return value, errbuf, the image's tensor, capacity, the
    result tensor); nothing is synchronized."""
    import torch
    L = zs.lib()
    if capacity is None:
        capacity = (L.zsk_zstd_pieces_bound if zstd else L.zsk_lz4_pieces_bound)(src_len, npieces, flags)
    t = torch.full((GUARD + at + capacity + GUARD,), SENT, dtype=torch.uint8, device=gpu)
    res = torch.full((3,), -77, dtype=torch.int64, device=gpu) if isinstance(result, str) else result
    torch.cuda.synchronize()
    err = C.create_string_buffer(80)
    src = src_ptr if src_ptr is not None else (d_src.data_ptr() if src_len else None)
    sz = sizes_ptr if sizes_ptr is not None else (None if d_sizes is None else d_sizes.data_ptr())
    img = image_ptr if image_ptr is not None else t.data_ptr() + GUARD + at
    rp = None if res is None else res.data_ptr()
    if zstd:
        rc = L.zsk_zstd_build_image_pieces(src, src_len, sz, npieces, max_piece, flags, batch_bytes, img, capacity,
                                           rp, stream, err)
    else:
        rc = L.zsk_lz4_build_image_pieces(src, src_len, sz, npieces, max_piece, level, flags, batch_bytes, img,
                                          capacity, rp, stream, err)
    return rc, err.value.decode(), t, capacity, res


def _image(out, at=0):
    """After a synchronize: -> (the file, d_result as a tuple), the guards checked."""
    rc, err, t, cap, res = out
    assert rc == 0, err
    r = tuple(int(x) for x in res.cpu())
    host = t.cpu().numpy()
    assert (host[: GUARD + at] == SENT).all() and (host[GUARD + at + cap:] == SENT).all()   # guards
    assert r[0] <= cap
    return (bytes(host[GUARD + at: GUARD + at + r[0]]) if r[0] >= 0 else None), r


def _ref_reads_back(ref, image: bytes, want: bytes):
    r = ref.open(image, 0)
    assert r.h, r.error
    got = bytearray()
    while len(got) < len(want):
        k, b = r.pread(len(want) - len(got), len(got))
        assert k > 0, r.error
        got += b
    r.close()
    assert bytes(got) == want


@pytest.mark.parametrize("level", [0, -2])
@pytest.mark.parametrize("checksums", [False, True])
def test_lz4_byte_identity(gpu, zs, request, level, checksums):
    import torch
    from oracle.oracle import REF_SO
    host, dev = _source(zs, gpu)
    want = _pieces_file(zs, host, S, level, checksums)
    d_sizes = _sizes(gpu, S)
    for at in ATS:
        out = _queue(zs, gpu, False, dev, host.size, d_sizes, len(S), TOP, level, CK if checksums else 0, at=at)
        torch.cuda.synchronize()
        got, res = _image(out, at)
        assert res == (len(want), len(S), sum(S))
        assert got == want
    if os.path.exists(REF_SO):
        _ref_reads_back(request.getfixturevalue("ref"), got, host[: sum(S)].tobytes())
    with zs.Reader(got, 0) as r:                      # frame index = piece index
        _, d_off = r.frames()
        assert [int(x) for x in d_off] == [0] + [int(x) for x in np.cumsum(S)]


@pytest.mark.parametrize("checksums", [False, True])
def test_batch_chaining(gpu, zs, checksums):
    """Batches of 1, 2 and 3 pieces: the running source offset, the running
    file offset and the global frame index carry over; the bytes are the
    one-batch bytes."""
    import torch
    host, dev = _source(zs, gpu)
    want = _pieces_file(zs, host, S, 0, checksums)
    d_sizes = _sizes(gpu, S)
    for k, at in zip((1, 2, 3), ATS):
        out = _queue(zs, gpu, False, dev, host.size, d_sizes, len(S), TOP, 0, CK if checksums else 0,
                     batch_bytes=k * TOP, at=at)
        torch.cuda.synchronize()
        got, res = _image(out, at)
        assert res == (len(want), len(S), sum(S)), k
        assert got == want, k


@pytest.mark.parametrize("length,frame_size", [(0, 65536), (1, 65536), (3 * 65536 + 100, 65536), (200_000, 4096)])
@pytest.mark.parametrize("checksums", [False, True])
def test_null_sizes_is_the_fixed_frame_build(gpu, zs, length, frame_size, checksums):
    import torch
    host, dev = _source(zs, gpu)
    w = zs.Writer(zs.ZSEEK_LZ4, frame_size, 0)        # test_gpu_build_image.py's _writer_file
    assert w.set_checksums(checksums)
    w.write_device(dev.data_ptr(), length, frame_size)
    want = w.close()
    n = -(-length // frame_size)
    for at in ATS:
        out = _queue(zs, gpu, False, dev, length, None, n, frame_size, 0, CK if checksums else 0, at=at)
        torch.cuda.synchronize()
        got, res = _image(out, at)
        assert res == (len(want), n, length)
        assert got == want
    for bad in (n + 1, n - 1):
        if bad < 0:
            continue
        rc, err, t, cap, res = _queue(zs, gpu, False, dev, length, None, bad, frame_size, 0, 0,
                                      capacity=zs.lz4_pieces_bound(length, n + 1) + 64)
        torch.cuda.synchronize()
        assert (rc, err) == (-1, "build image: invalid piece count")
        assert bool((t == SENT).all()) and bool((res == -77).all())


def _table_sizes(image: bytes, nframes: int, ew: int):
    body = np.frombuffer(image[-9 - 4 * ew * nframes: -9], "<u4").reshape(nframes, ew)
    assert int.from_bytes(image[-9:-5], "little") == nframes
    return body


@pytest.mark.parametrize("fmt", [0, FULL, WIDE])
def test_zstd_frames_are_the_compressor_frames(gpu, zs, oracle, request, fmt):
    import torch
    from oracle.oracle import REF_SO
    host, dev = _source(zs, gpu)
    flags = fmt | CK | CONTENT
    d_sizes = _sizes(gpu, S)
    outs = [_queue(zs, gpu, True, dev, host.size, d_sizes, len(S), TOP, flags=flags, at=at,
                   batch_bytes=(3 * TOP if at == 1 else 0)) for at in ATS]
    # the yardstick: the existing call on the same pieces in the same format
    desc, total = zs.zstd_compress_layout(S, flags=[zs.COMPRESS_CONTENT_CHECKSUM] * len(S))
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    d_dst = torch.full((total,), SENT, dtype=torch.uint8, device=gpu)
    csize = torch.full((len(S),), -1, dtype=torch.int32, device=gpu)
    zs.zstd_compress_frames(d_desc, dev, d_dst, csize, full=bool(fmt & FULL), wide=bool(fmt & WIDE))
    torch.cuda.synchronize()
    slots, cs = d_dst.cpu().numpy(), csize.cpu().numpy()
    want = [slots[int(d["dst_off"]): int(d["dst_off"]) + int(c)].tobytes() for d, c in zip(desc, cs)]
    assert all(c > 0 for c in cs)
    zstd = zstd_util.load()
    for out, at in zip(outs, ATS):
        got, res = _image(out, at)
        assert res == (sum(len(f) for f in want) + 17 + 12 * len(S), len(S), sum(S))
        ent = _table_sizes(got, len(S), 3)
        c_at = s_at = 0
        for i, n in enumerate(S):
            piece = host[s_at: s_at + n].tobytes()
            frame = got[c_at: c_at + int(ent[i, 0])]
            assert frame == want[i], i
            assert int(ent[i, 1]) == n and int(ent[i, 2]) == oracle.xxh64(piece) & 0xFFFFFFFF
            if at == 0:
                dec, e = oracle.zstd_decode(frame, n)
                assert e == 0 and bytes(dec) == piece, i
                if zstd is not None:
                    assert zstd_util.decode(zstd, frame, n) == (piece, 0)    # (checks the in-frame word too)
            c_at += int(ent[i, 0])
            s_at += n
    if os.path.exists(REF_SO):
        _ref_reads_back(request.getfixturevalue("ref"), got, host[: sum(S)].tobytes())
    # NULL sizes: zsk_zstd_build_image's bytes
    length, fs = 3 * 65536 + 100, 65536
    same = zs.zstd_build_image(dev[:length], fs, checksums=True, content_checksums=True, full=bool(fmt & FULL),
                               wide=bool(fmt & WIDE)).cpu().numpy().tobytes()
    out = _queue(zs, gpu, True, dev, length, None, 4, fs, flags=flags, at=3)
    torch.cuda.synchronize()
    got, res = _image(out, 3)
    assert got == same and res == (len(same), 4, length)


def test_stream_order(gpu, zs):
    """Producer copies, two builds that share a pool set, and the copies of
    their results, queued back to back on a side stream: one synchronization,
    at the end."""
    import torch
    host, dev = _source(zs, gpu)
    other = [5000, 70_000, 1, 65536, 33]
    want = [_pieces_file(zs, host, z, 0, True) for z in (S, other)]
    n = host.size
    q = torch.cuda.Stream(device=gpu)
    pin_src = torch.from_numpy(host).pin_memory()
    pin_sizes = [torch.from_numpy(np.asarray(z, np.uint32).view(np.int32).copy()).pin_memory() for z in (S, other)]
    d_src = torch.empty(n, dtype=torch.uint8, device=gpu)
    d_sizes = [torch.empty(len(z), dtype=torch.int32, device=gpu) for z in (S, other)]
    caps = [zs.lz4_pieces_bound(n, len(z), True) for z in (S, other)]
    imgs = [torch.full((GUARD + 1 + c + GUARD,), SENT, dtype=torch.uint8, device=gpu) for c in caps]
    res = [torch.full((3,), -77, dtype=torch.int64, device=gpu) for _ in range(2)]
    seen = [torch.full((3,), -78, dtype=torch.int64, device=gpu) for _ in range(2)]
    # (a first call sizes the pooled scratch: growing it is the one wait the call may make)
    warm = _queue(zs, gpu, False, dev, n, _sizes(gpu, S), len(S), TOP, 0, CK)
    torch.cuda.synchronize()
    assert _image(warm)[0] == want[0]
    with torch.cuda.stream(q):
        d_src.fill_(0x55)                                  # 1. wrong values
        for t in d_sizes:
            t.fill_(9)
        d_src.copy_(pin_src, non_blocking=True)            # 2. the right ones
        for t, p in zip(d_sizes, pin_sizes):
            t.copy_(p, non_blocking=True)
        for i, z in enumerate((S, other)):                 # 3., 4. the builds
            zs.lz4_build_image_pieces(d_src, d_sizes[i], TOP, imgs[i][GUARD + 1: GUARD + 1 + caps[i]], res[i],
                                      checksums=True, stream=q.cuda_stream)
        for i in range(2):                                 # 5. consumers
            seen[i].copy_(res[i], non_blocking=True)
    q.synchronize()
    for i, z in enumerate((S, other)):
        r = tuple(int(x) for x in seen[i].cpu())
        assert r == (len(want[i]), len(z), sum(z)), i
        h = imgs[i].cpu().numpy()
        assert (h[: GUARD + 1] == SENT).all() and (h[GUARD + 1 + caps[i]:] == SENT).all()
        assert bytes(h[GUARD + 1: GUARD + 1 + r[0]]) == want[i], i


def test_device_refusals(gpu, zs):
    """The list is data: an invalid one answers IMAGE_BAD_PIECES, writes
    nothing outside the capacity, and the next call on the stream builds
    normally."""
    import torch
    host, dev = _source(zs, gpu)
    want = _pieces_file(zs, host, S, 0, False)
    zero, big = list(S), list(S)
    zero[4] = 0
    big[2] = TOP + 1
    q = torch.cuda.Stream(device=gpu)
    d_good = _sizes(gpu, S)
    for (sizes, src_len), at in zip(((zero, host.size), (big, host.size), (S, sum(S) - 1)), ATS):
        d_bad = _sizes(gpu, sizes)            # (the lists outlive the work queued on them)
        for zstd in (False, True):
            for batch in (0, 2 * TOP):
                bad = _queue(zs, gpu, zstd, dev, src_len, d_bad, len(sizes), TOP, at=at,
                             batch_bytes=batch, stream=q.cuda_stream)
                good = _queue(zs, gpu, False, dev, host.size, d_good, len(S), TOP, at=at,
                              stream=q.cuda_stream)
                q.synchronize()
                got, res = _image(bad, at)
                assert res[0] == zs.IMAGE_BAD_PIECES and got is None, (sizes, zstd, batch)
                got, res = _image(good, at)
                assert got == want and res == (len(want), len(S), sum(S))


def test_host_refusals(gpu, zs):
    import torch
    host, dev = _source(zs, gpu)
    d_sizes = _sizes(gpu, S)
    bound = zs.lz4_pieces_bound(host.size, len(S))

    def refused(text, zstd=False, **kw):
        rc, err, t, cap, res = _queue(zs, gpu, zstd, dev, host.size, d_sizes, len(S), kw.pop("max_piece", TOP), **kw)
        torch.cuda.synchronize()
        assert (rc, err) == (-1, text), kw
        assert bool((t == SENT).all())
        assert res is None or bool((res == -77).all())

    for zstd in (False, True):
        refused("build image: buffer too small", zstd,
                capacity=(zs.zstd_pieces_bound if zstd else zs.lz4_pieces_bound)(host.size, len(S)) - 1)
        refused("build image: NULL result", zstd, result=None)
        refused("build image: invalid piece size", zstd, max_piece=0)
        refused("build image: invalid piece size", zstd, max_piece=4 * MIB + 1)
        side, h_sizes = np.full(bound + 64, SENT, np.uint8), np.asarray(S, np.uint32)
        for kw in ({"src_ptr": host.ctypes.data}, {"sizes_ptr": h_sizes.ctypes.data},
                   {"image_ptr": side.ctypes.data}):
            refused("build image: not device memory of one device", zstd, capacity=bound + 64, **kw)
        assert (side == SENT).all()
    refused("build image: HC levels are not supported", level=3)
    # a capturing stream (the graph is never replayed)
    q = torch.cuda.Stream(device=gpu)
    x = torch.zeros(16, device=gpu)
    t = torch.full((GUARD + bound + GUARD,), SENT, dtype=torch.uint8, device=gpu)
    res = torch.full((3,), -77, dtype=torch.int64, device=gpu)
    torch.cuda.synchronize()
    err = C.create_string_buffer(80)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=q):
        rc = zs.lib().zsk_lz4_build_image_pieces(dev.data_ptr(), host.size, d_sizes.data_ptr(), len(S), TOP, 0, 0, 0,
                                                 t.data_ptr() + GUARD, bound, res.data_ptr(), q.cuda_stream, err)
        x.add_(1)
    assert (rc, err.value) == (-1, b"build image: stream is capturing")
    del g
    torch.cuda.synchronize()
    assert bool((t == SENT).all()) and bool((res == -77).all())


def test_round_trip_on_the_device(gpu, zs):
    """Built with checksums, opened where it is with verification on: frame i
    is piece i, one range per piece returns each piece, nothing uploaded."""
    import torch
    host, dev = _source(zs, gpu)
    image = torch.empty(zs.lz4_pieces_bound(host.size, len(S), True), dtype=torch.uint8, device=gpu)
    res = torch.zeros(3, dtype=torch.int64, device=gpu)
    zs.lz4_build_image_pieces(dev, _sizes(gpu, S), TOP, image, res, checksums=True)
    size, frames, used = (int(x) for x in res.cpu())      # (the copy is ordered behind the build)
    assert (frames, used) == (len(S), sum(S)) and 0 < size <= image.numel()
    offs = [0] + [int(x) for x in np.cumsum(S)]
    with zs.Reader.open_device(image.data_ptr(), size, 0) as r:
        r.set_verify_checksums(True)
        _, d_off = r.frames()
        assert [int(x) for x in d_off] == offs
        rg = np.zeros(len(S), zs.RANGE_DTYPE)
        at = 0
        for i, n in enumerate(S):
            rg[i] = (offs[i], n, at, -7)
            at += n + 16
        out = torch.full((at,), SENT, dtype=torch.uint8, device=gpu)
        got_rg, n_ok = r.preadv_device(out.data_ptr(), rg)
        assert n_ok == len(S)
        got = out.cpu().numpy()
        for q, o, n in zip(got_rg, offs, S):
            d = int(q["dst_off"])
            assert int(q["result"]) == n
            assert np.array_equal(got[d: d + n], host[o: o + n])
            assert (got[d + n: d + n + 16] == SENT).all()
        assert r.gpu_stats()["bytes_uploaded"] == 0
