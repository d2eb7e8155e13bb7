"""zsk_lz4_append_image_pieces / zsk_zstd_append_image_pieces
(csrc/image_build.hip): frames appended on the caller's stream to a seekable
file that is in device memory.

The yardstick is the file format's own: frames are independent and the table
is a function of their sizes, so "build A, then append B" is byte for byte
"build A + B" -- for LZ4 the host writer's file for one write per piece, for
zstd zsk_zstd_build_image_pieces over the whole list (pinned by its own
tests).  Shapes are test_gpu_build_image_pieces.py's: the 400,000-byte source,
the seven pieces S, every image between two 64-byte guards of 0xA5 at byte
offsets 0, 1 and 3.  Every bad input here is one the device refuses by a value
check before the access.

d_result[2] is the source bytes consumed of the call's own d_src: the append
of S[k:] answers sum(S[k:]), and the build's and the append's add up to
sum(S)."""
from __future__ import annotations

import ctypes as C
import os
import struct

import numpy as np
import pytest

import zstd_util

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 64
S = [1, 7, 4096, 65536, 65537, 3, 200_001]
TOP = max(S)
ATS = (0, 1, 3)
CK, CONTENT, FULL, WIDE = 1, 2, 4, 8     # ZSK_IMAGE_*

_SRC = {}
_WANT = {}


def _source(zs, gpu):
    """test_gpu_build_image_pieces.py's source, once.  -> (host bytes, device tensor)"""
    import torch
    if not _SRC:
        data = zs.synth_buffer(400_000).copy()
        rng = np.random.default_rng(77)
        for a, n in ((20_000, 10_000), (100_000, 40_000), (3 * 65536, 65536 + 5000)):
            data[a: a + n] = rng.integers(0, 256, n, dtype=np.uint8)
        _SRC["host"] = data
        _SRC["dev"] = torch.from_numpy(data).to(gpu)
        # the list with one word behind it, so that the empty rest S[7:] is still a pointer into it
        _SRC["sizes"] = torch.from_numpy(np.asarray(S + [0], np.uint32).view(np.int32).copy()).to(gpu)
        torch.cuda.synchronize()
    return _SRC["host"], _SRC["dev"], _SRC["sizes"]


def _pieces_file(zs, host, sizes, level, checksums) -> bytes:
    """The host writer's file for one write per piece (computed once per case)."""
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


class Image:
    """`capacity` bytes of device memory between two guards, `at` bytes past the first."""

    def __init__(self, gpu, capacity, at=0):
        import torch
        self.t = torch.full((GUARD + at + capacity + GUARD,), SENT, dtype=torch.uint8, device=gpu)
        self.at, self.cap = at, capacity
        self.ptr = self.t.data_ptr() + GUARD + at

    def put(self, data: bytes):
        import torch
        a = GUARD + self.at
        self.t[a: a + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(self.t.device)

    def host(self):
        return self.t.cpu().numpy()

    def file(self, size) -> bytes:
        h = self.host()
        a = GUARD + self.at
        assert (h[:a] == SENT).all() and (h[a + self.cap:] == SENT).all()      # the guards
        assert 0 <= size <= self.cap
        return bytes(h[a: a + size])


def _res(gpu, values=(-77, -77, -77)):
    import torch
    return torch.tensor(list(values), dtype=torch.int64, device=gpu)


def _tuple(res):
    return tuple(int(x) for x in res.cpu())


def _build(zs, zstd, src_ptr, src_len, sizes_ptr, k, img, res, stream=0, level=0, flags=0, batch=0, capacity=None):
    err = C.create_string_buffer(80)
    cap = img.cap if capacity is None else capacity
    L = zs.lib()
    if zstd:
        rc = L.zsk_zstd_build_image_pieces(src_ptr, src_len, sizes_ptr, k, TOP, flags, batch, img.ptr, cap,
                                           res.data_ptr(), stream, err)
    else:
        rc = L.zsk_lz4_build_image_pieces(src_ptr, src_len, sizes_ptr, k, TOP, level, flags, batch, img.ptr, cap,
                                          res.data_ptr(), stream, err)
    assert rc == 0, err.value.decode()


def _append(zs, zstd, src_ptr, src_len, sizes_ptr, k, img, prev, prev_frames, res, stream=0, level=0, flags=0,
            batch=0, capacity=None):
    err = C.create_string_buffer(80)
    cap = img.cap if capacity is None else capacity
    L = zs.lib()
    if zstd:
        rc = L.zsk_zstd_append_image_pieces(src_ptr, src_len, sizes_ptr, k, TOP, flags, batch, img.ptr, cap,
                                            prev.data_ptr(), prev_frames, res.data_ptr(), stream, err)
    else:
        rc = L.zsk_lz4_append_image_pieces(src_ptr, src_len, sizes_ptr, k, TOP, level, flags, batch, img.ptr, cap,
                                           prev.data_ptr(), prev_frames, res.data_ptr(), stream, err)
    assert rc == 0, err.value.decode()


def _split(zs, gpu, zstd, k, at, stream, level=0, flags=0, batch=0):
    """build(S[:k]) then append(S[k:]) queued on `stream`, nothing synchronized
    between; the append's d_prev is the build's d_result.  -> (image, the build's
    result, the append's result)"""
    host, dev, d_sizes = _source(zs, gpu)
    ck = bool(flags & CK)
    n = host.size
    pieces = zs.zstd_pieces_bound if zstd else zs.lz4_pieces_bound
    bound = zs.zstd_append_bound if zstd else zs.lz4_append_bound
    used = sum(S[:k])
    cap = bound(pieces(n, k, ck), k, n - used, len(S) - k, ck)
    img = Image(gpu, cap, at)
    r0, r1 = _res(gpu), _res(gpu)
    _build(zs, zstd, dev.data_ptr(), n, d_sizes.data_ptr(), k, img, r0, stream, level, flags, batch)
    _append(zs, zstd, dev.data_ptr() + used, n - used, d_sizes.data_ptr() + 4 * k, len(S) - k, img, r0, k, r1,
            stream, level, flags, batch)
    return img, r0, r1


@pytest.mark.parametrize("level", [0, -2])
@pytest.mark.parametrize("checksums", [False, True])
def test_lz4_identity_at_every_split(gpu, zs, level, checksums):
    import torch
    host, dev, _ = _source(zs, gpu)
    want = _pieces_file(zs, host, S, level, checksums)
    q = torch.cuda.Stream(device=gpu)
    outs = [_split(zs, gpu, False, k, ATS[k % 3], q.cuda_stream, level, CK if checksums else 0)
            for k in range(len(S) + 1)]
    q.synchronize()
    for k, (img, r0, r1) in enumerate(outs):
        built, got = _tuple(r0), _tuple(r1)
        assert built[1:] == (k, sum(S[:k])), k
        assert built[0] == (len(_pieces_file(zs, host, S[:k], level, checksums)) if k else 17), k
        assert got == (len(want), len(S), sum(S[k:])), k
        assert built[2] + got[2] == sum(S)
        assert img.file(got[0]) == want, k
        if k == len(S):                                   # nothing appended: the size unchanged
            assert got[0] == built[0]


@pytest.mark.parametrize("checksums", [False, True])
def test_chain_of_appends(gpu, zs, checksums):
    """Build 2 pieces, append 2, 2 and 1, back to back, d_prev == d_result (one
    tensor), one piece per batch: several batches per append."""
    import torch
    host, dev, d_sizes = _source(zs, gpu)
    want = _pieces_file(zs, host, S, 0, checksums)
    flags = CK if checksums else 0
    q = torch.cuda.Stream(device=gpu)
    for at, batch in zip(ATS, (TOP, 0, TOP)):
        img = Image(gpu, zs.lz4_pieces_bound(host.size, len(S), checksums), at)
        res = _res(gpu)
        _build(zs, False, dev.data_ptr(), sum(S[:2]), d_sizes.data_ptr(), 2, img, res, q.cuda_stream, 0, flags, batch)
        done = 2
        for k in (2, 2, 1):
            used, take = sum(S[:done]), sum(S[done: done + k])
            _append(zs, False, dev.data_ptr() + used, take, d_sizes.data_ptr() + 4 * done, k, img, res, done, res,
                    q.cuda_stream, 0, flags, batch)
            done += k
        q.synchronize()
        got = _tuple(res)
        assert got == (len(want), len(S), S[-1])
        assert img.file(got[0]) == want


def _table_sizes(image: bytes, nframes: int, ew: int):
    body = np.frombuffer(image[-9 - 4 * ew * nframes: -9], "<u4").reshape(nframes, ew)
    assert int.from_bytes(image[-9:-5], "little") == nframes
    return body


@pytest.mark.parametrize("fmt", [0, FULL, WIDE])
def test_zstd_identity(gpu, zs, fmt):
    import torch
    host, dev, d_sizes = _source(zs, gpu)
    flags = fmt | CK | CONTENT
    q = torch.cuda.Stream(device=gpu)
    one = Image(gpu, zs.zstd_pieces_bound(host.size, len(S), True), 0)
    r = _res(gpu)
    _build(zs, True, dev.data_ptr(), host.size, d_sizes.data_ptr(), len(S), one, r, q.cuda_stream, flags=flags)
    outs = [(k, _split(zs, gpu, True, k, at, q.cuda_stream, flags=flags, batch=b))
            for k, at, b in ((0, 3, 0), (3, 1, 0), (5, 3, 2 * TOP), (7, 0, 0))]
    q.synchronize()
    size = _tuple(r)[0]
    want = one.file(size)
    for k, (img, r0, r1) in outs:
        got = _tuple(r1)
        assert got == (size, len(S), sum(S[k:])), k
        assert img.file(got[0]) == want, k
    # the file is valid zstd, frame by frame, and frame i is piece i
    zstd = zstd_util.load()
    ent = _table_sizes(want, len(S), 3)
    c_at = s_at = 0
    for i, n in enumerate(S):
        assert int(ent[i, 1]) == n
        if zstd is not None:
            assert zstd_util.decode(zstd, want[c_at: c_at + int(ent[i, 0])], n) == (host[s_at: s_at + n].tobytes(), 0)
        c_at += int(ent[i, 0])
        s_at += n
    # read where it is, checksum verification on
    img = outs[1][1][0]
    _read_back(zs, gpu, img.ptr, size, host[: sum(S)], [0] + [int(x) for x in np.cumsum(S)])


def _read_back(zs, gpu, ptr, size, want, offs):
    """zsk_reader_open_device on the image: frames() and every frame's bytes."""
    import torch
    with zs.Reader.open_device(ptr, size, 0) as r:
        r.set_verify_checksums(True)
        _, d_off = r.frames()
        assert [int(x) for x in d_off] == offs
        out = torch.full((len(want) + 16,), SENT, dtype=torch.uint8, device=gpu)
        rg = np.zeros(len(offs) - 1, zs.RANGE_DTYPE)
        for i in range(len(offs) - 1):
            rg[i] = (offs[i], offs[i + 1] - offs[i], offs[i], -7)
        got_rg, n_ok = r.preadv_device(out.data_ptr(), rg)
        assert n_ok == len(rg) and [int(x["result"]) for x in got_rg] == list(np.diff(offs))
        got = out.cpu().numpy()
        assert np.array_equal(got[: len(want)], want) and (got[len(want):] == SENT).all()


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


@pytest.mark.parametrize("checksums", [False, True])
def test_an_image_this_library_did_not_build(gpu, zs, request, checksums):
    """A host-writer file of fixed 64 KiB frames whose last, short frame carries
    a content-size field; three pieces appended."""
    import torch
    from oracle.oracle import REF_SO
    host, dev, _ = _source(zs, gpu)
    old_len, new = 3 * 65536 + 100, [5000, 70_000, 33]
    w = zs.Writer(zs.ZSEEK_LZ4, 65536, 0)
    assert w.set_checksums(checksums)
    for a in range(0, old_len, 65536):                    # (a write of 64 KiB is a frame; the rest is
        w.write(host[a: min(a + 65536, old_len)])         # the frame close() flushes)
    old = w.close()
    assert int.from_bytes(old[-9:-5], "little") == 4
    ew = 3 if checksums else 2
    old_table = 17 + 4 * ew * 4
    for at in (1, 0):
        img = Image(gpu, zs.lz4_append_bound(len(old), 4, sum(new), 3, checksums), at)
        img.put(old)
        prev, res = _res(gpu, (len(old), 4)), _res(gpu)
        d_new = torch.from_numpy(np.asarray(new, np.uint32).view(np.int32).copy()).to(gpu)
        torch.cuda.synchronize()
        _append(zs, False, dev.data_ptr() + old_len, sum(new), d_new.data_ptr(), 3, img, prev, 4, res,
                flags=CK if checksums else 0)
        torch.cuda.synchronize()
        got = _tuple(res)
        assert got[1:] == (7, sum(new))
        image = img.file(got[0])
        assert image[: len(old) - old_table] == old[: len(old) - old_table]            # the old frames' bytes
        ent = _table_sizes(image, 7, ew)
        assert np.array_equal(ent[:4], _table_sizes(old, 4, ew))                       # the old entries
        assert [int(x) for x in ent[4:, 1]] == new
        want = host[: old_len + sum(new)]
        with zs.Reader(image, 0) as r:
            back = bytearray()
            while len(back) < len(want):
                part = r.pread(len(want) - len(back), len(back))
                assert part
                back += part
            assert bytes(back) == want.tobytes()
        _read_back(zs, gpu, img.ptr, got[0], want, [0, 65536, 2 * 65536, 3 * 65536, old_len] +
                   [old_len + int(x) for x in np.cumsum(new)])
    if os.path.exists(REF_SO):
        _ref_reads_back(request.getfixturevalue("ref"), image, want.tobytes())


def _built(zs, gpu, zstd, k, at, flags=0, extra=4096):
    """S[:k] built and synchronized.  -> (image, its size, d_prev for an append)"""
    import torch
    host, dev, d_sizes = _source(zs, gpu)
    ck = bool(flags & CK)
    pieces = zs.zstd_pieces_bound if zstd else zs.lz4_pieces_bound
    bound = zs.zstd_append_bound if zstd else zs.lz4_append_bound
    cap = bound(pieces(host.size, k, ck), k, host.size - sum(S[:k]), len(S) - k, ck) + extra
    img = Image(gpu, cap, at)
    r = _res(gpu)
    _build(zs, zstd, dev.data_ptr(), host.size, d_sizes.data_ptr(), k, img, r, flags=flags)
    torch.cuda.synchronize()
    size = _tuple(r)[0]
    assert size > 0
    return img, size, r


def test_refusals_on_the_device(gpu, zs):
    """d_prev and the image are data: a file that is not valid answers
    IMAGE_BAD_IMAGE, one that might not fit IMAGE_NO_ROOM, and the whole
    capacity and both guards are as they were."""
    import torch
    host, dev, d_sizes = _source(zs, gpu)
    k = 4
    used = sum(S[:k])

    def refused(img, prev, code, prev_frames=k, flags=0, zstd=False, capacity=None):
        before = img.t.clone()
        res = _res(gpu)
        torch.cuda.synchronize()
        _append(zs, zstd, dev.data_ptr() + used, host.size - used, d_sizes.data_ptr() + 4 * k, len(S) - k, img,
                prev, prev_frames, res, flags=flags, capacity=capacity)
        torch.cuda.synchronize()
        assert _tuple(res)[0] == code, (prev, prev_frames, flags)
        assert torch.equal(img.t, before), (prev, prev_frames, flags)

    for at in (1, 0):
        img, size, _ = _built(zs, gpu, False, k, at)
        for bad in (size - 1, size + 1, 0, -2, -1, img.cap + 1, 1 << 62):
            refused(img, _res(gpu, (bad, k)), zs.IMAGE_BAD_IMAGE)
        refused(img, _res(gpu, (size, k + 1)), zs.IMAGE_BAD_IMAGE)
        refused(img, _res(gpu, (size, k)), zs.IMAGE_BAD_IMAGE, prev_frames=k - 1)
        refused(img, _res(gpu, (size, k - 1)), zs.IMAGE_BAD_IMAGE, prev_frames=k - 1)
        refused(img, _res(gpu, (size, k)), zs.IMAGE_BAD_IMAGE, flags=CK)
        # one byte of the file changed, then put back
        a = GUARD + at
        table = a + size - (17 + 8 * k)
        for where, x in ((a + size - 1, 1), (a + size - 4, 0x80), (a + size - 5, 0x04), (a + size - 5, 0x80),
                         (a + size - 9, 1), (table, 1), (table + 4, 1), (table + 8, 1), (table + 8 + 8 * (k - 1), 2),
                         (a, 1)):
            img.t[where] ^= x
            refused(img, _res(gpu, (size, k)), zs.IMAGE_BAD_IMAGE)
            img.t[where] ^= x
        # the other codec's first magic, and the other codec's call
        first = img.t[a: a + 4].clone()
        img.t[a: a + 4] = torch.tensor(list(struct.pack("<I", 0xFD2FB528)), dtype=torch.uint8, device=gpu)
        refused(img, _res(gpu, (size, k)), zs.IMAGE_BAD_IMAGE)
        img.t[a: a + 4] = first
        refused(img, _res(gpu, (size, k)), zs.IMAGE_BAD_IMAGE, zstd=True)
        # no room: one byte below the bound at the actual size, above the host's check
        need = zs.lz4_append_bound(size, k, host.size - used, len(S) - k)
        assert need - 1 >= zs.lz4_append_bound(17 + 8 * k, k, host.size - used, len(S) - k) and need - 1 >= size
        refused(img, _res(gpu, (size, k)), zs.IMAGE_NO_ROOM, capacity=need - 1)
        # ... and BAD_IMAGE comes first
        refused(img, _res(gpu, (size + 1, k)), zs.IMAGE_BAD_IMAGE, capacity=need - 1)
        # the file is still good: the append at exactly the bound
        res = _res(gpu)
        _append(zs, False, dev.data_ptr() + used, host.size - used, d_sizes.data_ptr() + 4 * k, len(S) - k, img,
                _res(gpu, (size, k)), k, res, capacity=need)
        torch.cuda.synchronize()
        want = _pieces_file(zs, host, S, 0, False)
        assert _tuple(res) == (len(want), len(S), sum(S[k:])) and img.file(len(want)) == want
    zimg, zsize, zprev = _built(zs, gpu, True, k, 3)
    refused(zimg, zprev, zs.IMAGE_BAD_IMAGE, zstd=False)
    refused(zimg, _res(gpu, (zsize + 1, k)), zs.IMAGE_BAD_IMAGE, zstd=True)
    refused(zimg, zprev, zs.IMAGE_BAD_IMAGE, zstd=True, flags=CK)


@pytest.mark.parametrize("zstd", [False, True])
def test_restore_and_poisoned_chain(gpu, zs, zstd):
    """A piece list found invalid after earlier batches overwrote the old
    table: the old table comes back, the old file is byte for byte there, and
    the next call works.  A failed call's d_result as the next d_prev: refused,
    nothing written."""
    import torch
    host, dev, d_sizes = _source(zs, gpu)
    k = 3
    used = sum(S[:k])
    rest = S[k:]
    zero = list(rest)
    zero[1] = 0
    d_zero = torch.from_numpy(np.asarray(zero, np.uint32).view(np.int32).copy()).to(gpu)
    q = torch.cuda.Stream(device=gpu)
    for at, (sizes_ptr, src_len) in zip((1, 3), ((d_zero.data_ptr(), host.size - used),
                                                  (d_sizes.data_ptr() + 4 * k, sum(rest) - 1))):
        img, size, prev = _built(zs, gpu, zstd, k, at)
        old = img.file(size)
        one = Image(gpu, img.cap, at)                     # the yardstick: one build over S
        r_one = _res(gpu)
        _build(zs, zstd, dev.data_ptr(), host.size, d_sizes.data_ptr(), len(S), one, r_one)
        res, res2, res3 = _res(gpu), _res(gpu), _res(gpu)
        with torch.cuda.stream(q):
            # one piece per batch: the failure shows in the second or the last batch
            _append(zs, zstd, dev.data_ptr() + used, src_len, sizes_ptr, len(rest), img, prev, k, res,
                    q.cuda_stream, batch=TOP)
        q.synchronize()
        assert _tuple(res)[0] == zs.IMAGE_BAD_PIECES
        assert img.file(size) == old
        after = img.t.clone()
        torch.cuda.synchronize()
        # the poisoned chain: the failure code is no size
        _append(zs, zstd, dev.data_ptr() + used, host.size - used, d_sizes.data_ptr() + 4 * k, len(rest), img, res, k,
                res2, q.cuda_stream)
        _append(zs, zstd, dev.data_ptr() + used, host.size - used, d_sizes.data_ptr() + 4 * k, len(rest), img, res2, k,
                res3, q.cuda_stream)
        q.synchronize()
        assert _tuple(res2)[0] == zs.IMAGE_BAD_IMAGE and _tuple(res3)[0] == zs.IMAGE_BAD_IMAGE
        assert torch.equal(img.t, after)
        # given the old size again, the valid append succeeds
        _append(zs, zstd, dev.data_ptr() + used, host.size - used, d_sizes.data_ptr() + 4 * k, len(rest), img, prev, k,
                res, q.cuda_stream, batch=TOP)
        q.synchronize()
        want_size = _tuple(r_one)[0]
        assert _tuple(res) == (want_size, len(S), sum(rest))
        assert img.file(want_size) == one.file(want_size)
        if not zstd:
            assert img.file(want_size) == _pieces_file(zs, host, S, 0, False)
