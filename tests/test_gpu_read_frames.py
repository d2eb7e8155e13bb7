"""zsk_read_frames_indirect on the GPU: whole frames of a device image picked by
an index list in device memory, planned by the kernels of
csrc/frame_list_plan.hip and decoded straight into the caller's buffer, packed
or in padded rows, on the caller's stream.

Expected bytes are numpy slices of the golden files' payloads or of the records
the test itself wrote; expected offsets, results and counts are zseek_hip.h's
arithmetic computed in numpy here -- never the library's own output.  Every test
runs on a non-default torch stream, allocates and fills every tensor before the
call under test, and checks a guard region behind buf_size afterwards."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import golden_file

pytestmark = pytest.mark.gpu

SENT = 0xA5
UNSET = -7777          # what d_result and d_offsets hold before a call
GUARD = 4096
RECORDS = [1, 2, 63, 64, 65, 4095, 4096, 65535, 65536, 65537, 200000]


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
class _Open:
    """A reader over the image's bytes in device memory (at an odd address)."""

    def __init__(self, zs, gpu, img: bytes, census=True):
        import torch
        at = 2
        self.keep = torch.full((at + len(img) + 64,), SENT, dtype=torch.uint8, device=gpu)
        self.keep[at: at + len(img)].copy_(torch.from_numpy(np.frombuffer(img, np.uint8).copy()))
        torch.cuda.synchronize()
        self.r = zs.Reader.open_device(self.keep.data_ptr() + at, len(img), 0)
        if census and self.r.type == zs.ZSEEK_ZSTD:
            self.r.zstd_census()

    def __enter__(self):
        return self.r

    def __exit__(self, *exc):
        self.r.close()


class _Bufs:
    """The index list, the destination (with a guard region behind buf_size),
    the offsets and the results in device memory, all filled before the call."""

    def __init__(self, gpu, idx, buf_size):
        import torch
        self.n, self.buf_size = len(idx), buf_size
        self.h_idx = np.asarray(idx, np.int64).reshape(-1)
        self.idx = torch.from_numpy(self.h_idx.copy()).to(gpu) if self.n else torch.zeros(1, dtype=torch.int64,
                                                                                          device=gpu)
        self.buf = torch.full((buf_size + GUARD,), SENT, dtype=torch.uint8, device=gpu)
        self.off = torch.full((self.n + 1,), UNSET, dtype=torch.int64, device=gpu)
        self.res = torch.full((self.n + 1,), UNSET, dtype=torch.int64, device=gpu)
        assert self.buf.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def host(self):
        """-> (destination bytes, offsets, results) after checking the guard and the list."""
        b = self.buf.cpu().numpy()
        assert (b[self.buf_size:] == SENT).all(), "a write past buf_size"
        if self.n:
            assert (self.idx.cpu().numpy() == self.h_idx).all(), "the list was written"
        return b[: self.buf_size], self.off.cpu().numpy().tolist(), self.res.cpu().numpy().tolist()

    def untouched(self):
        assert (self.buf.cpu().numpy() == SENT).all()
        assert (self.off.cpu().numpy() == UNSET).all() and (self.res.cpu().numpy() == UNSET).all()


def _call(zs, r, B, stream, stride=0, n=None, d_idx=True, d_buf=True, d_off=True, d_res=True, buf_size=None, skew=0):
    """The C entry itself: -> (return value, errbuf text)."""
    err = C.create_string_buffer(b"untouched", 80)
    ret = zs.lib().zsk_read_frames_indirect(r.handle if r is not None else None, B.idx.data_ptr() if d_idx else None,
                                            B.n if n is None else n, stride,
                                            B.buf.data_ptr() + skew if d_buf else None,
                                            B.buf_size if buf_size is None else buf_size,
                                            B.off.data_ptr() if d_off else None,
                                            B.res.data_ptr() if d_res else None, stream.cuda_stream, err)
    return ret, err.value.decode()


class _Expect:
    """The header's arithmetic for one list: offsets, each slot's result when
    every frame decodes (`want`), the count."""

    def __init__(self, idx, sizes, stride, buf_size):
        idx = np.asarray(idx, np.int64).reshape(-1)
        n, nframes = len(idx), len(sizes)
        sizes = np.asarray(sizes, np.int64)
        self.valid = (idx >= 0) & (idx < nframes)
        self.frame = np.where(self.valid, idx, 0)
        self.size = np.where(self.valid, sizes[self.frame], 0)
        packed = np.concatenate([[0], np.cumsum(self.size)])
        self.offsets = (np.arange(n + 1) * stride if stride else packed).tolist()
        self.want = []
        for i in range(n):
            s, at = int(self.size[i]), self.offsets[i]
            if not self.valid[i]:
                self.want.append(-1)
            elif s == 0:
                self.want.append(0)
            elif at + s > buf_size or (stride and s > stride):
                self.want.append(-1)
            else:
                self.want.append(s)

    def results(self, failed=()):
        res = [-1 if i in failed and w > 0 else w for i, w in enumerate(self.want)]
        return res + [sum(x >= 0 for x in res)]

    def check_bytes(self, buf, data, d_off, failed=()):
        """Delivered regions hold the frames' bytes; everything else still the
        sentinel, except a failed slot's own region, which is unspecified."""
        payload = np.frombuffer(data, np.uint8)
        want = np.full(buf.size, SENT, np.uint8)
        look = np.ones(buf.size, bool)
        for i, w in enumerate(self.want):
            if w <= 0:
                continue
            at, f = self.offsets[i], int(self.frame[i])
            if i in failed:
                look[at: at + w] = False
            else:
                want[at: at + w] = payload[int(d_off[f]): int(d_off[f]) + w]
        bad = np.nonzero((buf != want) & look)[0]
        assert bad.size == 0, (bad[:8], len(bad))


def _read(zs, gpu, r, S, idx, sizes, stride=0, buf_size=None):
    """One call and its synchronization: -> (expectation, bytes, offsets, results)."""
    n = len(idx)
    if buf_size is None:
        buf_size = n * stride if stride else int(_Expect(idx, sizes, 0, 0).offsets[-1])
    E = _Expect(idx, sizes, stride, buf_size)
    B = _Bufs(gpu, idx, buf_size)
    assert _call(zs, r, B, S, stride=stride) == (0, "untouched")
    S.synchronize()
    buf, off, res = B.host()
    assert off == E.offsets
    return E, buf, off, res


def _lists(n, nframes, seed):
    """n slots with repeats: shuffled, and reversed."""
    rng = np.random.default_rng(seed)
    base = [int(x) for x in (np.arange(n) * 7 + seed) % nframes]
    return {"shuffled": rng.permutation(base).tolist(), "reversed": sorted(base, reverse=True)}


def _written(zs, oracle, ctype):
    """An image written by the host Writer, one frame per record of RECORDS
    bytes.  -> (image, the source bytes, its prefix sums)."""
    src = oracle.synth(sum(RECORDS), 17)
    d_off = np.concatenate([[0], np.cumsum(RECORDS)])
    w = zs.Writer(ctype, min_frame_size=1)
    for a, b in zip(d_off, d_off[1:]):
        w.write(src[int(a): int(b)].tobytes())
    img = w.close()
    _, got = zs.seek_table_of(np.frombuffer(img, np.uint8))
    assert [int(x) for x in got] == d_off.tolist()           # a frame per record
    return img, src.tobytes(), d_off


def _golden(zs, payloads, name):
    img = golden_file(name)
    _, d_off = zs.seek_table_of(np.frombuffer(img, np.uint8))
    d_off = np.asarray(d_off, np.int64)
    assert int(d_off[-1]) == len(payloads[name])
    return img, payloads[name], d_off


# ---------------------------------------------------------------------------
# 1. the bytes, offsets and results of every layout, list length and order
# ---------------------------------------------------------------------------
IMAGES = ["lz4_odd_frames", "lz4_4k_direct", "lz4_1m_direct", "zstd_64k_direct", "written_lz4", "written_zstd"]


def _image(zs, oracle, payloads, name):
    if name.startswith("written"):
        return _written(zs, oracle, zs.ZSEEK_LZ4 if name.endswith("lz4") else zs.ZSEEK_ZSTD)
    return _golden(zs, payloads, name)


@pytest.mark.parametrize("mode", ["packed", "rows"])
@pytest.mark.parametrize("name", IMAGES)
def test_frames_by_index(gpu, zs, oracle, payloads, name, mode):
    import torch
    img, data, d_off = _image(zs, oracle, payloads, name)
    sizes = np.diff(d_off)
    nframes, big = len(sizes), int(sizes.max())
    if name == "lz4_odd_frames":
        assert nframes == 151 and (sizes[:150] == 1333).all() and sizes[150] == 51
    S = torch.cuda.Stream(device=gpu)
    # (the 1 MiB frames: 300 rows of them would be 300 MiB of sentinel to compare)
    lengths = (1, 5, 64, 65) if big > (1 << 19) and mode == "rows" else (1, 5, 64, 65, 300)
    with _Open(zs, gpu, img) as r:
        if big > (1 << 19):
            r.set_batch_bytes(1 << 30)
        stride = big + 3 if mode == "rows" else 0            # odd rows: every row starts unaligned
        for n in lengths:
            for order, idx in _lists(n, nframes, n).items():
                if n >= 64 and big > (1 << 19) and order == "reversed":
                    continue
                E, buf, off, res = _read(zs, gpu, r, S, idx, sizes, stride=stride)
                assert res == E.results() and res[-1] == n, (n, order)
                assert res[:-1] == [int(sizes[f]) for f in idx]
                E.check_bytes(buf, data, d_off)


def test_python_wrappers(gpu, zs, payloads):
    import torch
    name = "lz4_odd_frames"
    img, data, d_off = _golden(zs, payloads, name)
    with _Open(zs, gpu, img) as r:
        buf, off, res = r.read_frames([150, 0, 7, 999, 7])
        assert off.cpu().tolist() == [0, 51, 1384, 2717, 2717, 4050]
        assert res.cpu().tolist() == [51, 1333, 1333, -1, 1333, 4]
        h = buf.cpu().numpy().tobytes()
        assert h == data[150 * 1333:] + data[:1333] + data[7 * 1333: 8 * 1333] * 2
        rows, off, res = r.read_frames(torch.tensor([3, 150], device=gpu), stride=1400)
        assert rows.shape == (2, 1400) and res.cpu().tolist() == [1333, 51, 2]
        assert rows[0, :1333].cpu().numpy().tobytes() == data[3 * 1333: 4 * 1333]
        assert rows[1, :51].cpu().numpy().tobytes() == data[150 * 1333:]
        buf, off, res = r.read_frames([])
        assert buf.numel() == 0 and off.cpu().tolist() == [0] and res.cpu().tolist() == [0]


# ---------------------------------------------------------------------------
# 2. buffers and rows that are too small, indices that are no frame
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lz4_odd_frames", "zstd_64k_direct", "written_lz4", "written_zstd"])
def test_buffer_one_byte_short(gpu, zs, oracle, payloads, name):
    import torch
    img, data, d_off = _image(zs, oracle, payloads, name)
    sizes = np.diff(d_off)
    nframes = len(sizes)
    S = torch.cuda.Stream(device=gpu)
    idx = _lists(40, nframes, 3)["shuffled"]
    total = int(sizes[idx].sum())
    with _Open(zs, gpu, img) as r:
        E, buf, off, res = _read(zs, gpu, r, S, idx, sizes, buf_size=total - 1)
        assert off[-1] == total                              # the size a caller needs, whatever buf_size is
        assert res[:-1] == [int(sizes[f]) for f in idx[:-1]] + [-1] and res[-1] == 39
        assert res == E.results()
        E.check_bytes(buf, data, d_off)
        # cut in the middle: the last fitting slot is delivered, the rest are not
        cut = off[18] - 1                                    # slot 17 is one byte short
        E, buf, off, res = _read(zs, gpu, r, S, idx, sizes, buf_size=cut)
        assert off[-1] == total and res == E.results()
        assert all(x > 0 for x in res[:17]) and res[17: -1] == [-1] * 23 and res[-1] == 17
        E.check_bytes(buf, data, d_off)


@pytest.mark.parametrize("name", ["written_lz4", "written_zstd", "lz4_odd_frames"])
def test_row_one_byte_too_narrow(gpu, zs, oracle, payloads, name):
    import torch
    img, data, d_off = _image(zs, oracle, payloads, name)
    sizes = np.diff(d_off)
    nframes, big = len(sizes), int(sizes.max())
    S = torch.cuda.Stream(device=gpu)
    idx = _lists(30, nframes, 5)["shuffled"]
    idx[7] = nframes - 1                                     # (the odd file's short tail)
    assert any(sizes[f] == big for f in idx) and any(sizes[f] < big for f in idx)
    with _Open(zs, gpu, img) as r:
        E, buf, off, res = _read(zs, gpu, r, S, idx, sizes, stride=big - 1)
        assert res[:-1] == [-1 if sizes[f] == big else int(sizes[f]) for f in idx]
        assert res == E.results()
        E.check_bytes(buf, data, d_off)                      # a frame is never truncated to its row
        # the last row cut off by buf_size
        E, buf, off, res = _read(zs, gpu, r, S, idx, sizes, stride=big, buf_size=29 * big + int(sizes[idx[-1]]) - 1)
        assert res[-2] == -1 and res[:-2] == [int(sizes[f]) for f in idx[:-1]] and res == E.results()
        E.check_bytes(buf, data, d_off)


@pytest.mark.parametrize("name", ["lz4_4k_direct", "zstd_64k_direct"])
def test_invalid_indices_in_the_middle(gpu, zs, oracle, payloads, name):
    import torch
    img, data, d_off = _image(zs, oracle, payloads, name)
    sizes = np.diff(d_off)
    nframes = len(sizes)
    S = torch.cuda.Stream(device=gpu)
    idx = [2, -1, 0, nframes, nframes - 1, 2**40, 1, -2**63, 2, 2]
    with _Open(zs, gpu, img) as r:
        for stride in (0, int(sizes.max())):
            E, buf, off, res = _read(zs, gpu, r, S, idx, sizes, stride=stride)
            assert [res[i] for i in (1, 3, 5, 7)] == [-1] * 4 and res[-1] == 6 and res == E.results()
            E.check_bytes(buf, data, d_off)
        E, buf, off, res = _read(zs, gpu, r, S, [-5, nframes + 1] * 40, sizes)   # nothing valid at all
        assert res == [-1] * 80 + [0] and off == [0] * 81


# ---------------------------------------------------------------------------
# 3. zstd: the census is the switch
# ---------------------------------------------------------------------------
def test_zstd_needs_the_census(gpu, zs, payloads):
    import torch
    img, data, d_off = _golden(zs, payloads, "zstd_64k_direct")
    sizes = np.diff(d_off)
    S = torch.cuda.Stream(device=gpu)
    idx = [3, 1, 3]
    with _Open(zs, gpu, img, census=False) as r:
        B = _Bufs(gpu, idx, int(sizes[idx].sum()))
        assert _call(zs, r, B, S) == (-1, "frame-list read: zstd is not supported")
        S.synchronize()
        B.untouched()
        assert r.gpu_stats()["batches"] == 0
        r.zstd_census()
        E, buf, off, res = _read(zs, gpu, r, S, idx, sizes)
        assert res == [int(sizes[3]), int(sizes[1]), int(sizes[3]), 3]
        E.check_bytes(buf, data, d_off)


# ---------------------------------------------------------------------------
# 4. failed frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lz4_64k_direct", "zstd_64k_direct"])
def test_seek_table_checksum_flipped(gpu, zs, oracle, payloads, name):
    import torch
    plain, data = np.frombuffer(golden_file(name), np.uint8), payloads[name]
    _, d_off = zs.seek_table_of(plain)
    d = [int(x) for x in d_off]
    sizes = np.diff(d)
    sums = np.array([oracle.xxh64(data[d[i]: d[i + 1]]) & 0xFFFFFFFF for i in range(len(d) - 1)], np.uint32)
    sums[5] ^= 1                                             # one wrong word
    bad = zs.with_frame_checksums(plain, sums).tobytes()
    idx = [4, 5, 6, 0, 5, 7]
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, bad) as r:
        r.set_verify_checksums(True)
        E, buf, off, res = _read(zs, gpu, r, S, idx, sizes)
        assert res == E.results(failed={1, 4}) and res[-1] == 4
        E.check_bytes(buf, data, d, failed={1, 4})
        r.set_verify_checksums(False)                        # verification off: all delivered
        E, buf, off, res = _read(zs, gpu, r, S, idx, sizes, stride=65536 + 16)
        assert res == E.results() and res[-1] == 6
        E.check_bytes(buf, data, d)


@pytest.mark.parametrize("case", ["frame_magic", "header_checksum", "1m_block4_size_huge"])
def test_corrupt_frame(gpu, zs, golden, payloads, case):
    """One frame corrupted as the golden corruption records say: its slots get
    -1, its neighbours are intact, nothing outside its own regions is written."""
    import torch
    rec = golden["corrupt"][case]
    name = rec.get("base") or "lz4_64k_direct"
    data = payloads[name]
    img = bytearray(golden_file(name))
    c_off, d_off = zs.seek_table_of(np.frombuffer(bytes(img), np.uint8))
    for at, v in rec["mutations"]:
        img[at] = v
    bad = int(np.searchsorted(c_off, rec["mutations"][0][0], side="right") - 1)
    d = [int(x) for x in d_off]
    sizes = np.diff(d)
    nframes = len(sizes)
    a, b = d[bad], d[bad + 1]
    # the goldens record the frame as failing for a cached read
    assert [q for q in rec["results"] if q["cache"] >= 1 and q["ret"] != "hang" and q["ret"] < 0
            and a <= q["offset"] < b]
    idx = [(bad + 1) % nframes, bad, (bad - 1) % nframes, bad, (bad + 2) % nframes]
    failed = {i for i, f in enumerate(idx) if f == bad}
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, bytes(img)) as r:
        for stride in (0, int(sizes.max()) + 5):
            E, buf, off, res = _read(zs, gpu, r, S, idx, sizes, stride=stride)
            print(case, "results", res)
            assert res == E.results(failed=failed) and res[-1] == len(idx) - len(failed)
            E.check_bytes(buf, data, d, failed=failed)


def test_zstd_corrupt_frame(gpu, zs, payloads):
    """frame 3's magic number broken"""
    import torch
    name = "zstd_64k_direct"
    img = bytearray(golden_file(name))
    c_off, d_off = zs.seek_table_of(np.frombuffer(bytes(img), np.uint8))
    img[int(c_off[3])] ^= 0xFF
    d = [int(x) for x in d_off]
    sizes = np.diff(d)
    idx = [2, 3, 4, 3, 0]
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, bytes(img)) as r:
        E, buf, off, res = _read(zs, gpu, r, S, idx, sizes)
        assert res == E.results(failed={1, 3}) and res[-1] == 3
        E.check_bytes(buf, payloads[name], d, failed={1, 3})


# ---------------------------------------------------------------------------
# 5. stream order, calls in flight, counters
# ---------------------------------------------------------------------------
def test_list_made_on_the_stream_and_a_consumer_behind(gpu, zs, payloads):
    """On one stream: the list is computed by torch ops, the read, copies of
    the bytes, offsets and results, then everything is overwritten; one
    synchronize.  The copies hold the payload, so the read saw the list the
    producer wrote and ran before the consumer."""
    import torch
    name = "lz4_odd_frames"
    img, data, d_off = _golden(zs, payloads, name)
    sizes = np.diff(d_off)
    n = 200
    want_idx = [(k * 37 + 11) % 151 for k in range(n)]
    total = int(sizes[want_idx].sum())
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, img) as r:
        d_idx = torch.full((n,), 10**9, dtype=torch.int64, device=gpu)   # garbage until the producer runs
        k = torch.arange(n, dtype=torch.int64, device=gpu)
        d_buf = torch.zeros(total + GUARD, dtype=torch.uint8, device=gpu)
        d_copy = torch.zeros(total + GUARD, dtype=torch.uint8, device=gpu)
        d_off_t = torch.full((n + 1,), UNSET, dtype=torch.int64, device=gpu)
        d_res = torch.full((n + 1,), UNSET, dtype=torch.int64, device=gpu)
        d_off_copy, d_res_copy = torch.zeros_like(d_off_t), torch.zeros_like(d_res)
        torch.cuda.synchronize()
        err = C.create_string_buffer(b"untouched", 80)
        with torch.cuda.stream(S):
            d_buf.fill_(SENT)
            d_idx.copy_(k)
            d_idx.mul_(37).add_(11).remainder_(151)
            ret = zs.lib().zsk_read_frames_indirect(r.handle, d_idx.data_ptr(), n, 0, d_buf.data_ptr(), total,
                                                    d_off_t.data_ptr(), d_res.data_ptr(), S.cuda_stream, err)
            d_copy.copy_(d_buf)
            d_off_copy.copy_(d_off_t)
            d_res_copy.copy_(d_res)
            d_buf.zero_()
            d_res.zero_()
        assert (ret, err.value) == (0, b"untouched")
        S.synchronize()
        assert d_idx.cpu().tolist() == want_idx
        E = _Expect(want_idx, sizes, 0, total)
        assert d_off_copy.cpu().tolist() == E.offsets
        assert d_res_copy.cpu().tolist() == E.results() and E.results()[-1] == n
        h = d_copy.cpu().numpy()
        assert (h[total:] == SENT).all()
        E.check_bytes(h[:total], data, d_off)
        assert not d_buf.cpu().numpy().any() and not d_res.cpu().numpy().any()


@pytest.mark.parametrize("name", ["lz4_4k_direct", "zstd_64k_direct"])
def test_four_calls_back_to_back(gpu, zs, payloads, name):
    """More calls than slots and call tables on one stream: the fourth waits
    for the first's slot; all four are correct; the counters."""
    import torch
    img, data, d_off = _golden(zs, payloads, name)
    sizes = np.diff(d_off)
    nframes = len(sizes)
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, img) as r:
        b0 = r.gpu_stats()
        sets = []
        for k, (n, stride) in enumerate([(70, 0), (3, int(sizes.max()) + 1), (130, 0), (64, 0)]):
            idx = _lists(n, nframes, 40 + k)["shuffled"]
            buf_size = n * stride if stride else int(sizes[idx].sum())
            sets.append((idx, stride, _Expect(idx, sizes, stride, buf_size), _Bufs(gpu, idx, buf_size)))
        rets = [_call(zs, r, B, S, stride=stride) for _, stride, _, B in sets]
        assert rets == [(0, "untouched")] * 4
        S.synchronize()
        for idx, stride, E, B in sets:
            buf, off, res = B.host()
            assert off == E.offsets and res == E.results() and res[-1] == len(idx)
            E.check_bytes(buf, data, d_off)
        gs = r.gpu_stats()
        assert gs["batches"] == b0["batches"] + 4 and gs["bytes_uploaded"] == 0
        assert (gs["frames_decoded"], gs["bytes_decoded"]) == (b0["frames_decoded"], b0["bytes_decoded"])
        assert r.stats()["cached_frames"] == 0


def test_one_call_counts_one_batch(gpu, zs, payloads):
    import torch
    img, data, d_off = _golden(zs, payloads, "lz4_4k_direct")
    sizes = np.diff(d_off)
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, img) as r:
        b0 = r.gpu_stats()
        _read(zs, gpu, r, S, [1, 2, 3], sizes)
        gs = r.gpu_stats()
        assert gs["batches"] == b0["batches"] + 1 and gs["bytes_uploaded"] == 0


# ---------------------------------------------------------------------------
# 6. refusals: -1, the text, nothing queued, nothing written
# ---------------------------------------------------------------------------
def test_refusals(gpu, zs, payloads):
    import torch
    S = torch.cuda.Stream(device=gpu)
    idx = [3, 1]
    B = _Bufs(gpu, idx, 2 * 65536)
    assert _call(zs, None, B, S) == (-1, "invalid reader")
    with zs.Reader(golden_file("lz4_64k_direct"), 0) as r:   # a host image
        assert _call(zs, r, B, S) == (-1, "frame-list read: needs a device image")
    with _Open(zs, gpu, golden_file("lz4_64k_direct")) as r:
        for kw in (dict(d_idx=False), dict(d_res=False), dict(d_off=False)):
            ret, err = _call(zs, r, B, S, **kw)
            assert ret == -1 and err not in ("", "untouched"), kw
        assert _call(zs, r, B, S, d_off=False, n=0) == (-1, "frame-list read: the packed layout needs d_offsets")
        assert _call(zs, r, B, S, d_buf=False) == (-1, "invalid buffer")
        for skew in (1, 8):                                  # d_buf not 16-byte aligned
            ret, err = _call(zs, r, B, S, skew=skew, buf_size=100)
            assert ret == -1 and "16-byte aligned" in err
        # d_offsets / d_result off their words
        err = C.create_string_buffer(b"untouched", 80)
        for o_skew, r_skew in ((4, 0), (0, 4), (1, 0)):
            assert zs.lib().zsk_read_frames_indirect(r.handle, B.idx.data_ptr(), 2, 0, B.buf.data_ptr(), 2 * 65536,
                                                     B.off.data_ptr() + o_skew, B.res.data_ptr() + r_skew,
                                                     S.cuda_stream, err) == -1
            assert b"misaligned" in err.value
        # nidx x the largest frame (or the stride) against the batch size
        r.set_batch_bytes(4 * 65536)
        B5 = _Bufs(gpu, [0, 1, 2, 3, 4], 5 * 65536)
        assert _call(zs, r, B5, S) == (-1, "frame-list read: the list exceeds the batch size")
        assert _call(zs, r, B, S, stride=2 * 65536 + 1) == (-1, "frame-list read: the list exceeds the batch size")
        r.set_batch_bytes(1 << 40)
        ret, err = _call(zs, r, B, S, stride=1 << 31)        # 2 x 2 GiB: 4 GiB
        assert (ret, err) == (-1, "frame-list read: the list exceeds 4 GiB")
        r.set_batch_bytes(4 * 65536)
        S.synchronize()
        B.untouched()
        B5.untouched()
        assert r.gpu_stats()["batches"] == 0
        B4 = _Bufs(gpu, [0, 1, 2, 3], 4 * 65536)             # ... and what just fits
        assert _call(zs, r, B4, S) == (0, "untouched")
        S.synchronize()
        assert B4.res.cpu().tolist() == [65536] * 4 + [4]
        # an empty list: d_result[0] = 0 and d_offsets[0] = 0 alone
        B = _Bufs(gpu, idx, 2 * 65536)
        assert _call(zs, r, B, S, n=0) == (0, "untouched")
        assert _call(zs, r, B, S, n=0, d_idx=False, d_res=False, stride=8, d_off=False) == (0, "untouched")
        S.synchronize()
        assert B.res.cpu().tolist() == [0, UNSET, UNSET] and B.off.cpu().tolist() == [0, UNSET, UNSET]
        assert (B.buf.cpu().numpy() == SENT).all()
        # a buffer of no bytes: nothing fits, the total is still reported
        B = _Bufs(gpu, idx, 2 * 65536)
        assert _call(zs, r, B, S, d_buf=False, buf_size=0) == (0, "untouched")
        S.synchronize()
        assert B.res.cpu().tolist() == [-1, -1, 0] and B.off.cpu().tolist() == [0, 65536, 131072]
        assert (B.buf.cpu().numpy() == SENT).all()
    # a seek table that reaches past the image (frame 3's cSize entry inflated
    # by the file's size: 8-byte entries before the 9-byte footer)
    img = bytearray(golden_file("lz4_64k_direct"))
    n = int.from_bytes(img[-9:-5], "little")
    at = len(img) - 9 - 8 * (n - 3)
    assert img[-5] == 0
    img[at: at + 4] = (int.from_bytes(img[at: at + 4], "little") + len(img)).to_bytes(4, "little")
    B = _Bufs(gpu, idx, 2 * 65536)
    with _Open(zs, gpu, bytes(img)) as r:
        assert _call(zs, r, B, S) == (-1, "unexpected EOF")
        S.synchronize()
        B.untouched()


def test_refuses_a_capturing_stream(gpu, zs):
    """Nothing of the call may end up in a graph.  (The graph is never replayed.)"""
    import torch
    S = torch.cuda.Stream(device=gpu)
    idx = [3, 1]
    B = _Bufs(gpu, idx, 2 * 65536)
    x = torch.zeros(16, device=gpu)
    with _Open(zs, gpu, golden_file("lz4_64k_direct")) as r:
        assert _call(zs, r, B, S) == (0, "untouched")        # (buffers exist: the refusal is not an allocation's)
        S.synchronize()
        B = _Bufs(gpu, idx, 2 * 65536)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=S):
            got = _call(zs, r, B, S)
            x.add_(1)
        assert got == (-1, "frame-list read: stream is capturing")
        del g
        torch.cuda.synchronize()
        B.untouched()
        assert r.gpu_stats()["batches"] == 1
