"""zsk_preadv_device_indirect on the GPU: a vectored read of a device image
whose range list is in device memory, planned by the kernels of
csrc/range_plan_dev.hip, decoded in place, gathered and answered on the
caller's stream.

Expected bytes are numpy slices of the golden files' payloads; expected results
are the arithmetic zseek_hip.h states (min(count, size - offset), the bytes
before the first failed frame, -1, the plan's flags) or come from the golden
corruption records -- never the library's own output.  Every test runs on a
non-default torch stream and allocates every tensor before the call under
test."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import golden_file

pytestmark = pytest.mark.gpu

SENT = 0xA5
UNSET = -7777          # what d_result holds before a call
OVERFLOW, SPAN = -2, -3


# ---------------------------------------------------------------------------
# helpers (own copies of test_gpu_preadv_async.py's)
# ---------------------------------------------------------------------------
def _ranges_for(d_off, seed):
    """test_gpu_preadv_async.py's 257 (offset, count) ranges in shuffled
    order: the named edge cases, then random ones."""
    rng = np.random.default_rng(seed)
    d = [int(x) for x in d_off]
    size, n = d[-1], len(d) - 1
    f = min(1, n - 1)
    fs = d[f + 1] - d[f]
    rg = [(d[f] + k * (fs // 7), 1 + fs // 11) for k in range(5)]          # several in one frame
    rg += [(d[f] + 100, 333), (d[f] + 100, 333)]                            # duplicates
    rg += [(d[f] + 5, 0), (0, 0)]                                           # zero-length
    rg += [(d[2] - 100, 100), (d[1] - 1, 1)]                                # ending exactly at a frame boundary
    rg += [(d[1] - 10, d[2] - d[1] + 20)]                                   # spanning three frames
    rg += [(0, size)]                                                       # the whole file
    rg += [(size - 1, 10)]                                                  # starting in the last byte
    rg += [(size, 10), (size + 100, 10)]                                    # at and past EOF
    rg += [(size - 500, 1000)]                                              # count running past EOF
    while len(rg) < 257:
        off = int(rng.integers(0, size))
        cnt = int(rng.integers(1, 100000)) if len(rg) % 16 == 0 else int(rng.integers(1, 3000))
        rg.append((off, cnt))
    return [rg[i] for i in rng.permutation(len(rg))], size


def _layout(zs, ranges):
    """RANGE_DTYPE array with disjoint destinations at odd offsets, a gap
    after every range; -> (array, buffer bytes)."""
    rg = np.zeros(len(ranges), zs.RANGE_DTYPE)
    at = 3
    for i, (off, cnt) in enumerate(ranges):
        rg[i]["offset"], rg[i]["count"], rg[i]["dst_off"] = off, cnt, at
        at += cnt + 1 + (i % 7)
    assert any(int(x) % 4 for x in rg["dst_off"])
    rg["result"] = 424242                     # the call must not write it
    return rg, at + 16


def _full(ranges, size):
    return [min(c, size - o) if o < size and c else 0 for o, c in ranges]


def _check(rg, buf, data, results):
    """Every byte up to each result the payload's, the gaps (and everything
    else) still the sentinel; bytes of a destination past its result are
    unspecified and not looked at."""
    want = np.full(buf.size, SENT, np.uint8)
    look = np.ones(buf.size, bool)
    payload = np.frombuffer(data, np.uint8)
    for q, res in zip(rg, results):
        off, cnt, dst = int(q["offset"]), int(q["count"]), int(q["dst_off"])
        got = max(res, 0)
        want[dst: dst + got] = payload[off: off + got]
        look[dst + got: dst + cnt] = False
    bad = np.nonzero((buf != want) & look)[0]
    assert bad.size == 0, (bad[:8], len(bad))


def _place(gpu, img: bytes, at: int = 2):
    """The image at byte offset `at` of a device tensor.  -> (tensor, pointer)."""
    import torch
    t = torch.full((at + len(img) + 64,), SENT, dtype=torch.uint8, device=gpu)
    t[at: at + len(img)].copy_(torch.from_numpy(np.frombuffer(img, np.uint8).copy()))
    torch.cuda.synchronize()
    return t, t.data_ptr() + at


class _Open:
    """A reader over the image's bytes in device memory."""

    def __init__(self, zs, gpu, img: bytes):
        self.keep, ptr = _place(gpu, img)
        self.r = zs.Reader.open_device(ptr, len(img), 0)

    def __enter__(self):
        return self.r

    def __exit__(self, *exc):
        self.r.close()


class _Bufs:
    """The destination (with a guard region behind buf_size), the results and
    the range list in device memory, all filled before the call."""

    def __init__(self, gpu, rg, nbytes, guard=64):
        import torch
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + guard,), SENT, dtype=torch.uint8, device=gpu)
        self.res = torch.full((len(rg) + 1,), UNSET, dtype=torch.int64, device=gpu)
        self.rg = torch.from_numpy(rg.view(np.uint8).copy()).to(gpu)
        torch.cuda.synchronize()

    def host(self):
        """-> (destination bytes, results) after checking the guard and the list."""
        b = self.buf.cpu().numpy()
        assert (b[self.nbytes:] == SENT).all(), "a write past buf_size"
        return b[: self.nbytes], self.res.cpu().numpy().tolist()


def _call(zs, r, B, n, max_frames, stream, d_buf=True, d_rg=True, d_res=True, buf_size=None):
    """The C entry itself: -> (return value, errbuf text)."""
    err = C.create_string_buffer(b"untouched", 80)
    ret = zs.lib().zsk_preadv_device_indirect(r.handle, B.buf.data_ptr() if d_buf else None,
                                              B.nbytes if buf_size is None else buf_size,
                                              B.rg.data_ptr() if d_rg else None, n, max_frames,
                                              B.res.data_ptr() if d_res else None, stream.cuda_stream, err)
    return ret, err.value.decode()


def _list_unchanged(B, rg):
    assert B.rg.cpu().numpy().tobytes() == rg.tobytes()      # `result` fields included


# ---------------------------------------------------------------------------
# 1. parity with the host-planned read's contract
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lz4_64k_direct", "lz4_4k_direct", "lz4_1m_direct", "lz4f_content_checksum"])
def test_indirect_matches_payload(gpu, zs, payloads, name):
    import torch
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name)) as r:
        _, d_off = r.frames()
        nframes = len(d_off) - 1
        ranges, size = _ranges_for(d_off, 11)
        assert len(ranges) == 257 and size == len(payloads[name])
        rg, nbytes = _layout(zs, ranges)
        B = _Bufs(gpu, rg, nbytes)
        b0 = r.gpu_stats()
        assert _call(zs, r, B, len(rg), nframes, S) == (0, "untouched")
        S.synchronize()
        buf, res = B.host()
        assert res[:-1] == _full(ranges, size)
        assert res[-1] == len(ranges)
        _check(rg, buf, payloads[name], res[:-1])             # the gaps still hold the sentinel
        _list_unchanged(B, rg)
        gs = r.gpu_stats()
        assert gs["batches"] == b0["batches"] + 1
        # the host never learns what the ranges touched
        assert (gs["frames_decoded"], gs["bytes_decoded"], gs["bytes_uploaded"]) == (0, 0, 0)
        assert r.stats()["cached_frames"] == 0


def test_indirect_python_wrapper(gpu, zs, payloads):
    import torch
    data = payloads["lz4_64k_direct"]
    S = torch.cuda.Stream(device=gpu)
    rg = np.zeros(2, zs.RANGE_DTYPE)
    rg["offset"], rg["count"], rg["dst_off"] = [131070, 9], [4, 3], [1, 33]
    B = _Bufs(gpu, rg, 64)
    with _Open(zs, gpu, golden_file("lz4_64k_direct")) as r:
        assert r.preadv_device_indirect(B.buf.data_ptr(), 64, B.rg.data_ptr(), 2, 3, B.res.data_ptr(),
                                        S.cuda_stream) is None
        S.synchronize()
        h, res = B.host()
        assert res == [4, 3, 2]
        assert h[1:5].tobytes() == data[131070:131074] and h[33:36].tobytes() == data[9:12]
        assert (h[5:33] == SENT).all() and h[0] == SENT and (h[36:] == SENT).all()
        with pytest.raises(zs.ZseekError):
            r.preadv_device_indirect(B.buf.data_ptr(), 64, B.rg.data_ptr(), 2, 0, B.res.data_ptr(), S.cuda_stream)


# ---------------------------------------------------------------------------
# 2. padding descriptors and the decoder's routes (<= 64 frames: the one-frame
#    route; one descriptor: no plan launch at all)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_frames", [1, 64, 65, 74])
def test_indirect_one_touched_frame_and_padding(gpu, zs, payloads, max_frames):
    import torch
    name = "lz4_4k_direct"
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name)) as r:
        _, d_off = r.frames()
        d = [int(x) for x in d_off]
        assert len(d) - 1 == 74
        a, b = d[37], d[38]
        ranges = [(a, b - a), (a + 5, 100), (a + 1, 1), (b - 1, 1), (a + 200, 0)]
        rg, nbytes = _layout(zs, ranges)
        B = _Bufs(gpu, rg, nbytes)
        assert _call(zs, r, B, len(rg), max_frames, S) == (0, "untouched")
        S.synchronize()
        buf, res = B.host()
        assert res == [b - a, 100, 1, 1, 0, 5]
        _check(rg, buf, payloads[name], res[:-1])


def test_indirect_every_frame_touched(gpu, zs, payloads):
    import torch
    name = "lz4_4k_direct"
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name)) as r:
        _, d_off = r.frames()
        d = [int(x) for x in d_off]
        size = d[-1]
        # pieces that tile the file, cut inside frames, in reverse order
        cuts = [0] + [d[k] + 7 * k for k in range(1, 74, 3)] + [size]
        ranges = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)][::-1]
        rg, nbytes = _layout(zs, ranges)
        B = _Bufs(gpu, rg, nbytes)
        assert _call(zs, r, B, len(rg), 74, S) == (0, "untouched")
        S.synchronize()
        buf, res = B.host()
        assert res == [c for _, c in ranges] + [len(ranges)]
        _check(rg, buf, payloads[name], res[:-1])


# ---------------------------------------------------------------------------
# 3. ranges made on the stream, a consumer behind the call, no host wait
# ---------------------------------------------------------------------------
def test_indirect_ranges_made_on_the_stream(gpu, zs, payloads):
    """On one stream: the list is computed by torch ops, fill(sentinel), the
    read, copies of the bytes and the results, then everything is overwritten;
    one synchronize.  The copies hold the payload and the results, so the read
    saw the list the producer wrote and ran before the consumer."""
    import torch
    name = "lz4_64k_direct"
    data = payloads[name]
    size = len(data)
    n = 200
    S = torch.cuda.Stream(device=gpu)
    # what the producer computes: offset = (k * 7919 + 13) * 37 % (size - 700), count = 100 + 3 k, dst = 5 + 701 k
    want = [(((k * 7919 + 13) * 37) % (size - 700), 100 + 3 * k, 5 + 701 * k) for k in range(n)]
    nbytes = 5 + 701 * n
    with _Open(zs, gpu, golden_file(name)) as r:
        d_rg = torch.full((n, 4), 99, dtype=torch.int64, device=gpu)      # garbage until the producer runs
        k = torch.arange(n, dtype=torch.int64, device=gpu)
        d_buf = torch.zeros(nbytes, dtype=torch.uint8, device=gpu)
        d_copy = torch.zeros(nbytes, dtype=torch.uint8, device=gpu)
        d_res = torch.full((n + 1,), UNSET, dtype=torch.int64, device=gpu)
        d_res_copy = torch.full((n + 1,), UNSET, dtype=torch.int64, device=gpu)
        torch.cuda.synchronize()
        err = C.create_string_buffer(b"untouched", 80)
        with torch.cuda.stream(S):
            d_buf.fill_(SENT)
            col = d_rg[:, 0]
            col.copy_(k)
            col.mul_(7919).add_(13).mul_(37).remainder_(size - 700)
            d_rg[:, 1].copy_(k)
            d_rg[:, 1].mul_(3).add_(100)
            d_rg[:, 2].copy_(k)
            d_rg[:, 2].mul_(701).add_(5)
            ret = zs.lib().zsk_preadv_device_indirect(r.handle, d_buf.data_ptr(), nbytes, d_rg.data_ptr(), n, 16,
                                                      d_res.data_ptr(), S.cuda_stream, err)
            d_copy.copy_(d_buf)
            d_res_copy.copy_(d_res)
            d_buf.zero_()
            d_res.zero_()
        assert (ret, err.value) == (0, b"untouched")
        S.synchronize()
        assert d_rg.cpu().numpy()[:, :3].tolist() == [list(q) for q in want]
        assert d_res_copy.cpu().numpy().tolist() == [c for _, c, _ in want] + [n]
        rg = np.zeros(n, zs.RANGE_DTYPE)
        rg["offset"], rg["count"], rg["dst_off"] = zip(*want)
        _check(rg, d_copy.cpu().numpy(), data, [c for _, c, _ in want])
        assert not d_buf.cpu().numpy().any() and not d_res.cpu().numpy().any()


# ---------------------------------------------------------------------------
# 4. more touched frames than max_frames
# ---------------------------------------------------------------------------
def test_indirect_overflow(gpu, zs, payloads):
    import torch
    name = "lz4_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name)) as r:
        _, d_off = r.frames()
        d = [int(x) for x in d_off]
        # frames 1, 2 (one range over the boundary), 5, 9, 9 again, 15: T = 5
        ranges = [(d[2] - 10, 20), (d[5] + 1, 100), (d[9], 50), (d[9] + 60, 5), (d[16] - 7, 100), (3, 0)]
        T = 5
        rg, nbytes = _layout(zs, ranges)
        B = _Bufs(gpu, rg, nbytes)
        assert _call(zs, r, B, len(rg), T - 1, S) == (0, "untouched")
        S.synchronize()
        buf, res = B.host()
        assert res == [-1] * len(ranges) + [OVERFLOW]
        assert (buf == SENT).all()                           # nothing was moved
        B = _Bufs(gpu, rg, nbytes)
        assert _call(zs, r, B, len(rg), T, S) == (0, "untouched")
        S.synchronize()
        buf, res = B.host()
        assert res == [20, 100, 50, 5, 7, 0, len(ranges)]
        _check(rg, buf, payloads[name], res[:-1])


# ---------------------------------------------------------------------------
# 5. a destination that leaves the buffer
# ---------------------------------------------------------------------------
def test_indirect_destination_bounds(gpu, zs, payloads):
    import torch
    name = "lz4_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name)) as r:
        ranges = [(10, 100), (65530, 10), (200000, 50), (70000, 300)]
        rg, nbytes = _layout(zs, ranges)
        nbytes += 64                                         # room for the third range at the buffer's end
        rg[2]["dst_off"] = nbytes - 50                       # ends exactly at buf_size
        B = _Bufs(gpu, rg, nbytes, guard=4096)
        assert _call(zs, r, B, len(rg), 8, S) == (0, "untouched")
        S.synchronize()
        buf, res = B.host()
        assert res == [100, 10, 50, 300, 4]
        _check(rg, buf, payloads[name], res[:-1])
        rg[2]["dst_off"] = nbytes - 49                       # one byte past it
        B = _Bufs(gpu, rg, nbytes, guard=4096)
        assert _call(zs, r, B, len(rg), 8, S) == (0, "untouched")
        S.synchronize()
        buf, res = B.host()                                  # (the guard region kept its sentinel)
        assert res == [100, 10, -1, 300, 3]
        rg2 = rg.copy()
        rg2[2]["count"] = 0                                  # it moved no byte
        _check(rg2, buf, payloads[name], [100, 10, 0, 300])


# ---------------------------------------------------------------------------
# 6. corrupt frames
# ---------------------------------------------------------------------------
def _five_ranges(a, b):
    """Before the failed frame [a, b), ending inside it, starting inside it,
    after it, and the frame itself; -> (ranges, want)."""
    ranges = [(a - 5000, 3000), (a - 300, 1000), (a + 10, (b - a) + 500), (b + 5, 3000), (a, b - a)]
    return ranges, [3000, 300, -1, 3000, -1]


@pytest.mark.parametrize("case", ["frame_magic", "header_checksum", "1m_block4_size_huge"])
def test_indirect_corrupt_frame(gpu, zs, golden, payloads, case):
    import torch
    rec = golden["corrupt"][case]
    name = rec.get("base") or "lz4_64k_direct"
    data = payloads[name]
    img = bytearray(golden_file(name))
    c_off, d_off = zs.seek_table_of(np.frombuffer(bytes(img), np.uint8))
    for at, v in rec["mutations"]:
        img[at] = v
    bad = int(np.searchsorted(c_off, rec["mutations"][0][0], side="right") - 1)
    a, b = int(d_off[bad]), int(d_off[bad + 1])
    size = int(d_off[-1])
    # the goldens record the frame as failing for a cached read
    assert [q for q in rec["results"] if q["cache"] >= 1 and q["ret"] != "hang" and q["ret"] < 0
            and a <= q["offset"] < b]
    if bad > 0:
        ranges, want = _five_ranges(a, b)
    else:                                                    # (the 1 MiB file's first frame: nothing before it)
        ranges = [(a + 10, 100), (b - 5, 10), (b + 5, 3000), (0, size), (b, size - b), (b - 1, 1)]
        want = [-1, -1, 3000, -1, size - b, -1]
    rg, nbytes = _layout(zs, ranges)
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, bytes(img)) as r:
        B = _Bufs(gpu, rg, nbytes)
        assert _call(zs, r, B, len(rg), len(d_off) - 1, S) == (0, "untouched")
        S.synchronize()
        buf, res = B.host()
        print(case, "results", res)
        assert res[:-1] == want
        assert res[-1] == sum(1 for (o, c), w in zip(ranges, want) if w == c)
        _check(rg, buf, data, want)


# ---------------------------------------------------------------------------
# 7. seek-table checksums from the resident table
# ---------------------------------------------------------------------------
def test_indirect_checksums(gpu, zs, oracle, payloads):
    import torch
    name = "lz4_64k_direct"
    plain, data = np.frombuffer(golden_file(name), np.uint8), payloads[name]
    _, d_off = zs.seek_table_of(plain)
    d = [int(x) for x in d_off]
    sums = np.array([oracle.xxh64(data[d[i]: d[i + 1]]) & 0xFFFFFFFF for i in range(len(d) - 1)], np.uint32)
    sums[5] ^= 1                                             # one wrong word
    bad = zs.with_frame_checksums(plain, sums).tobytes()
    ranges, want = _five_ranges(d[5], d[6])
    ranges.append((d[4] + 9, 3 * 65536))                    # frames 4 .. 7: the bytes before frame 5
    want.append(d[5] - d[4] - 9)
    rg, nbytes = _layout(zs, ranges)
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, bad) as r:
        B, B2 = _Bufs(gpu, rg, nbytes), _Bufs(gpu, rg, nbytes)
        r.set_verify_checksums(True)
        assert _call(zs, r, B, len(rg), 6, S) == (0, "untouched")     # 5 touched frames and one padding word
        r.set_verify_checksums(False)
        assert _call(zs, r, B2, len(rg), 6, S) == (0, "untouched")
        S.synchronize()
        buf, res = B.host()
        assert res[:-1] == want and res[-1] == 2
        _check(rg, buf, data, want)
        buf, res = B2.host()                                 # verification off: all full
        assert res[:-1] == [c for _, c in ranges] and res[-1] == len(ranges)
        _check(rg, buf, data, res[:-1])


# ---------------------------------------------------------------------------
# 8. scratch bounded by max_frames, not by how far apart the frames lie
# ---------------------------------------------------------------------------
def test_indirect_scratch_independent_of_sparsity(gpu, zs, oracle):
    """Image A: 16 frames of 64 KiB.  Image B: the same 16 frames as the first
    8 and the last 8 of 512 (the 496 between them repeat frame 0, so B's
    largest frame is A's).  The same read of those 16 frames with max_frames
    16 on fresh readers: B's device memory exceeds A's by the resident table's
    growth alone."""
    import torch
    F = 65536
    a = oracle.synth(16 * F, 3)
    b = np.concatenate([a[: 8 * F]] + [a[:F]] * 496 + [a[8 * F:]])
    img_a, img_b = zs.lz4_seekable(a, F).tobytes(), zs.lz4_seekable(b, F).tobytes()
    assert len(img_b) > 20 * len(img_a)                      # the touched frames lie far apart
    S = torch.cuda.Stream(device=gpu)
    mem = []
    for img, base in ((img_a, 0), (img_b, 496 * F)):
        with _Open(zs, gpu, img) as r:
            _, d_off = r.frames()
            assert len(d_off) - 1 == (16 if base == 0 else 512)
            ranges = [(k * F + 11, F - 20) for k in range(8)] + [(base + k * F + 3, F - 9) for k in range(8, 16)]
            rg, nbytes = _layout(zs, ranges)
            B = _Bufs(gpu, rg, nbytes)
            assert _call(zs, r, B, len(rg), 16, S) == (0, "untouched")
            S.synchronize()
            buf, res = B.host()
            assert res == [c for _, c in ranges] + [16]
            _check(rg, buf, (a if base == 0 else b).tobytes(), res[:-1])
            mem.append(r.gpu_stats()["device_memory"])
    print("device memory: A", mem[0], "B", mem[1], "difference", mem[1] - mem[0])
    assert mem[1] - mem[0] <= 496 * (16 + 4) + 4096


# ---------------------------------------------------------------------------
# 9. calls in flight, mixing with synchronous reads, teardown
# ---------------------------------------------------------------------------
def test_indirect_five_calls_back_to_back(gpu, zs, payloads):
    import torch
    name = "lz4_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name)) as r:
        _, d_off = r.frames()
        sets = []
        for seed in range(20, 25):
            ranges, size = _ranges_for(d_off, seed)
            rg, nbytes = _layout(zs, ranges)
            sets.append((ranges, rg, _Bufs(gpu, rg, nbytes)))
        rets = [_call(zs, r, B, len(rg), 16, S) for _, rg, B in sets]    # more calls than slots: they are recycled
        assert rets == [(0, "untouched")] * 5
        S.synchronize()
        for ranges, rg, B in sets:
            buf, res = B.host()
            assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
            _check(rg, buf, payloads[name], res[:-1])
        assert r.gpu_stats()["batches"] == 5


def test_indirect_then_synchronous_read(gpu, zs, payloads):
    import torch
    name = "lz4_64k_direct"
    data = payloads[name]
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name)) as r:
        _, d_off = r.frames()
        ranges, size = _ranges_for(d_off, 14)
        rg, nbytes = _layout(zs, ranges)
        B = _Bufs(gpu, rg, nbytes)
        assert _call(zs, r, B, len(rg), 16, S) == (0, "untouched")
        # no synchronization: the synchronous read first waits for what it needs
        assert r.pread(200000, 12345) == data[12345:212345]
        S.synchronize()
        buf, res = B.host()
        assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
        _check(rg, buf, data, res[:-1])


def test_indirect_then_close(gpu, zs, payloads):
    import torch
    name = "lz4_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    o = _Open(zs, gpu, golden_file(name))
    r = o.r
    _, d_off = r.frames()
    ranges, size = _ranges_for(d_off, 15)
    rg, nbytes = _layout(zs, ranges)
    B = _Bufs(gpu, rg, nbytes)
    assert _call(zs, r, B, len(rg), 16, S) == (0, "untouched")
    r.close()                                                # waits for the queued work, then frees
    S.synchronize()
    buf, res = B.host()
    assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
    _check(rg, buf, payloads[name], res[:-1])


# ---------------------------------------------------------------------------
# 10. refusals: -1, the text, nothing queued
# ---------------------------------------------------------------------------
def _untouched(B):
    assert (B.buf.cpu().numpy() == SENT).all() and (B.res.cpu().numpy() == UNSET).all()


def test_indirect_refusals(gpu, zs):
    import torch
    S = torch.cuda.Stream(device=gpu)
    rg, nbytes = _layout(zs, [(10, 100), (70000, 5)])
    B = _Bufs(gpu, rg, nbytes)
    err = C.create_string_buffer(b"untouched", 80)
    assert zs.lib().zsk_preadv_device_indirect(None, B.buf.data_ptr(), nbytes, B.rg.data_ptr(), 2, 2,
                                               B.res.data_ptr(), S.cuda_stream, err) == -1
    assert err.value == b"invalid reader"
    with zs.Reader(golden_file("lz4_64k_direct"), 0) as r:   # a host image
        assert _call(zs, r, B, 2, 2, S) == (-1, "device-planned read: needs a device image")
    with _Open(zs, gpu, golden_file("zstd_64k_direct")) as r:
        assert _call(zs, r, B, 2, 2, S) == (-1, "device-planned read: zstd is not supported")
    with _Open(zs, gpu, golden_file("lz4_64k_direct")) as r:
        ret, err = _call(zs, r, B, 2, 2, S, d_rg=False)
        assert ret == -1 and err not in ("", "untouched")
        ret, err = _call(zs, r, B, 2, 2, S, d_res=False)
        assert ret == -1 and err not in ("", "untouched")
        ret, err = _call(zs, r, B, 2, 0, S)
        assert ret == -1 and err not in ("", "untouched")
        assert _call(zs, r, B, 2, 2, S, d_buf=False) == (-1, "invalid buffer")
        # max_frames x the largest frame against the batch size
        r.set_batch_bytes(4 * 65536)
        assert _call(zs, r, B, 2, 5, S) == (-1, "device-planned read: max_frames frames exceed the batch size")
        S.synchronize()
        _untouched(B)
        assert r.gpu_stats()["batches"] == 0
        assert _call(zs, r, B, 2, 4, S) == (0, "untouched")  # ... and what just fits
        S.synchronize()
        assert B.res.cpu().numpy().tolist() == [100, 5, 2]
        # no ranges: d_result[0] = 0 alone; nothing for a NULL d_result
        B = _Bufs(gpu, rg, nbytes)
        assert _call(zs, r, B, 0, 0, S) == (0, "untouched")
        assert _call(zs, r, B, 0, 0, S, d_res=False, d_rg=False) == (0, "untouched")
        S.synchronize()
        assert B.res.cpu().numpy().tolist() == [0, UNSET, UNSET]
        assert (B.buf.cpu().numpy() == SENT).all()
        # a buffer of no bytes: every range with bytes is outside it
        B = _Bufs(gpu, rg, nbytes)
        assert _call(zs, r, B, 2, 2, S, d_buf=False, buf_size=0) == (0, "untouched")
        S.synchronize()
        assert B.res.cpu().numpy().tolist() == [-1, -1, 0]
        assert (B.buf.cpu().numpy() == SENT).all()


def test_indirect_refuses_a_capturing_stream(gpu, zs):
    """The asynchronous call's rule with this call's prefix: nothing of the
    call may end up in a graph.  (The graph is never replayed.)"""
    import torch
    S = torch.cuda.Stream(device=gpu)
    rg, nbytes = _layout(zs, [(10, 100), (70000, 5)])
    B = _Bufs(gpu, rg, nbytes)
    x = torch.zeros(16, device=gpu)
    with _Open(zs, gpu, golden_file("lz4_64k_direct")) as r:
        assert _call(zs, r, B, 2, 2, S) == (0, "untouched")  # (buffers exist: the refusal is not an allocation's)
        S.synchronize()
        B = _Bufs(gpu, rg, nbytes)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=S):
            got = _call(zs, r, B, 2, 2, S)
            x.add_(1)
        assert got == (-1, "device-planned read: stream is capturing")
        del g
        torch.cuda.synchronize()
        _untouched(B)
        assert r.gpu_stats()["batches"] == 1
