"""zsk_preadv_device_async on the GPU: a vectored read queued on the caller's
stream, its per-range results left in device memory by range_result_kernel
(csrc/range_result.hip) behind the decode.

Expected bytes are numpy slices of the golden files' payloads; expected results
are the arithmetic zseek_hip.h states (min(count, size - offset), the bytes
before the first failed frame, -1) or come from the golden records -- never the
library's own output.  Every test runs on a non-default torch stream unless it
says otherwise, and allocates every tensor before the call under test, so
torch's allocator cannot be what synchronizes."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import golden_file

pytestmark = pytest.mark.gpu

SENT = 0xA5
UNSET = -7777          # what d_result holds before a call


# ---------------------------------------------------------------------------
# helpers (own copies of test_gpu_preadv.py's and test_gpu_device_image.py's)
# ---------------------------------------------------------------------------
def _ranges_for(d_off, seed):
    """257 (offset, count) ranges in shuffled order: the named edge cases,
    then random ones."""
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
    assert (rg["result"] == 424242).all()     # const


def _place(gpu, img: bytes, at: int = 2):
    """The image at byte offset `at` of a device tensor.  -> (tensor, pointer)."""
    import torch
    t = torch.full((at + len(img) + 64,), SENT, dtype=torch.uint8, device=gpu)
    t[at: at + len(img)].copy_(torch.from_numpy(np.frombuffer(img, np.uint8).copy()))
    torch.cuda.synchronize()
    return t, t.data_ptr() + at


class _Open:
    """A reader over a host image or over the same bytes in device memory."""

    def __init__(self, zs, gpu, img: bytes, device_image: bool):
        self.keep = None
        if device_image:
            self.keep, ptr = _place(gpu, img)
            self.r = zs.Reader.open_device(ptr, len(img), 0)
        else:
            self.r = zs.Reader(img, 0)

    def __enter__(self):
        return self.r

    def __exit__(self, *exc):
        self.r.close()


def _buffers(gpu, rg, nbytes):
    import torch
    d_buf = torch.full((nbytes,), SENT, dtype=torch.uint8, device=gpu)
    d_res = torch.full((len(rg) + 1,), UNSET, dtype=torch.int64, device=gpu)
    torch.cuda.synchronize()
    return d_buf, d_res


def _call(zs, r, d_buf, rg, d_res, stream):
    """The C entry itself: -> (return value, errbuf text)."""
    err = C.create_string_buffer(b"untouched", 80)
    ret = zs.lib().zsk_preadv_device_async(r.handle, d_buf.data_ptr() if d_buf is not None else None,
                                           rg.ctypes.data if rg.size else None, rg.size,
                                           d_res.data_ptr() if d_res is not None else None, stream.cuda_stream, None,
                                           err)
    return ret, err.value.decode()


# ---------------------------------------------------------------------------
# 1. parity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device_image", [False, True], ids=["host_image", "device_image"])
@pytest.mark.parametrize("name", ["lz4_64k_direct", "lz4_4k_direct", "lz4_1m_direct"])
def test_async_matches_payload(gpu, zs, payloads, name, device_image):
    import torch
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name), device_image) as r:
        _, d_off = r.frames()
        ranges, size = _ranges_for(d_off, 11)
        assert len(ranges) == 257 and size == len(payloads[name])
        rg, nbytes = _layout(zs, ranges)
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        ret, err = _call(zs, r, d_buf, rg, d_res, S)
        assert (ret, err) == (0, "untouched")
        S.synchronize()
        res = d_res.cpu().numpy().tolist()
        assert res[:-1] == _full(ranges, size)
        assert res[-1] == len(ranges)
        _check(rg, d_buf.cpu().numpy(), payloads[name], res[:-1])
        gs = r.gpu_stats()
        assert gs["batches"] >= 1 and gs["frames_decoded"] == len(d_off) - 1
        if device_image:
            assert gs["bytes_uploaded"] == 0


def test_async_python_wrapper(gpu, zs, payloads):
    import torch
    data = payloads["lz4_64k_direct"]
    S = torch.cuda.Stream(device=gpu)
    d = torch.full((64,), SENT, dtype=torch.uint8, device=gpu)
    res = torch.full((3,), UNSET, dtype=torch.int64, device=gpu)
    torch.cuda.synchronize()
    with zs.Reader(golden_file("lz4_64k_direct"), 0) as r:
        assert r.preadv_device_async(d.data_ptr(), [(131070, 4, 1), (9, 3, 33)], res.data_ptr(), S.cuda_stream) is None
        S.synchronize()
        h = d.cpu().numpy()
        assert res.cpu().tolist() == [4, 3, 2]
        assert h[1:5].tobytes() == data[131070:131074] and h[33:36].tobytes() == data[9:12]
        assert (h[5:33] == SENT).all() and h[0] == SENT and (h[36:] == SENT).all()
        with pytest.raises(zs.ZseekError):
            r.preadv_device_async(d.data_ptr(), [(0, 4, 0)], 0, S.cuda_stream)


# ---------------------------------------------------------------------------
# 2. stream order, without a host wait in between
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device_image", [False, True], ids=["host_image", "device_image"])
def test_async_is_ordered_on_the_stream(gpu, zs, payloads, device_image):
    """fill(sentinel), read, copy, fill(0) on one stream, one synchronize: the
    copy holds payload bytes and sentinel gaps, so the read ran after the first
    fill and before the copy."""
    import torch
    name = "lz4_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name), device_image) as r:
        _, d_off = r.frames()
        ranges, size = _ranges_for(d_off, 12)
        rg, nbytes = _layout(zs, ranges)
        d_buf = torch.zeros(nbytes, dtype=torch.uint8, device=gpu)
        d_copy = torch.zeros(nbytes, dtype=torch.uint8, device=gpu)
        d_res = torch.full((len(rg) + 1,), UNSET, dtype=torch.int64, device=gpu)
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            d_buf.fill_(SENT)
            ret, err = _call(zs, r, d_buf, rg, d_res, S)
            d_copy.copy_(d_buf)
            d_buf.zero_()
        assert (ret, err) == (0, "untouched")
        S.synchronize()
        res = d_res.cpu().numpy().tolist()
        assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
        _check(rg, d_copy.cpu().numpy(), payloads[name], res[:-1])
        assert not d_buf.cpu().numpy().any()


# ---------------------------------------------------------------------------
# 3. the call returns before its work runs
# ---------------------------------------------------------------------------
def _busy_work(gpu, S, seconds):
    """Preallocated torch.mm work for stream S sized at run time to last at
    least `seconds`: -> a callable that queues it."""
    import torch
    a = torch.randn(4096, 4096, device=gpu)
    b = torch.randn(4096, 4096, device=gpu)
    c = torch.empty(4096, 4096, device=gpu)
    with torch.cuda.stream(S):
        for _ in range(3):
            torch.mm(a, b, out=c)
        S.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(S)
        for _ in range(4):
            torch.mm(a, b, out=c)
        t1.record(S)
        S.synchronize()
    one = t0.elapsed_time(t1) / 4 / 1e3
    reps = int(seconds / one) + 1
    print(f"busy work: one mm {one * 1e3:.3f} ms, {reps} queued for {seconds} s")

    def queue():
        with torch.cuda.stream(S):
            for _ in range(reps):
                torch.mm(a, b, out=c)
    return queue


@pytest.mark.parametrize("device_image", [False, True], ids=["host_image", "device_image"])
def test_async_returns_before_its_work_runs(gpu, zs, payloads, device_image):
    """Behind >= 0.2 s of queued work (far above any latency of the
    synchronous call, 0.1 to 8 ms) the stream is still busy when the call
    returns: it did not wait for its own work.  Then three single-batch calls
    back to back (within kSlots)."""
    import torch
    name = "lz4_64k_direct"
    data = payloads[name]
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name), device_image) as r:
        _, d_off = r.frames()
        ranges, size = _ranges_for(d_off, 13)
        rg, nbytes = _layout(zs, ranges)
        bufs = [_buffers(gpu, rg, nbytes) for _ in range(5)]
        queue = _busy_work(gpu, S, 0.25)
        # one warm-up call: buffers are grown
        assert _call(zs, r, bufs[0][0], rg, bufs[0][1], S)[0] == 0
        S.synchronize()
        queue()
        ret, err = _call(zs, r, bufs[1][0], rg, bufs[1][1], S)
        busy = not S.query()
        assert (ret, err) == (0, "untouched")
        assert busy, "the call waited for the stream"
        S.synchronize()
        b0 = r.gpu_stats()["batches"]
        queue()
        rets = [_call(zs, r, bufs[k][0], rg, bufs[k][1], S)[0] for k in (2, 3, 4)]
        busy = not S.query()
        assert rets == [0, 0, 0]
        assert busy, "three calls in flight waited for the stream"
        assert r.gpu_stats()["batches"] == b0 + 3           # single-batch calls
        S.synchronize()
        for d_buf, d_res in bufs:
            res = d_res.cpu().numpy().tolist()
            assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
            _check(rg, d_buf.cpu().numpy(), data, res[:-1])


# ---------------------------------------------------------------------------
# 4. corrupt frames
# ---------------------------------------------------------------------------
def _five_ranges(a, b, fails=True):
    """test_preadv_corrupt_frame's: before the frame [a, b), ending inside it,
    starting inside it, after it, and the frame itself; -> (ranges, want)."""
    ranges = [(a - 5000, 3000), (a - 300, 1000), (a + 10, (b - a) + 500), (b + 5, 3000), (a, b - a)]
    want = [3000, 300 if fails else 1000, -1 if fails else (b - a) + 500, 3000, -1 if fails else b - a]
    return ranges, want


@pytest.mark.parametrize("device_image", [False, True], ids=["host_image", "device_image"])
@pytest.mark.parametrize("case", ["frame_magic", "header_checksum"])
def test_async_corrupt_frame(gpu, zs, golden, payloads, case, device_image):
    import torch
    rec = golden["corrupt"][case]
    assert rec.get("base", "lz4_64k_direct") == "lz4_64k_direct"
    data = payloads["lz4_64k_direct"]
    img = bytearray(golden_file("lz4_64k_direct"))
    c_off, d_off = zs.seek_table_of(np.frombuffer(bytes(img), np.uint8))
    for at, v in rec["mutations"]:
        img[at] = v
    bad = int(np.searchsorted(c_off, rec["mutations"][0][0], side="right") - 1)
    a, b = int(d_off[bad]), int(d_off[bad + 1])
    # the goldens record the frame as failing for a cached read
    assert [q for q in rec["results"] if q["cache"] >= 1 and q["ret"] != "hang" and q["ret"] < 0]
    ranges, want = _five_ranges(a, b)
    rg, nbytes = _layout(zs, ranges)
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, bytes(img), device_image) as r:
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        ret, err = _call(zs, r, d_buf, rg, d_res, S)
        S.synchronize()
        assert (ret, err) == (0, "untouched")              # no error text is deferred
        res = d_res.cpu().numpy().tolist()
        print(case, "results", res)
        assert res[:-1] == want
        assert res[-1] == sum(1 for (o, c), w in zip(ranges, want) if w == c)
        _check(rg, d_buf.cpu().numpy(), data, want)


# ---------------------------------------------------------------------------
# 5. many batches, and a failure in a later batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device_image", [False, True], ids=["host_image", "device_image"])
def test_async_many_batches(gpu, zs, golden, payloads, device_image):
    import torch
    name = "lz4_64k_direct"
    data = payloads[name]
    good = golden_file(name)
    c_off, d_off = zs.seek_table_of(np.frombuffer(good, np.uint8))
    d = [int(x) for x in d_off]
    size = d[-1]
    rng = np.random.default_rng(5)
    ranges = [(0, size)] + [(int(rng.integers(0, size)), int(rng.integers(1, 3000))) for _ in range(50)]
    ranges += [(d[3] + 17, d[8] - d[3]), (d[9] + 1, 100), (d[8] + 5, 2 * 65536), (d[12], 10)]
    rg, nbytes = _layout(zs, ranges)
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, good, device_image) as r:
        r.set_batch_bytes(131072)
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        b0 = r.gpu_stats()["batches"]
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        assert r.gpu_stats()["batches"] - b0 >= 8           # more than kSlots: slots are recycled
        S.synchronize()
        res = d_res.cpu().numpy().tolist()
        assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
        _check(rg, d_buf.cpu().numpy(), data, res[:-1])
    # frame 9 corrupt: the goldens' frame_magic mutation moved to that frame's c_off
    (at, v), = golden["corrupt"]["frame_magic"]["mutations"]
    img = bytearray(good)
    img[int(c_off[9]) + (at - int(c_off[1]))] = v
    want = []
    for o, c in ranges:                                      # the header's rules, frame 9 = [d[9], d[10]) failed
        full = min(c, size - o)
        if o + full <= d[9] or o >= d[10]:
            want.append(full)
        elif o >= d[9]:
            want.append(-1)
        else:
            want.append(d[9] - o)
    assert want[0] == d[9] and want[51] == d[8] - d[3] and want[52] == -1 and want[53] == d[9] - d[8] - 5
    with _Open(zs, gpu, bytes(img), device_image) as r:
        r.set_batch_bytes(131072)
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        S.synchronize()
        res = d_res.cpu().numpy().tolist()
        assert res[:-1] == want                              # the statuses of every batch reached the results
        assert res[-1] == sum(1 for (o, c), w in zip(ranges, want) if w == min(c, size - o))
        _check(rg, d_buf.cpu().numpy(), data, want)


# ---------------------------------------------------------------------------
# 6. seek-table checksums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device_image", [False, True], ids=["host_image", "device_image"])
def test_async_checksums(gpu, zs, oracle, payloads, device_image):
    import torch
    name = "lz4_64k_direct"
    plain, data = np.frombuffer(golden_file(name), np.uint8), payloads[name]
    _, d_off = zs.seek_table_of(plain)
    d = [int(x) for x in d_off]
    sums = np.array([oracle.xxh64(data[d[i]: d[i + 1]]) & 0xFFFFFFFF for i in range(len(d) - 1)], np.uint32)
    sums[5] ^= 1                                             # one wrong word
    bad = zs.with_frame_checksums(plain, sums).tobytes()
    ranges, want = _five_ranges(d[5], d[6])
    ranges.append((0, d[-1]))
    want.append(d[5])
    rg, nbytes = _layout(zs, ranges)
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, bad, device_image) as r:
        r.set_batch_bytes(192 << 10)                        # frame 5's word rides in a later batch
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        d_buf2, d_res2 = _buffers(gpu, rg, nbytes)
        r.set_verify_checksums(True)
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        r.set_verify_checksums(False)
        assert _call(zs, r, d_buf2, rg, d_res2, S) == (0, "untouched")
        S.synchronize()
        res = d_res.cpu().numpy().tolist()
        assert res[:-1] == want and res[-1] == 2
        _check(rg, d_buf.cpu().numpy(), data, want)
        res = d_res2.cpu().numpy().tolist()                  # verification off: all full
        assert res[:-1] == [c for _, c in ranges] and res[-1] == len(ranges)
        _check(rg, d_buf2.cpu().numpy(), data, res[:-1])


# ---------------------------------------------------------------------------
# 7. mixing with synchronous calls, teardown
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device_image", [False, True], ids=["host_image", "device_image"])
def test_async_then_synchronous_reads(gpu, zs, payloads, device_image):
    import torch
    name = "lz4_64k_direct"
    data = payloads[name]
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name), device_image) as r:
        _, d_off = r.frames()
        ranges, size = _ranges_for(d_off, 14)
        rg, nbytes = _layout(zs, ranges)
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        d_buf2, _ = _buffers(gpu, rg, nbytes)
        rg2 = rg.copy()
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        # no synchronization: each synchronous read first waits for what it needs
        assert r.pread(200000, 12345) == data[12345:212345]
        n_ok = r.preadv_raw(d_buf2.data_ptr(), rg2, device=True)
        torch.cuda.synchronize()
        assert n_ok == len(ranges) and rg2["result"].tolist() == _full(ranges, size)
        res = d_res.cpu().numpy().tolist()
        assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
        _check(rg, d_buf.cpu().numpy(), data, res[:-1])
        rg2["result"] = 424242
        _check(rg2, d_buf2.cpu().numpy(), data, res[:-1])


@pytest.mark.parametrize("device_image", [False, True], ids=["host_image", "device_image"])
def test_async_then_close(gpu, zs, payloads, device_image):
    import torch
    name = "lz4_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    o = _Open(zs, gpu, golden_file(name), device_image)
    r = o.r
    _, d_off = r.frames()
    ranges, size = _ranges_for(d_off, 15)
    rg, nbytes = _layout(zs, ranges)
    d_buf, d_res = _buffers(gpu, rg, nbytes)
    assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
    r.close()                                                # waits for the queued work, then frees
    S.synchronize()
    res = d_res.cpu().numpy().tolist()
    assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
    _check(rg, d_buf.cpu().numpy(), payloads[name], res[:-1])


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def test_async_refusals(gpu, zs):
    import torch
    S = torch.cuda.Stream(device=gpu)
    rg, nbytes = _layout(zs, [(10, 100), (70000, 5)])
    d_buf, d_res = _buffers(gpu, rg, nbytes)
    with zs.Reader(golden_file("zstd_64k_direct"), 0) as r:
        assert _call(zs, r, d_buf, rg, d_res, S) == (-1, "asynchronous read: zstd is not supported")
        S.synchronize()
        assert (d_buf.cpu().numpy() == SENT).all() and (d_res.cpu().numpy() == UNSET).all()
    with zs.Reader(golden_file("lz4_64k_direct"), 0) as r:
        ret, err = _call(zs, r, d_buf, rg, None, S)
        assert ret == -1 and err
        ret, err = _call(zs, r, None, rg, d_res, S)
        assert (ret, err) == (-1, "invalid buffer")
        S.synchronize()
        assert (d_buf.cpu().numpy() == SENT).all() and (d_res.cpu().numpy() == UNSET).all()
        assert _call(zs, r, d_buf, rg[:0], d_res, S) == (0, "untouched")
        S.synchronize()
        assert d_res.cpu().numpy().tolist() == [0, UNSET, UNSET]
        assert (d_buf.cpu().numpy() == SENT).all()
