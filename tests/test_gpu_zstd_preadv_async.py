"""zsk_preadv_device_async on a zstd reader (zsk_reader_set_zstd_async): the
tests of test_gpu_preadv_async.py for the three zstd goldens, over a host image
and over a device image, with its helpers.  Each batch is decoded without a
host plan and without a wait, by bounds from the seek table; a batch beyond
them is refused whole on the device and its ranges fail.

Expected bytes are numpy slices of the golden files' payloads; expected results
the arithmetic zseek_hip.h states, or what zsk_preadv_device reports for the
same ranges on the same file."""
from __future__ import annotations

import numpy as np
import pytest

import zstd_caps_util as zu
import zstd_craft as zc
from conftest import golden_file
from test_gpu_preadv_async import (SENT, UNSET, _Open, _buffers, _busy_work, _call, _check, _five_ranges, _full,
                                   _layout, _ranges_for)

pytestmark = pytest.mark.gpu

NAMES = ["zstd_64k_direct", "zstd_64k_buffered", "zstd_1m_direct"]
IMAGES = pytest.mark.parametrize("device_image", [False, True], ids=["host_image", "device_image"])


def _open(zs, gpu, img, device_image, seq_bytes=3):
    o = _Open(zs, gpu, img, device_image)
    assert o.r.set_zstd_async(seq_bytes) is True
    return o


def _results(d_res):
    return d_res.cpu().numpy().tolist()


@IMAGES
@pytest.mark.parametrize("name", NAMES)
def test_async_matches_payload(gpu, zs, payloads, name, device_image):
    import torch
    S = torch.cuda.Stream(device=gpu)
    with _open(zs, gpu, golden_file(name), device_image) as r:
        _, d_off = r.frames()
        ranges, size = _ranges_for(d_off, 21)
        assert size == len(payloads[name])
        rg, nbytes = _layout(zs, ranges)
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        S.synchronize()
        res = _results(d_res)
        assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
        _check(rg, d_buf.cpu().numpy(), payloads[name], res[:-1])
        gs = r.gpu_stats()
        assert gs["batches"] >= 1 and gs["frames_decoded"] == len(d_off) - 1
        if device_image:
            assert gs["bytes_uploaded"] == 0


def test_switch(gpu, zs):
    """off by default; 1 and 2 are refused and change nothing; 0 turns it off again"""
    import torch
    S = torch.cuda.Stream(device=gpu)
    rg, nbytes = _layout(zs, [(10, 100), (70000, 5)])
    d_buf, d_res = _buffers(gpu, rg, nbytes)
    refusal = (-1, "asynchronous read: zstd is not supported")
    with zs.Reader(golden_file("zstd_64k_direct"), 0) as r:
        assert _call(zs, r, d_buf, rg, d_res, S) == refusal
        assert r.set_zstd_async(1) is False and r.set_zstd_async(2) is False
        assert _call(zs, r, d_buf, rg, d_res, S) == refusal
        assert r.set_zstd_async(8) is True
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        S.synchronize()
        assert _results(d_res) == [100, 5, 2]
        assert r.set_zstd_async(1) is False          # still on
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        assert r.set_zstd_async(0) is True
        assert _call(zs, r, d_buf, rg, d_res, S) == refusal
        S.synchronize()


@IMAGES
def test_async_is_ordered_on_the_stream(gpu, zs, payloads, device_image):
    """fill(sentinel), read, copy, fill(0) on one stream, one synchronize"""
    import torch
    name = "zstd_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    with _open(zs, gpu, golden_file(name), device_image) as r:
        _, d_off = r.frames()
        ranges, size = _ranges_for(d_off, 22)
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
        res = _results(d_res)
        assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
        _check(rg, d_copy.cpu().numpy(), payloads[name], res[:-1])
        assert not d_buf.cpu().numpy().any()


@IMAGES
def test_async_returns_before_its_work_runs(gpu, zs, payloads, device_image):
    """behind >= 0.25 s of queued work the stream is still busy when the call
    returns, for one call and for three in flight (within kSlots)"""
    import torch
    name = "zstd_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    with _open(zs, gpu, golden_file(name), device_image) as r:
        _, d_off = r.frames()
        ranges, size = _ranges_for(d_off, 23)
        rg, nbytes = _layout(zs, ranges)
        bufs = [_buffers(gpu, rg, nbytes) for _ in range(5)]
        queue = _busy_work(gpu, S, 0.25)
        assert _call(zs, r, bufs[0][0], rg, bufs[0][1], S)[0] == 0      # warm-up: buffers and scratch are grown
        S.synchronize()
        queue()
        ret, err = _call(zs, r, bufs[1][0], rg, bufs[1][1], S)
        busy = not S.query()
        assert (ret, err) == (0, "untouched")
        assert busy, "the call waited for the stream"
        S.synchronize()
        queue()
        rets = [_call(zs, r, bufs[k][0], rg, bufs[k][1], S)[0] for k in (2, 3, 4)]
        busy = not S.query()
        assert rets == [0, 0, 0]
        assert busy, "three calls in flight waited for the stream"
        S.synchronize()
        for d_buf, d_res in bufs:
            res = _results(d_res)
            assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
            _check(rg, d_buf.cpu().numpy(), payloads[name], res[:-1])


@IMAGES
def test_async_corrupt_frame(gpu, zs, payloads, device_image):
    """frame 3's magic number broken: the results are zsk_preadv_device's
    for the same ranges, and the frame fails"""
    import torch
    name = "zstd_64k_direct"
    img = bytearray(golden_file(name))
    c_off, d_off = zs.seek_table_of(np.frombuffer(bytes(img), np.uint8))
    img[int(c_off[3])] ^= 0xFF
    a, b = int(d_off[3]), int(d_off[4])
    ranges, _ = _five_ranges(a, b)
    rg, nbytes = _layout(zs, ranges)
    rg2 = rg.copy()
    S = torch.cuda.Stream(device=gpu)
    with _open(zs, gpu, bytes(img), device_image) as r:
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        d_buf2, _ = _buffers(gpu, rg, nbytes)
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        S.synchronize()
        n_ok = r.preadv_raw(d_buf2.data_ptr(), rg2, device=True)
        torch.cuda.synchronize()
        want = rg2["result"].tolist()
        print("zsk_preadv_device:", n_ok, want)
        assert want[0] == 3000 and want[3] == 3000 and want[4] == -1 and want[2] == -1 and n_ok == 2
        res = _results(d_res)
        assert res[:-1] == want and res[-1] == n_ok
        _check(rg, d_buf.cpu().numpy(), payloads[name], want)


@IMAGES
def test_async_many_batches(gpu, zs, payloads, device_image):
    import torch
    name = "zstd_64k_direct"
    good = golden_file(name)
    _, d_off = zs.seek_table_of(np.frombuffer(good, np.uint8))
    d = [int(x) for x in d_off]
    size = d[-1]
    rng = np.random.default_rng(6)
    ranges = [(0, size)] + [(int(rng.integers(0, size)), int(rng.integers(1, 3000))) for _ in range(50)]
    ranges += [(d[3] + 17, d[8] - d[3]), (d[9] + 1, 100), (d[8] + 5, 2 * 65536), (d[7], 10)]
    rg, nbytes = _layout(zs, ranges)
    S = torch.cuda.Stream(device=gpu)
    with _open(zs, gpu, good, device_image) as r:
        r.set_batch_bytes(131072)
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        b0 = r.gpu_stats()["batches"]
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        assert r.gpu_stats()["batches"] - b0 > 3            # more than kSlots: slots are recycled
        S.synchronize()
        res = _results(d_res)
        assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
        _check(rg, d_buf.cpu().numpy(), payloads[name], res[:-1])


@IMAGES
def test_async_checksums(gpu, zs, oracle, payloads, device_image):
    import torch
    name = "zstd_64k_direct"
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
    with _open(zs, gpu, bad, device_image) as r:
        r.set_batch_bytes(192 << 10)                        # frame 5's word rides in a later batch
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        d_buf2, d_res2 = _buffers(gpu, rg, nbytes)
        r.set_verify_checksums(True)
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        r.set_verify_checksums(False)
        assert _call(zs, r, d_buf2, rg, d_res2, S) == (0, "untouched")
        S.synchronize()
        res = _results(d_res)
        assert res[:-1] == want and res[-1] == 2
        _check(rg, d_buf.cpu().numpy(), data, want)
        res = _results(d_res2)                               # verification off: all full
        assert res[:-1] == [c for _, c in ranges] and res[-1] == len(ranges)
        _check(rg, d_buf2.cpu().numpy(), data, res[:-1])


@IMAGES
def test_async_then_synchronous_reads(gpu, zs, payloads, device_image):
    import torch
    name = "zstd_64k_direct"
    data = payloads[name]
    S = torch.cuda.Stream(device=gpu)
    with _open(zs, gpu, golden_file(name), device_image) as r:
        _, d_off = r.frames()
        ranges, size = _ranges_for(d_off, 24)
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
        res = _results(d_res)
        assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
        _check(rg, d_buf.cpu().numpy(), data, res[:-1])
        rg2["result"] = 424242
        _check(rg2, d_buf2.cpu().numpy(), data, res[:-1])


@IMAGES
def test_async_then_close(gpu, zs, payloads, device_image):
    import torch
    name = "zstd_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    o = _open(zs, gpu, golden_file(name), device_image)
    r = o.r
    _, d_off = r.frames()
    ranges, size = _ranges_for(d_off, 25)
    rg, nbytes = _layout(zs, ranges)
    d_buf, d_res = _buffers(gpu, rg, nbytes)
    assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
    r.close()                                                # waits for the queued work, then frees
    S.synchronize()
    res = _results(d_res)
    assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
    _check(rg, d_buf.cpu().numpy(), payloads[name], res[:-1])


@IMAGES
def test_too_tight_bound(gpu, zs, device_image):
    """entries of many short sequences (about four decoded bytes each) read
    with a sequence per 64 bytes: the batch does not fit, every range fails;
    the same ranges succeed through zsk_preadv_device, and asynchronously at 3"""
    import torch
    c = zc.CASE["s_rep0_minus1_is_0_at128"]
    assert c[3] is not None and c[4] == 0
    n, ds = 9, c[2]
    caps = zu.load()
    assert zu.plan(caps, c[1])[3] * 64 > 8 * ds
    # (the reader's bounds for the whole file as one batch)
    assert not zu.fits(caps, [c[1]] * n, n * ds, n * (2 + ds // 16384), n * ds // 64)
    assert zu.fits(caps, [c[1]] * n, n * ds, n * (2 + ds // 16384), n * ds // 3)
    img = zc.seekable([c[1]] * n, [ds] * n)
    data = c[3] * n
    ranges = [(i * ds, ds) for i in range(n)] + [(5, 2 * ds)]
    rg, nbytes = _layout(zs, ranges)
    rg2 = rg.copy()
    S = torch.cuda.Stream(device=gpu)
    with _open(zs, gpu, img, device_image, seq_bytes=64) as r:
        d_buf, d_res = _buffers(gpu, rg, nbytes)
        d_buf2, d_res2 = _buffers(gpu, rg, nbytes)
        d_buf3, _ = _buffers(gpu, rg, nbytes)
        assert _call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        S.synchronize()
        assert _results(d_res) == [-1] * len(ranges) + [0]
        n_ok = r.preadv_raw(d_buf3.data_ptr(), rg2, device=True)      # the remedy
        torch.cuda.synchronize()
        assert n_ok == len(ranges) and rg2["result"].tolist() == [cnt for _, cnt in ranges]
        rg2["result"] = 424242
        _check(rg2, d_buf3.cpu().numpy(), data, [cnt for _, cnt in ranges])
        assert r.set_zstd_async(3) is True
        assert _call(zs, r, d_buf2, rg, d_res2, S) == (0, "untouched")
        S.synchronize()
        res = _results(d_res2)
        assert res[:-1] == [cnt for _, cnt in ranges] and res[-1] == len(ranges)
        _check(rg, d_buf2.cpu().numpy(), data, res[:-1])
