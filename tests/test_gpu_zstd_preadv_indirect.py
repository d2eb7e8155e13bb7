"""zsk_preadv_device_indirect on a zstd reader, bounded by zsk_reader_zstd_census:
the census against the CPU walk of the same file, the switch, parity with the
payload and with zsk_preadv_device, padding descriptors over the decoder's
routes and chunks, a file of many tiny blocks that the host-planned
asynchronous read refuses, failed frames, an image rewritten behind the census
(refused whole on the device), and stream order.

Expected bytes are numpy slices of the golden files' payloads or the hand-built
entries' contents (tests/zstd_craft.py); expected results the arithmetic
zseek_hip.h states or what zsk_preadv_device reports for the same ranges on the
same reader; the expected census the CPU walk's maxima (tests/zstd_census_util.py).
Helpers are test_gpu_preadv_indirect.py's and test_gpu_preadv_async.py's."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import test_gpu_preadv_async as host_planned
import zstd_census_util as cu
import zstd_craft as zc
from conftest import golden_file
from test_gpu_preadv_async import _five_ranges
from test_gpu_preadv_indirect import (OVERFLOW, SENT, UNSET, _Bufs, _call, _check, _full, _layout, _list_unchanged,
                                      _Open, _ranges_for)

pytestmark = pytest.mark.gpu

GOLDENS = ["zstd_64k_direct", "zstd_64k_buffered", "zstd_1m_direct"]
REFUSAL = (-1, "device-planned read: zstd is not supported")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return cu.load(tmp_path_factory.mktemp("zstd_census_gpu"))


@pytest.fixture(scope="module")
def nofit():
    return cu.nofit_file()


def _read(zs, r, ranges, max_frames, S, gpu):
    """one device-planned read -> (rg, destination bytes, results)"""
    rg, nbytes = _layout(zs, ranges)
    B = _Bufs(gpu, rg, nbytes)
    assert _call(zs, r, B, len(rg), max_frames, S) == (0, "untouched")
    S.synchronize()
    buf, res = B.host()
    _list_unchanged(B, rg)
    return rg, buf, res


# ---------------------------------------------------------------------------
# 1. the census against the CPU walk
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS + ["nofit"])
def test_census_equals_the_cpu_walk(gpu, zs, shim, nofit, name):
    img = nofit[0] if name == "nofit" else golden_file(name)
    want = cu.census(shim, img)
    assert want["max_sequences"] >= 1 and want["max_items"] > 8
    with _Open(zs, gpu, img) as r:
        m0 = r.gpu_stats()["device_memory"]
        got = r.zstd_census()
        print(name, got)
        assert got == want
        b1 = r.gpu_stats()
        assert r.zstd_census() == want                       # stored: the same numbers, no GPU work
        b2 = r.gpu_stats()
        assert b2 == b1 and b1["batches"] == 0
        assert b1["device_memory"] >= m0                     # (nothing is kept for the census itself)


def test_census_refusals(gpu, zs):
    err = C.create_string_buffer(b"untouched", 80)
    c = zs.ZstdCensusC()
    L = zs.lib()
    assert L.zsk_reader_zstd_census(None, C.byref(c), err) == -1 and err.value == b"invalid reader"
    with _Open(zs, gpu, golden_file("zstd_64k_direct")) as r:
        assert L.zsk_reader_zstd_census(r.handle, None, err) == -1 and err.value == b"invalid census pointer"
    with _Open(zs, gpu, golden_file("lz4_64k_direct")) as r:
        assert L.zsk_reader_zstd_census(r.handle, C.byref(c), err) == -1
        assert err.value == b"zstd census: not a zstd reader"
        with pytest.raises(zs.ZseekError, match="not a zstd reader"):
            r.zstd_census()
    with zs.Reader(golden_file("zstd_64k_direct"), 0) as r:          # a host image
        assert L.zsk_reader_zstd_census(r.handle, C.byref(c), err) == -1
        assert err.value == b"zstd census: needs a device image"
    # a table that puts frames past the image: the device-planned read's check
    # (frame 3's cSize entry inflated by the file's size: 8-byte entries before the 9-byte footer)
    img = bytearray(golden_file("zstd_64k_direct"))
    n = int.from_bytes(img[-9:-5], "little")
    at = len(img) - 9 - 8 * (n - 3)
    assert img[-5] == 0
    img[at: at + 4] = (int.from_bytes(img[at: at + 4], "little") + len(img)).to_bytes(4, "little")
    with _Open(zs, gpu, bytes(img)) as r:
        assert L.zsk_reader_zstd_census(r.handle, C.byref(c), err) == -1 and err.value == b"unexpected EOF"


# ---------------------------------------------------------------------------
# 2. the switch
# ---------------------------------------------------------------------------
def test_census_is_the_switch(gpu, zs, payloads):
    import torch
    name = "zstd_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    ranges = [(10, 100), (70000, 5)]
    rg, nbytes = _layout(zs, ranges)
    with _Open(zs, gpu, golden_file(name)) as r:
        B = _Bufs(gpu, rg, nbytes)
        assert _call(zs, r, B, 2, 2, S) == REFUSAL
        assert r.set_zstd_async(3) is True                   # plays no part
        assert _call(zs, r, B, 2, 2, S) == REFUSAL
        assert r.set_zstd_async(0) is True
        r.zstd_census()
        for seq_bytes in (0, 3, 64, 0):
            assert r.set_zstd_async(seq_bytes) is True
            B = _Bufs(gpu, rg, nbytes)
            assert _call(zs, r, B, 2, 2, S) == (0, "untouched")
            S.synchronize()
            buf, res = B.host()
            assert res == [100, 5, 2]
            _check(rg, buf, payloads[name], res[:-1])


# ---------------------------------------------------------------------------
# 3. parity with the payload and with zsk_preadv_device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_indirect_matches_payload_and_preadv_device(gpu, zs, payloads, name):
    import torch
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name)) as r:
        r.zstd_census()
        _, d_off = r.frames()
        nframes = len(d_off) - 1
        # unsorted, overlapping in the source, repeated, zero-length, at and past
        # EOF; and offset + count wrapping past 2^64
        ranges, size = _ranges_for(d_off, 31)
        ranges = ranges[:120] + [((1 << 64) - 10, 20), ((1 << 64) - 1, 1)] + ranges[120:]
        assert size == len(payloads[name])
        rg, nbytes = _layout(zs, ranges)
        B = _Bufs(gpu, rg, nbytes)
        b0 = r.gpu_stats()
        assert _call(zs, r, B, len(rg), nframes, S) == (0, "untouched")
        gs = r.gpu_stats()
        assert gs["batches"] == b0["batches"] + 1
        assert all(gs[k] == b0[k] for k in ("frames_decoded", "bytes_decoded", "bytes_uploaded"))
        S.synchronize()
        buf, res = B.host()
        assert res[:-1] == _full(ranges, size) and res[-1] == len(ranges)
        _check(rg, buf, payloads[name], res[:-1])             # the gaps still hold the sentinel
        _list_unchanged(B, rg)
        rg2 = rg.copy()
        d_buf2 = torch.full((nbytes,), SENT, dtype=torch.uint8, device=gpu)
        n_ok = r.preadv_raw(d_buf2.data_ptr(), rg2, device=True)
        torch.cuda.synchronize()
        assert rg2["result"].tolist() == res[:-1] and n_ok == res[-1]
        rg2["result"] = 424242
        _check(rg2, d_buf2.cpu().numpy(), payloads[name], res[:-1])


# ---------------------------------------------------------------------------
# 4. padding descriptors over the routes and the chunks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_frames", [1, 64, 65])
def test_one_touched_frame_and_padding(gpu, zs, payloads, max_frames):
    """<= 64 descriptors: the fused one-frame route; 65: the wave kernels"""
    import torch
    name = "zstd_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name)) as r:
        r.zstd_census()
        _, d_off = r.frames()
        d = [int(x) for x in d_off]
        a, b = d[6], d[7]
        ranges = [(a, b - a), (a + 5, 100), (a + 1, 1), (b - 1, 1), (a + 200, 0)]
        rg, buf, res = _read(zs, r, ranges, max_frames, S, gpu)
        assert res == [b - a, 100, 1, 1, 0, 5]
        _check(rg, buf, payloads[name], res[:-1])


@pytest.fixture(scope="module")
def tiny_file():
    """4,300 entries of 8 and 4 decoded bytes"""
    a, b = zc.CASE["h_seed_A"], zc.CASE["h_seed_B1"]
    cases = [a if (i * 7) % 3 else b for i in range(4300)]
    return zc.seekable([c[1] for c in cases], [c[2] for c in cases]), b"".join(c[3] for c in cases)


@pytest.mark.parametrize("touched", [2100, 40])
def test_two_chunks_the_second_padding(gpu, zs, tiny_file, touched):
    """max_frames = 4096 decodes in two chunks of 2048 descriptors: 2,100
    touched frames leave the second mostly padding, 40 wholly"""
    import torch
    img, data = tiny_file
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, img) as r:
        assert r.zstd_census()["frames"] == 4300
        _, d_off = r.frames()
        d = [int(x) for x in d_off]
        f0 = 1000
        cuts = [d[f0], d[f0 + 3] + 1, d[f0 + touched // 2] + 2, d[f0 + touched]]
        ranges = [(cuts[i], cuts[i + 1] - cuts[i]) for i in (2, 0, 1)] + [(d[f0 + 5], 3), (d[f0] + 1, 0)]
        rg, buf, res = _read(zs, r, ranges, 4096, S, gpu)
        assert res == [c for _, c in ranges] + [len(ranges)]
        _check(rg, buf, data, res[:-1])
        rg, buf, res = _read(zs, r, ranges, touched - 1, S, gpu)     # (and one frame too many for the bound)
        assert res == [-1] * len(ranges) + [OVERFLOW] and (buf == SENT).all()


def test_every_frame_touched(gpu, zs, shim):
    """48 random valid entries (several frames each, skippable frames, content
    checksums), max_frames the frame count"""
    import torch
    img, data = cu.random_file()
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, img) as r:
        assert r.zstd_census() == cu.census(shim, img)
        _, d_off = r.frames()
        d = [int(x) for x in d_off]
        n, size = len(d) - 1, d[-1]
        assert n == 48 and size == len(data)
        # pieces that tile the file, cut inside frames, in reverse order
        cuts = sorted({0, size} | {min(d[k] + 3 * k, d[k + 1]) for k in range(1, n, 2)})
        ranges = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)][::-1]
        rg, buf, res = _read(zs, r, ranges, n, S, gpu)
        assert res == [c for _, c in ranges] + [len(ranges)]
        _check(rg, buf, data, res[:-1])


# ---------------------------------------------------------------------------
# 5. many tiny blocks: refused by the policy, read by the census
# ---------------------------------------------------------------------------
def test_many_tiny_blocks(gpu, zs, nofit):
    import torch
    img, data = nofit
    S = torch.cuda.Stream(device=gpu)
    entries, dsizes = cu.seek_table(img)
    n = len(entries)
    d = np.concatenate([[0], np.cumsum(dsizes)]).tolist()
    ranges = [(d[i], dsizes[i]) for i in range(n)][::-1] + [(3, d[3]), (d[5] + 1, 7)]
    rg, nbytes = _layout(zs, ranges)
    with host_planned._Open(zs, gpu, img, True) as r:
        assert r.set_zstd_async(3) is True
        d_buf, d_res = host_planned._buffers(gpu, rg, nbytes)
        assert host_planned._call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        S.synchronize()
        assert d_res.cpu().numpy().tolist() == [-1] * len(ranges) + [0]
        assert (d_buf.cpu().numpy() == SENT).all()
        cen = r.zstd_census()
        assert cen["max_blocks"] == 1001
        B = _Bufs(gpu, rg, nbytes)
        assert _call(zs, r, B, len(rg), n, S) == (0, "untouched")
        S.synchronize()
        buf, res = B.host()
        assert res == [c for _, c in ranges] + [len(ranges)]
        _check(rg, buf, data, res[:-1])
        # (the host-planned call does not depend on the census: still refused)
        d_buf, d_res = host_planned._buffers(gpu, rg, nbytes)
        assert host_planned._call(zs, r, d_buf, rg, d_res, S) == (0, "untouched")
        S.synchronize()
        assert d_res.cpu().numpy().tolist() == [-1] * len(ranges) + [0]


# ---------------------------------------------------------------------------
# 6. failures
# ---------------------------------------------------------------------------
def test_corrupt_frame(gpu, zs, payloads):
    """frame 3's magic number broken (test_async_corrupt_frame's corruption)"""
    import torch
    name = "zstd_64k_direct"
    img = bytearray(golden_file(name))
    c_off, d_off = zs.seek_table_of(np.frombuffer(bytes(img), np.uint8))
    img[int(c_off[3])] ^= 0xFF
    ranges, want = _five_ranges(int(d_off[3]), int(d_off[4]))
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, bytes(img)) as r:
        r.zstd_census()
        rg, buf, res = _read(zs, r, ranges, 6, S, gpu)
        assert res == want + [2]
        _check(rg, buf, payloads[name], want)
        rg2 = rg.copy()
        d_buf2 = torch.full((buf.size,), SENT, dtype=torch.uint8, device=gpu)
        n_ok = r.preadv_raw(d_buf2.data_ptr(), rg2, device=True)
        torch.cuda.synchronize()
        assert rg2["result"].tolist() == want and n_ok == 2


def test_seek_table_checksums(gpu, zs, oracle, payloads):
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
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, bad) as r:
        r.zstd_census()
        r.set_verify_checksums(True)
        rg, buf, res = _read(zs, r, ranges, len(d) - 1, S, gpu)
        assert res == want + [2]
        _check(rg, buf, data, want)
        r.set_verify_checksums(False)                        # verification off: all full
        rg, buf, res = _read(zs, r, ranges, len(d) - 1, S, gpu)
        assert res == [c for _, c in ranges] + [len(ranges)]
        _check(rg, buf, data, res[:-1])


def test_overflow(gpu, zs, payloads):
    import torch
    name = "zstd_64k_direct"
    S = torch.cuda.Stream(device=gpu)
    with _Open(zs, gpu, golden_file(name)) as r:
        r.zstd_census()
        _, d_off = r.frames()
        d = [int(x) for x in d_off]
        # frames 1, 2 (one range over the boundary), 5, 8, 8 again, 9: T = 5
        ranges = [(d[2] - 10, 20), (d[5] + 1, 100), (d[8], 50), (d[8] + 60, 5), (d[10] - 7, 100), (3, 0)]
        rg, buf, res = _read(zs, r, ranges, 4, S, gpu)
        assert res == [-1] * len(ranges) + [OVERFLOW]
        assert (buf == SENT).all()                           # nothing was moved
        rg, buf, res = _read(zs, r, ranges, 5, S, gpu)
        assert res == [20, 100, 50, 5, 7, 0, len(ranges)]
        _check(rg, buf, payloads[name], res[:-1])


# ---------------------------------------------------------------------------
# 7. the guard: an image rewritten behind the census
# ---------------------------------------------------------------------------
def test_image_rewritten_after_the_census_is_refused_on_the_device(gpu, zs, shim):
    """Two files with one seek table and one payload: every entry of the first
    is one raw block (padded by a skippable frame), the middle entry of the
    second 1,000 empty raw blocks and then that block.  The census is the
    first's; with the second's bytes under it a batch of all three entries has
    1,003 block headers against a bound of 3: zstd_fit_kernel refuses it
    whole.  A designed refusal, not a fault."""
    import torch
    many = zc.CASE["b_1000_empty_raw"]
    content, ds = many[3], many[2]
    one = zc.frame([zc.Raw(content)])
    one += zc.skippable(bytes(len(many[1]) - len(one) - 8))
    assert len(one) == len(many[1]) and cu.plan(shim, one)[1] == 1 and cu.plan(shim, many[1])[1] == 1001
    first = zc.seekable([one, one, one], [ds] * 3)
    second = zc.seekable([one, many[1], one], [ds] * 3)
    assert len(first) == len(second) and first[-40:] == second[-40:]
    data = content * 3
    ranges = [(ds, ds), (0, ds), (2 * ds + 1, 9), (5, 2 * ds)]
    S = torch.cuda.Stream(device=gpu)
    o = _Open(zs, gpu, first)
    with o as r:
        cen = r.zstd_census()
        assert (cen["max_blocks"], cen["max_sequences"]) == (1, 0)
        rg, buf, res = _read(zs, r, ranges, 3, S, gpu)
        assert res == [c for _, c in ranges] + [len(ranges)]
        _check(rg, buf, data, res[:-1])
        o.keep[2: 2 + len(second)].copy_(torch.from_numpy(np.frombuffer(second, np.uint8).copy()))
        torch.cuda.synchronize()
        rg, buf, res = _read(zs, r, ranges, 3, S, gpu)
        assert res == [-1] * len(ranges) + [0]
        assert (buf == SENT).all()
        o.keep[2: 2 + len(first)].copy_(torch.from_numpy(np.frombuffer(first, np.uint8).copy()))
        torch.cuda.synchronize()
        rg, buf, res = _read(zs, r, ranges, 3, S, gpu)
        assert res == [c for _, c in ranges] + [len(ranges)]
        _check(rg, buf, data, res[:-1])


# ---------------------------------------------------------------------------
# 8. stream order
# ---------------------------------------------------------------------------
def test_ranges_made_on_the_stream(gpu, zs, payloads):
    """On one stream: the list computed by torch ops, fill(sentinel), the read,
    copies of the bytes and the results, then everything overwritten; one
    synchronize."""
    import torch
    name = "zstd_64k_direct"
    data = payloads[name]
    size = len(data)
    n = 200
    S = torch.cuda.Stream(device=gpu)
    want = [(((k * 7919 + 13) * 37) % (size - 700), 100 + 3 * k, 5 + 701 * k) for k in range(n)]
    nbytes = 5 + 701 * n
    with _Open(zs, gpu, golden_file(name)) as r:
        r.zstd_census()
        nframes = r.stats()["frames"]
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
            ret = zs.lib().zsk_preadv_device_indirect(r.handle, d_buf.data_ptr(), nbytes, d_rg.data_ptr(), n, nframes,
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
