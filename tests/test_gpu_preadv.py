"""Vectored reads on the GPU: zsk_gather_segments (csrc/range_gather.hip) on
its own, then zsk_preadv / zsk_preadv_device through the reader
(csrc/reader_vec.cpp's gathered batches, planned by csrc/range_plan.h).

Expected bytes are numpy slices of the source buffer or of the golden files'
payloads, never the library's own output -- except where a corrupted frame
still decodes (to other bytes): there the yardstick is what zseek_hip.h
defines the call by, a zseek_pread loop on a reader opened with a cache."""
from __future__ import annotations

import os

import numpy as np
import pytest

from conftest import golden_file, sha

pytestmark = pytest.mark.gpu

SENT = 0xA5
GOOD = ["lz4_64k_direct", "lz4_4k_direct", "lz4_1m_direct", "zstd_64k_direct"]


# ---------------------------------------------------------------------------
# 1. the gather kernel alone
# ---------------------------------------------------------------------------
def _source(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _run_gather(zs, gpu, segs, src, dst_bytes, status=None):
    """segs: (src_off, dst_off, len, frame).  -> the destination after the
    launch, and what numpy slicing says it must be."""
    import torch
    arr = np.zeros(len(segs), zs.SEGMENT_DTYPE)
    for i, (so, do, ln, fr) in enumerate(segs):
        arr[i] = (so, do, ln, fr)
    want = np.full(dst_bytes, SENT, np.uint8)
    for so, do, ln, fr in segs:
        if status is None or status[fr] == 0:
            want[do: do + ln] = src[so: so + ln]
    d_seg = torch.from_numpy(arr.view(np.uint8).copy()).to(gpu)
    d_src = torch.from_numpy(src).to(gpu)
    d_dst = torch.full((dst_bytes,), SENT, dtype=torch.uint8, device=gpu)
    d_st = None if status is None else torch.from_numpy(np.asarray(status, np.int32)).to(gpu)
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    zs.gather_segments(d_seg, d_src, d_dst, d_st)
    torch.cuda.synchronize()
    return d_dst.cpu().numpy(), want


LENS = [0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 255, 4097]


def test_gather_every_alignment_pair(gpu, zs):
    """All 256 (src % 16, dst % 16) pairs x 12 lengths in one launch, every
    destination between 32-byte guard zones: the payload is exact and no
    guard byte changes (the whole destination buffer is compared)."""
    segs, s_at, d_at = [], 0, 0
    for sa in range(16):
        for da in range(16):
            for ln in LENS:
                so = (s_at + 15) // 16 * 16 + sa
                do = (d_at + 32 + 15) // 16 * 16 + da      # >= 32 guard bytes before ...
                segs.append((so, do, ln, 0))
                s_at = so + ln
                d_at = do + ln + 32                        # ... and after
    assert {(s[0] % 16, s[1] % 16) for s in segs} == {(a, b) for a in range(16) for b in range(16)}
    src = _source(s_at + 16, 1)
    got, want = _run_gather(zs, gpu, segs, src, d_at + 32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], len(bad))


def test_gather_one_big_segment_among_thousands_of_small(gpu, zs):
    """One launch: a 3 MiB segment and 4,000 segments of 1..80 bytes, at
    random alignments, in shuffled order."""
    rng = np.random.default_rng(2)
    big = 3 << 20
    parts = [(big, int(rng.integers(0, 16)), int(rng.integers(0, 16)))]
    parts += [(int(rng.integers(1, 81)), int(rng.integers(0, 16)), int(rng.integers(0, 16))) for _ in range(4000)]
    order = rng.permutation(len(parts))
    segs, s_at, d_at = [None] * len(parts), 0, 0
    for i in order:                                        # laid out in one order, listed in another
        ln, sa, da = parts[i]
        so = (s_at + 15) // 16 * 16 + sa
        do = (d_at + 32 + 15) // 16 * 16 + da
        segs[i] = (so, do, ln, 0)
        s_at, d_at = so + ln, do + ln + 32
    src = _source(s_at + 16, 3)
    got, want = _run_gather(zs, gpu, segs, src, d_at + 32)
    assert np.array_equal(got, want)


def test_gather_skips_failed_frames(gpu, zs):
    rng = np.random.default_rng(4)
    status = [0, 16, 0, 104, 0x7FFF, 0, 0, 1]
    segs, s_at, d_at = [], 0, 0
    for i in range(300):
        ln = int(rng.integers(0, 3000))
        so, do = s_at + int(rng.integers(0, 9)), d_at + 32 + int(rng.integers(0, 9))
        segs.append((so, do, ln, int(rng.integers(0, len(status)))))
        s_at, d_at = so + ln, do + ln
    src = _source(s_at + 16, 5)
    got, want = _run_gather(zs, gpu, segs, src, d_at + 32, status)
    assert np.array_equal(got, want)
    skipped = [s for s in segs if status[s[3]] != 0 and s[2]]
    assert skipped and all((got[s[1]: s[1] + s[2]] == SENT).all() for s in skipped)


def test_gather_no_segments(gpu, zs):
    import torch
    d = torch.zeros(64, dtype=torch.uint8, device=gpu)
    assert zs.lib().zsk_gather_segments(d.data_ptr(), 0, d.data_ptr(), d.data_ptr(), None, None) == 0
    zs.gather_segments(d[:0], d, d)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 2. parity on good files
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
    return rg, at + 16


def _check(rg, buf, data, size, results=None):
    """Every result min(count, size - offset), every byte the payload's, the
    gaps (and everything else) still the sentinel; bytes of a destination
    past its result are unspecified and not looked at."""
    want = np.full(buf.size, SENT, np.uint8)
    look = np.ones(buf.size, bool)
    payload = np.frombuffer(data, np.uint8)
    for i, q in enumerate(rg):
        off, cnt, dst = int(q["offset"]), int(q["count"]), int(q["dst_off"])
        exp = min(cnt, size - off) if off < size else 0
        if results is not None:
            exp = results[i]
        assert int(q["result"]) == exp, (i, off, cnt, int(q["result"]))
        got = max(exp, 0)
        want[dst: dst + got] = payload[off: off + got]
        look[dst + got: dst + cnt] = False
    bad = np.nonzero((buf != want) & look)[0]
    assert bad.size == 0, (bad[:8], len(bad))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", GOOD)
def test_preadv_matches_payload(gpu, zs, payloads, name, device):
    import torch
    img = golden_file(name)
    with zs.Reader(img, 0) as r:
        _, d_off = r.frames()
        ranges, size = _ranges_for(d_off, 11)
        assert len(ranges) == 257 and size == len(payloads[name])
        rg, nbytes = _layout(zs, ranges)
        if device:
            d_buf = torch.full((nbytes,), SENT, dtype=torch.uint8, device=gpu)
            ret = r.preadv_raw(d_buf.data_ptr(), rg, device=True)
            torch.cuda.synchronize()
            buf = d_buf.cpu().numpy()
        else:
            buf = np.full(nbytes, SENT, np.uint8)
            ret = r.preadv_raw(buf.ctypes.data, rg)
        assert ret == len(ranges), r.error
        _check(rg, buf, payloads[name], size)


def test_preadv_python_wrappers(gpu, zs, payloads):
    import torch
    data = payloads["lz4_64k_direct"]
    with zs.Reader(golden_file("lz4_64k_direct"), 0) as r:
        got, n_ok = r.preadv([(70000, 100), (5, 0), (1 << 20, 4), (65530, 12)])
        assert got == [data[70000:70100], b"", b"", data[65530:65542]] and n_ok == 4
        d = torch.full((64,), SENT, dtype=torch.uint8, device=gpu)
        rg, n_ok = r.preadv_device(d.data_ptr(), [(131070, 4, 1), (9, 3, 33)])
        assert n_ok == 2 and rg["result"].tolist() == [4, 3]
        h = d.cpu().numpy()
        assert h[1:5].tobytes() == data[131070:131074] and h[33:36].tobytes() == data[9:12]
        assert (h[5:33] == SENT).all() and h[0] == SENT and (h[36:] == SENT).all()


# ---------------------------------------------------------------------------
# 3. corrupt frames
# ---------------------------------------------------------------------------
def _pread_loop(reader_pread, offset, count):
    """What a caller gets in total by looping pread until `count` bytes, a 0
    return or a -1: (result, bytes, failed)."""
    done, out = 0, b""
    while done < count:
        ret, chunk = reader_pread(count - done, offset + done)
        if ret < 0:
            return (done if done else -1), out, True
        if ret == 0:
            break
        done += ret
        out += chunk
    return done, out, False


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", ["frame_magic", "block_byte", "header_checksum", "zstd1m_block4_first"])
def test_preadv_corrupt_frame(gpu, zs, golden, payloads, case, device):
    """Ranges entirely before the corrupt frame, ending inside it, starting
    inside it and entirely after it (plus the frame itself): complete, the
    bytes up to the frame's start, -1 and complete, with the error string the
    goldens record for a cached read of that frame.

    Two fixtures bend that shape, as the goldens have them: `block_byte`
    corrupts a literal, so its frame still decodes (the goldens record no
    failing cached query) -- every range is complete there and the frame's
    bytes are pinned by the golden's sha for the cached read of that frame;
    the zstd fixtures corrupt frame 0, which leaves no room for the two
    ranges that start before the corrupt frame."""
    import torch
    rec = golden["corrupt"][case]
    base = rec.get("base", "lz4_64k_direct")
    data = payloads[base]
    img = bytearray(golden_file(base))
    c_off, d_off = zs.seek_table_of(np.frombuffer(bytes(img), np.uint8))
    for at, v in rec["mutations"]:
        img[at] = v
    bad = int(np.searchsorted(c_off, rec["mutations"][0][0], side="right") - 1)
    a, b = int(d_off[bad]), int(d_off[bad + 1])
    assert bad + 1 < len(d_off) - 1
    errors = [q["error"] for q in rec["results"] if q["cache"] >= 1 and q["ret"] != "hang" and q["ret"] < 0]
    fails = bool(errors)
    ranges, want = [], []
    if bad > 0:
        ranges += [(a - 5000, 3000), (a - 300, 1000)]
        want += [3000, 300 if fails else 1000]
    ranges += [(a + 10, (b - a) + 500), (b + 5, 3000), (a, b - a)]
    want += [-1 if fails else (b - a) + 500, 3000, -1 if fails else b - a]
    rg, nbytes = _layout(zs, ranges)
    with zs.Reader(bytes(img), 0) as r:
        if device:
            d_buf = torch.full((nbytes,), SENT, dtype=torch.uint8, device=gpu)
            ret = r.preadv_raw(d_buf.data_ptr(), rg, device=True)
            torch.cuda.synchronize()
            buf = d_buf.cpu().numpy()
        else:
            buf = np.full(nbytes, SENT, np.uint8)
            ret = r.preadv_raw(buf.ctypes.data, rg)
        err = r.error
    print(case, "results", rg["result"].tolist(), "ret", ret, "error", err)
    assert rg["result"].tolist() == want
    assert ret == sum(1 for (o, c), w in zip(ranges, want) if w == c)
    if fails:
        assert err == errors[0]
        _check(rg, buf, data, len(data), results=want)
    else:
        # the frame decodes to other bytes: the golden's cached read of it
        q = next(q for q in rec["results"] if q["cache"] >= 1 and (q["offset"], q["count"]) == (a, b - a))
        whole = int(rg[-1]["dst_off"])
        assert sha(buf[whole: whole + (b - a)]) == q["sha256"]
        frame = buf[whole: whole + (b - a)]
        for i, (off, cnt) in enumerate(ranges):   # every range: the payload outside the frame, the frame's bytes inside
            dst = int(rg[i]["dst_off"])
            exp = np.frombuffer(data, np.uint8)[off: off + cnt].copy()
            lo, hi = max(off, a), min(off + cnt, b)
            if hi > lo:
                exp[lo - off: hi - off] = frame[lo - a: hi - a]
            assert np.array_equal(buf[dst: dst + cnt], exp), i
    # the definition: a zseek_pread loop on a reader opened with a cache
    with zs.Reader(bytes(img), 1) as c:
        def ours(n, off):
            out = np.empty(max(n, 1), np.uint8)
            ret = c.pread_raw(out.ctypes.data, n, off)
            return ret, out[:max(ret, 0)].tobytes()
        for i, (off, cnt) in enumerate(ranges):
            res, out, _ = _pread_loop(ours, off, cnt)
            dst = int(rg[i]["dst_off"])
            assert int(rg[i]["result"]) == res, i
            assert buf[dst: dst + max(res, 0)].tobytes() == out, i
    # ... and, where it is built, on the reference itself
    from oracle.oracle import REF_SO, RefZseek
    if os.path.exists(REF_SO) and not any(q["ret"] == "hang" for q in rec["results"]):
        ref = RefZseek().open(bytes(img), 1)
        try:
            for i, (off, cnt) in enumerate(ranges):
                res, out, _ = _pread_loop(ref.pread, off, cnt)
                dst = int(rg[i]["dst_off"])
                assert int(rg[i]["result"]) == res, i
                assert buf[dst: dst + max(res, 0)].tobytes() == out, i
        finally:
            ref.close()


# ---------------------------------------------------------------------------
# 4. what makes it one grid
# ---------------------------------------------------------------------------
def test_many_ranges_in_one_frame_decode_it_once(gpu, zs, payloads):
    data = payloads["lz4_64k_direct"]
    with zs.Reader(golden_file("lz4_64k_direct"), 0) as r:
        r.preadv([(0, 1)])                                  # (lanes and buffers exist)
        g0, p0 = r.gpu_stats(), r.npreads
        ranges = [(3 * 65536 + 611 * k, 1 + 7 * k) for k in range(100)]
        got, n_ok = r.preadv(ranges)
        g1 = r.gpu_stats()
        assert n_ok == 100 and got == [data[o: o + c] for o, c in ranges]
        assert g1["frames_decoded"] - g0["frames_decoded"] == 1
        assert g1["batches"] - g0["batches"] == 1
        assert r.npreads - p0 == 1


def test_reads_only_touched_frames_run_by_run(gpu, zs, payloads):
    data = payloads["lz4_64k_direct"]
    with zs.Reader(golden_file("lz4_64k_direct"), 0) as r:
        c_off, d_off = r.frames()
        g0, p0 = r.gpu_stats(), r.npreads
        frames = [15, 7, 0, 8, 1]
        ranges = [(int(d_off[f]) + 100 + f, 2000 + f) for f in frames]
        got, n_ok = r.preadv(ranges)
        g1 = r.gpu_stats()
        assert n_ok == 5 and got == [data[o: o + c] for o, c in ranges]
        assert r.npreads - p0 == 3                          # runs {0, 1}, {7, 8}, {15}
        assert g1["bytes_uploaded"] - g0["bytes_uploaded"] == sum(int(c_off[f + 1] - c_off[f]) for f in frames)
        assert g1["frames_decoded"] - g0["frames_decoded"] == 5 and g1["batches"] - g0["batches"] == 1


# ---------------------------------------------------------------------------
# 5. other reader-level checks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_multi_batch(gpu, zs, payloads, device):
    import torch
    data = payloads["lz4_64k_direct"]
    size = len(data)
    rng = np.random.default_rng(21)
    ranges = [(0, size)] + [(int(rng.integers(0, size - 5000)), int(rng.integers(1, 5000))) for _ in range(50)]
    rg, nbytes = _layout(zs, ranges)
    with zs.Reader(golden_file("lz4_64k_direct"), 0) as r:
        r.set_batch_bytes(131072)
        g0 = r.gpu_stats()
        if device:
            d_buf = torch.full((nbytes,), SENT, dtype=torch.uint8, device=gpu)
            ret = r.preadv_raw(d_buf.data_ptr(), rg, device=True)
            torch.cuda.synchronize()
            buf = d_buf.cpu().numpy()
        else:
            buf = np.full(nbytes, SENT, np.uint8)
            ret = r.preadv_raw(buf.ctypes.data, rg)
        assert ret == len(ranges), r.error
        assert r.gpu_stats()["batches"] - g0["batches"] >= 8
        _check(rg, buf, data, size)


def test_big_host_batch_goes_by_dma(gpu, zs, payloads):
    """More bytes than the mapped-bounce bound in one batch (the device
    compaction and one DMA), with ranges that repeat and overlap."""
    data = payloads["lz4_1m_direct"]
    size = len(data)
    ranges = [(0, size), (1000001, 700000), (0, size), (5, 0), (size - 3, 3)]
    rg, nbytes = _layout(zs, ranges)
    with zs.Reader(golden_file("lz4_1m_direct"), 0) as r:
        buf = np.full(nbytes, SENT, np.uint8)
        assert r.preadv_raw(buf.ctypes.data, rg) == len(ranges), r.error
        _check(rg, buf, data, size)


def test_cache_is_left_alone(gpu, zs, payloads):
    data = payloads["lz4_64k_direct"]
    with zs.Reader(golden_file("lz4_64k_direct"), 4) as r:
        got, n_ok = r.preadv([(100, 50), (200000, 70000), (65536 * 9, 10)])
        assert n_ok == 3 and got == [data[100:150], data[200000:270000], data[65536 * 9: 65536 * 9 + 10]]
        assert r.stats()["cached_frames"] == 0
        assert r.pread(1000, 70000) == data[70000:71000]    # a miss, decoded and cached as before
        assert r.stats()["cached_frames"] == 1
        n = r.npreads
        assert r.pread(10, 70010) == data[70010:70020]      # the hit
        assert r.npreads == n
        r.preadv([(70000, 10)])                             # does not consult it either: reads the frame
        assert r.npreads == n + 1 and r.stats()["cached_frames"] == 1


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_checksums_when_asked(gpu, zs, oracle, codec):
    data = zs.synth_buffer(1 << 20)
    img = zs.lz4_seekable(data, 65536) if codec == "lz4" else zs.zstd_seekable(data, 65536)
    c_off, d_off = zs.seek_table_of(img)
    want = np.array([oracle.xxh64(data[int(d_off[i]): int(d_off[i + 1])].tobytes()) & 0xFFFFFFFF
                     for i in range(len(d_off) - 1)], np.uint32)
    d5, d6 = int(d_off[5]), int(d_off[6])
    ranges = [(d5 + 7, 100), (d6 + 1, 3000), (d5 - 50, 100), (10, 20), (d6 - 1, 2)]
    exact = [data[o: o + c].tobytes() for o, c in ranges]
    with zs.Reader(zs.with_frame_checksums(img, want), 0) as r:
        r.set_verify_checksums(True)
        assert r.preadv(ranges) == (exact, 5)
    want[5] ^= 1
    bad = zs.with_frame_checksums(img, want)
    with zs.Reader(bad, 0) as r:                            # default off
        assert r.preadv(ranges) == (exact, 5)
    with zs.Reader(bad, 0) as r:
        r.set_verify_checksums(True)
        got, n_ok = r.preadv(ranges)
        assert n_ok == 2 and r.error.endswith(": frame checksum mismatch")
        assert got == [None, exact[1], exact[2][:50], exact[3], None]
