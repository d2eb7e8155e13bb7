"""A reader over a seekable file that lives in device memory
(zsk_reader_open_device; csrc/reader.cpp's device-image branches and
csrc/image_build.hip's image_desc_kernel).

The yardsticks are the goldens -- the compiled reference's recorded answers --
and the golden files' payloads.  Next to them every result is compared with
what a reader opened on a host copy of the same bytes gives in the same test
(the contract of the call), and that path is pinned by test_gpu_parity.py,
test_gpu_zstd.py and test_gpu_preadv.py."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_file, sha

pytestmark = pytest.mark.gpu

SENT = 0xA5
with open(os.path.join(GOLDEN, "golden.json")) as _f:
    _G = json.load(_f)
FILES = sorted(_G["files"])
CORRUPT = sorted(_G["corrupt"])


def _place(gpu, img: bytes, at: int = 0, tail: int = 64):
    """The image at byte offset `at` of a device tensor, 0xA5 guard bytes on
    both sides (tail 0: the image ends with the tensor).  -> (tensor, pointer)."""
    import torch
    t = torch.full((max(at + len(img) + tail, 1),), SENT, dtype=torch.uint8, device=gpu)
    if img:
        t[at: at + len(img)].copy_(torch.from_numpy(np.frombuffer(img, np.uint8).copy()))
    torch.cuda.synchronize()
    return t, t.data_ptr() + at


def _guards_ok(t, at: int, n: int) -> bool:
    h = t.cpu().numpy()
    return bool((h[:at] == SENT).all() and (h[at + n:] == SENT).all())


def _mutated(rec) -> bytes:
    base = golden_file(rec.get("base", "lz4_64k_direct"))
    if "truncate" in rec:
        return base[: rec["truncate"]]
    b = bytearray(base)
    for at, v in rec["mutations"]:
        b[at] = v
    return bytes(b)


def _pread(r, q):
    out = np.full(max(q["count"], 1), SENT, np.uint8)
    ret = r.pread_raw(out.ctypes.data, q["count"], q["offset"])
    return ret, out, (r.error if ret < 0 else None)


# ---------------------------------------------------------------------------
# goldens
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", FILES)
def test_golden_files(gpu, zs, golden, payloads, name):
    """Every recorded read of every golden file.  The reference reads one
    frame per call, the library every frame of the range: the answer is the
    full range and starts with exactly the reference's bytes (as
    test_gpu_parity.py / test_gpu_zstd.py hold the host-image reader to)."""
    entry = golden["files"][name]
    img = golden_file(name)
    t, ptr = _place(gpu, img, 0)
    if "open_error" in entry:
        with pytest.raises(zs.ZseekError) as e:
            zs.Reader.open_device(ptr, len(img), 1)
        assert str(e.value) == entry["open_error"]
        return
    data = payloads[name]
    dev = {c: zs.Reader.open_device(ptr, len(img), c) for c in (0, 1)}
    host = {c: zs.Reader(img, c) for c in (0, 1)}
    try:
        for q in entry["reads"]:
            ret, out, _ = _pread(dev[q["cache"]], q)
            off, cnt = q["offset"], q["count"]
            assert q["ret"] >= 0
            assert ret == max(0, min(cnt, len(data) - off)), (q, ret)
            assert ret >= q["ret"]
            assert sha(out[: q["ret"]]) == q["sha256"], q
            assert bytes(out[:ret]) == data[off: off + ret], q
            hret, hout, _ = _pread(host[q["cache"]], q)
            assert (ret, bytes(out)) == (hret, bytes(hout)), q
        for c in (0, 1):
            st = dev[c].stats()
            assert st["frames"] == entry[f"stats_cache{c}"]["frames"]
            assert st["decompressed_size"] == entry[f"stats_cache{c}"]["decompressed_size"]
            assert st["cached_frames"] == host[c].stats()["cached_frames"]
            assert dev[c].gpu_stats()["bytes_uploaded"] == 0
        assert dev[1].stats()["cached_frames"] == entry["stats_cache1"]["cached_frames"]
    finally:
        for r in list(dev.values()) + list(host.values()):
            r.close()
    assert _guards_ok(t, 0, len(img))


@pytest.mark.parametrize("case", CORRUPT)
def test_golden_corrupt(gpu, zs, golden, case):
    """Every corruption case, mutations applied to its base file: open failures
    give the recorded text; every recorded read gives the recorded return and
    error (a read the reference never returns from: -1), a successful one the
    recorded bytes first -- and all of it what the host-image reader gives."""
    rec = golden["corrupt"][case]
    img = _mutated(rec)
    t, ptr = _place(gpu, img, 0)
    if "open_error" in rec:
        with pytest.raises(zs.ZseekError) as e:
            zs.Reader.open_device(ptr, len(img), 1)
        assert str(e.value) == rec["open_error"]
        return
    zstd = rec.get("base", "").startswith("zstd")
    for q in rec["results"]:
        with zs.Reader.open_device(ptr, len(img), q["cache"]) as r, zs.Reader(img, q["cache"]) as h:
            ret, out, err = _pread(r, q)
            if q["ret"] == "hang":
                assert ret == -1, q
            elif q["ret"] < 0:
                assert ret == -1, q
                assert err == q["error"], q
            else:
                assert ret == q["ret"] if zstd else ret >= q["ret"], (q, ret, err)
                assert sha(out[: q["ret"]]) == q["sha256"], q
            hret, hout, herr = _pread(h, q)
            assert (ret, err) == (hret, herr), q
            assert bytes(out[: max(ret, 0)]) == bytes(hout[: max(ret, 0)]), q
            assert r.gpu_stats()["bytes_uploaded"] == 0
    assert _guards_ok(t, 0, len(img))


# ---------------------------------------------------------------------------
# placement: the rebased c_off and the aligned-down base
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lz4_4k_direct", "zstd_64k_direct"])
@pytest.mark.parametrize("at,tail", [(0, 64), (1, 64), (2, 64), (3, 64), (5, 64), (17, 64), (255, 64), (5, 0),
                                     (0, 0)])
def test_placement(gpu, zs, golden, payloads, name, at, tail):
    """The image at odd byte offsets of a larger tensor, and ending exactly
    with the tensor: every golden read exact, the guard bytes unchanged.  This
    covers placement (the rebased c_off, the aligned-down base) and stray
    writes; a read past the image would go unseen (the tensor ends inside its
    allocator block) -- test_table_past_end_of_image holds the bounds."""
    img, data = golden_file(name), payloads[name]
    t, ptr = _place(gpu, img, at, tail)
    assert t.data_ptr() % 256 == 0 and ptr % 256 == at
    readers = {c: zs.Reader.open_device(ptr, len(img), c) for c in (0, 1)}
    try:
        for q in golden["files"][name]["reads"]:
            ret, out, _ = _pread(readers[q["cache"]], q)
            off, cnt = q["offset"], q["count"]
            assert ret == max(0, min(cnt, len(data) - off)), (q, ret)
            assert bytes(out[:ret]) == data[off: off + ret], q
            assert sha(out[: q["ret"]]) == q["sha256"], q
        for r in readers.values():
            assert r.pread(len(data) + 9, 0) == data
    finally:
        for r in readers.values():
            r.close()
    assert _guards_ok(t, at, len(img))
    assert bytes(t[at: at + len(img)].cpu().numpy()) == img


# ---------------------------------------------------------------------------
# batch edges of image_desc_kernel; no host I/O
# ---------------------------------------------------------------------------
def _edge_reads(d_off):
    """(offset, count): the whole file, then reads that start and end mid-frame
    in the first, a middle and the last frame."""
    d = [int(x) for x in d_off]
    n, size = len(d) - 1, d[-1]
    m = n // 2
    rd = [(0, size), (0, size + 100)]
    for f in (0, m, n - 1):
        a, b = d[f], d[f + 1]
        rd += [(a + 7, max(1, (b - a) // 2)), (a + (b - a) // 3, (b - a) // 3 + 1)]
    # start mid-frame in one, end mid-frame in another
    rd += [(d[0] + 100, d[m] + 1000 - (d[0] + 100)), (d[m] + 1234, d[n - 1] + 50 - (d[m] + 1234)),
           (d[1] + 1, size - d[1] - 2), (d[n - 1] + 1, size)]
    return rd


def test_batch_edges_and_no_host_io(gpu, zs, payloads):
    """8 KiB batches over the 4 KiB-frame file: the whole file in one
    zsk_pread_device call and mid-frame reads, byte-exact, over more than one
    batch -- and not one compressed byte uploaded, where the host-image reader
    given the same reads uploads them all."""
    import torch
    name = "lz4_4k_direct"
    img, data = golden_file(name), payloads[name]
    t, ptr = _place(gpu, img, 3)
    with zs.Reader.open_device(ptr, len(img), 0) as r, zs.Reader(img, 0) as h:
        c_off, d_off = r.frames()
        stats = []
        for rd in (r, h):
            rd.set_batch_bytes(8192)
            for off, cnt in _edge_reads(d_off):
                out = torch.full((cnt + 64,), SENT, dtype=torch.uint8, device=gpu)
                ret = rd.pread_device(out.data_ptr() + 32, cnt, off)
                got = out.cpu().numpy()
                assert ret == min(cnt, len(data) - off), (off, cnt)
                assert bytes(got[32: 32 + ret]) == data[off: off + ret], (off, cnt)
                assert (got[:32] == SENT).all() and (got[32 + ret:] == SENT).all(), (off, cnt)
                assert rd.pread(cnt, off) == data[off: off + cnt]
            stats.append(rd.gpu_stats())
        dev, host = stats
        assert dev["batches"] > 1 and dev["batches"] == host["batches"]
        assert dev["frames_decoded"] == host["frames_decoded"]
        assert dev["bytes_uploaded"] == 0
        assert host["bytes_uploaded"] > 0
        # the resident table: two prefix sums of n + 1 entries
        assert dev["device_memory"] >= 16 * len(c_off)
        assert dev["device"] == gpu.index
    assert _guards_ok(t, 3, len(img))


# ---------------------------------------------------------------------------
# vectored reads
# ---------------------------------------------------------------------------
def _vec_ranges(d_off, seed):
    """Unsorted ranges that share frames, overlap in the source, repeat, are
    empty, at EOF and past it; destinations 32 guard bytes apart."""
    rng = np.random.default_rng(seed)
    d = [int(x) for x in d_off]
    n, size = len(d) - 1, d[-1]
    f = min(1, n - 1)
    fs = d[f + 1] - d[f]
    rg = [(d[f] + k * (fs // 7), 1 + fs // 11) for k in range(5)]          # share a frame
    rg += [(d[f] + 10, fs), (d[f] + 10, fs), (d[f] + 5, fs + 40)]            # repeated, overlapping
    rg += [(0, 0), (size // 2, 0), (size, 10), (size + 1000, 10), (size - 7, 100), (size - 1, 1)]
    rg += [(0, min(size, 3 * fs + 17)), (d[n - 1] - min(9, d[n - 1]), 20)]
    for _ in range(40):
        off = int(rng.integers(0, size))
        rg.append((off, int(rng.integers(1, min(size - off, 2 * fs) + 1))))
    order = rng.permutation(len(rg))
    out, at = np.zeros(len(rg), dtype=[("offset", "<u8"), ("count", "<u8"), ("dst_off", "<u8"), ("result", "<i8")]), 32
    for i in order:
        out[i] = (rg[i][0], rg[i][1], at, -7)
        at += rg[i][1] + 32
    return out, at


def _preadv_both(zs, gpu, r, rg, nbytes):
    """zsk_preadv and zsk_preadv_device with the same ranges -> per call
    (return value, results, destination buffer, errbuf)."""
    import torch
    res = []
    a = rg.copy()
    hbuf = np.full(nbytes, SENT, np.uint8)
    ret = r.preadv_raw(hbuf.ctypes.data, a)
    res.append((ret, a["result"].copy(), hbuf, r.error))
    b = rg.copy()
    dbuf = torch.full((nbytes,), SENT, dtype=torch.uint8, device=gpu)
    ret = r.preadv_raw(dbuf.data_ptr(), b, device=True)
    res.append((ret, b["result"].copy(), dbuf.cpu().numpy(), r.error))
    return res


def _check_vec(rg, nbytes, got, want, data=None):
    gret, gres, gbuf, gerr = got
    wret, wres, wbuf, werr = want
    assert gret == wret
    assert list(gres) == list(wres)
    if wret < len(rg):
        assert gerr == werr
    covered = np.zeros(nbytes, bool)
    for q, res in zip(rg, gres):
        a, c = int(q["dst_off"]), int(q["count"])
        covered[a: a + c] = True
        if res > 0:
            assert bytes(gbuf[a: a + res]) == bytes(wbuf[a: a + res])
            if data is not None:
                assert bytes(gbuf[a: a + res]) == data[int(q["offset"]): int(q["offset"]) + res]
    assert (gbuf[~covered] == SENT).all()      # guard zones untouched


@pytest.mark.parametrize("name", ["lz4_4k_direct", "lz4_64k_direct", "zstd_64k_direct"])
def test_vectored(gpu, zs, payloads, name):
    img, data = golden_file(name), payloads[name]
    t, ptr = _place(gpu, img, 17)
    with zs.Reader.open_device(ptr, len(img), 0) as r, zs.Reader(img, 0) as h:
        for rd in (r, h):
            rd.set_batch_bytes(256 << 10)      # several batches
        _, d_off = r.frames()
        rg, nbytes = _vec_ranges(d_off, 11)
        got, want = _preadv_both(zs, gpu, r, rg, nbytes), _preadv_both(zs, gpu, h, rg, nbytes)
        for g, w in zip(got, want):
            assert g[0] == len(rg)
            _check_vec(rg, nbytes, g, w, data)
        assert r.gpu_stats()["bytes_uploaded"] == 0 and h.gpu_stats()["bytes_uploaded"] > 0
        assert r.stats()["cached_frames"] == 0
    assert _guards_ok(t, 17, len(img))


def test_vectored_sparse_ranges_cut_by_span(gpu, zs, payloads):
    """Ranges in the first and the last frame: 128 KiB decoded, one batch by
    bytes, but ~540 KB apart in the image -- more than 4 x batch_bytes, so the
    device-image reader decodes them as two batches (frames in place are not
    packed: its parse scratch follows the span).  Same bytes either way."""
    name = "lz4_64k_direct"
    img, data = golden_file(name), payloads[name]
    t, ptr = _place(gpu, img, 5)
    with zs.Reader.open_device(ptr, len(img), 0) as r, zs.Reader(img, 0) as h:
        c_off, d_off = r.frames()
        n = len(d_off) - 1
        assert int(c_off[n]) - int(c_off[0]) > 4 * (128 << 10)
        rg = [(int(d_off[n - 1]) + 11, 3000), (100, 5000), (int(d_off[n - 1]) + 40000, 10**6), (65000, 400)]
        want = [data[o: o + c] for o, c in rg]
        before = {}
        for rd in (r, h):
            rd.set_batch_bytes(128 << 10)
            before[rd] = rd.gpu_stats()["batches"]
            got, n_ok = rd.preadv(rg)
            assert n_ok == len(rg) and got == want
        assert h.gpu_stats()["batches"] - before[h] == 1
        assert r.gpu_stats()["batches"] - before[r] == 2
        assert r.gpu_stats()["frames_decoded"] == h.gpu_stats()["frames_decoded"] == 2
        assert r.gpu_stats()["bytes_uploaded"] == 0


def test_vectored_corrupt_middle_frame(gpu, zs, golden):
    """frame_magic: frame 1 of 16 fails.  Results, delivered bytes, errbuf and
    guard zones equal the host-image reader's."""
    rec = golden["corrupt"]["frame_magic"]
    img = _mutated(rec)
    t, ptr = _place(gpu, img, 1)
    with zs.Reader.open_device(ptr, len(img), 0) as r, zs.Reader(img, 0) as h:
        _, d_off = r.frames()
        rg, nbytes = _vec_ranges(d_off, 12)
        got, want = _preadv_both(zs, gpu, r, rg, nbytes), _preadv_both(zs, gpu, h, rg, nbytes)
        for g, w in zip(got, want):
            assert 0 <= g[0] < len(rg)
            assert g[3] == "decompress frame: ERROR_frameType_unknown"
            assert (g[1] == -1).any() and (g[1] > 0).any()
            _check_vec(rg, nbytes, g, w)


# ---------------------------------------------------------------------------
# a seek table that points outside the image
# ---------------------------------------------------------------------------
def _inflated(img: bytes, frame: int, by: int) -> bytes:
    """The file with `by` added to frame `frame`'s cSize entry (8-byte entries
    before the 9-byte footer): every later frame's c_off moves by that much."""
    b = bytearray(img)
    assert b[-5] == 0                                   # no checksums: 8-byte entries
    n = int.from_bytes(b[-9:-5], "little")
    at = len(b) - 9 - 8 * (n - frame)
    b[at: at + 4] = (int.from_bytes(b[at: at + 4], "little") + by).to_bytes(4, "little")
    return bytes(b)


@pytest.mark.parametrize("name", ["lz4_64k_direct", "zstd_64k_direct"])
@pytest.mark.parametrize("cache", [0, 1])
def test_table_past_end_of_image(gpu, zs, payloads, name, cache):
    """One cSize entry inflated by the file's size: frame 3 and everything after
    it lie past the end of the image.  Open succeeds (the table is only
    summed); a read whose batch reaches frame 3 gets what the host-image reader
    gets, -1 "unexpected EOF" (there the pread comes back short), and nothing
    is decoded from outside the image; reads before frame 3 are exact."""
    good, data = golden_file(name), payloads[name]
    img = _inflated(good, 3, len(good))
    t, ptr = _place(gpu, img, 7, 4096)
    with zs.Reader.open_device(ptr, len(img), cache) as r, zs.Reader(img, cache) as h:
        _, d_off = r.frames()
        d = [int(x) for x in d_off]
        n = len(d) - 1
        reads = [(0, d[n]), (d[1] + 5, d[5]), (d[3], 100), (d[3] + 1000, 100), (d[4], 100), (d[n - 1] + 9, 50),
                 (d[2] + 10, d[3] - d[2] - 10), (0, d[3])]
        for off, cnt in reads:
            q = {"offset": off, "count": cnt}
            ret, out, err = _pread(r, q)
            hret, hout, herr = _pread(h, q)
            assert (ret, err) == (hret, herr), q
            assert bytes(out) == bytes(hout), q
            if off + cnt <= d[3]:
                assert ret == cnt and bytes(out[:ret]) == data[off: off + cnt], q
            else:       # (one batch: its whole span is read, or checked, at once)
                assert ret == -1 and err == "unexpected EOF", q
        rg = [(d[4] + 1, 100), (10, 100), (d[3] + 7, 9), (d[2] + 1, 2 * 65536), (d[n - 1], 10)]
        for device in (False, True):
            res = []
            for rd in (r, h):
                a = zs.Reader._ranges(rg)
                buf = np.full(int(a["count"].sum()) + 64, SENT, np.uint8)
                if device:
                    import torch
                    dbuf = torch.from_numpy(buf.copy()).to(gpu)
                    ret = rd.preadv_raw(dbuf.data_ptr(), a, device=True)
                    buf = dbuf.cpu().numpy()
                else:
                    ret = rd.preadv_raw(buf.ctypes.data, a)
                res.append((ret, list(a["result"]), bytes(buf), rd.error))
            assert res[0] == res[1]
            assert res[0][0] == -1 and res[0][3] == "unexpected EOF" and set(res[0][1]) == {-1}
        assert r.gpu_stats()["bytes_uploaded"] == 0
    assert _guards_ok(t, 7, len(img))


def test_vectored_batch_spanning_2gib(gpu, zs, payloads):
    """Three frames: a golden's first frame, 2 GiB + 4 KiB that no read touches,
    the golden's second frame.  Ranges in the first and the last: by default the
    planner's span cut (4 x 64 MiB) makes them two batches and both are read;
    with 1 GiB batches they are one batch 2 GiB wide, which the parse kernels'
    32-bit resources cannot address: the call is refused, nothing is decoded."""
    import struct

    import torch
    name = "lz4_64k_direct"
    good, data = golden_file(name), payloads[name]
    c_off, d_off = zs.seek_table_of(np.frombuffer(good, np.uint8))
    c = [int(x) for x in c_off[:3]]
    gap = (2 << 30) + 4096
    table = struct.pack("<II", 0x184D2A5E, 3 * 8 + 9)
    table += struct.pack("<II", c[1], 65536) + struct.pack("<II", gap, 1) + struct.pack("<II", c[2] - c[1], 65536)
    table += struct.pack("<IBI", 3, 0, 0x8F92EAB1)
    size = c[1] + gap + (c[2] - c[1]) + len(table)
    t = torch.empty(size, dtype=torch.uint8, device=gpu)      # (the gap's bytes are never read)
    f0 = torch.from_numpy(np.frombuffer(good[: c[2]], np.uint8).copy()).to(gpu)
    t[: c[1]].copy_(f0[: c[1]])
    t[c[1] + gap: c[1] + gap + c[2] - c[1]].copy_(f0[c[1]:])
    t[size - len(table):].copy_(torch.from_numpy(np.frombuffer(table, np.uint8).copy()).to(gpu))
    torch.cuda.synchronize()
    rg = [(65536 + 1 + 100, 3000), (50, 700)]                 # the last frame starts at 65537
    want = [data[65536 + 100:][:3000], data[50:750]]
    with zs.Reader.open_device(t.data_ptr(), size, 0) as r:
        assert r.stats()["frames"] == 3
        got, n_ok = r.preadv(rg)
        assert n_ok == 2 and got == want
        assert r.gpu_stats()["batches"] == 2 and r.gpu_stats()["frames_decoded"] == 2
        r.set_batch_bytes(1 << 30)
        with pytest.raises(zs.ZseekError) as e:
            r.preadv(rg)
        assert str(e.value) == "vectored read: a batch spans 2 GiB of the device image"
        assert r.gpu_stats()["frames_decoded"] == 2
        assert r.pread(700, 50) == want[1]                    # a contiguous read is not affected
        assert r.gpu_stats()["bytes_uploaded"] == 0


# ---------------------------------------------------------------------------
# seek-table checksums from the resident table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("codec", ["lz4", "zstd"])
@pytest.mark.parametrize("cache", [0, 1])
def test_checksums(gpu, zs, oracle, payloads, codec, cache):
    name = "lz4_64k_direct" if codec == "lz4" else "zstd_64k_direct"
    plain, data = np.frombuffer(golden_file(name), np.uint8), payloads[name]
    _, d_off = zs.seek_table_of(plain)
    want = np.array([oracle.xxh64(data[int(d_off[i]): int(d_off[i + 1])]) & 0xFFFFFFFF
                     for i in range(len(d_off) - 1)], np.uint32)
    good = zs.with_frame_checksums(plain, want).tobytes()
    t, ptr = _place(gpu, good, 2)
    with zs.Reader.open_device(ptr, len(good), cache) as r:
        r.set_verify_checksums(True)
        r.set_batch_bytes(192 << 10)        # the words of a later batch: at f0 of the table
        assert r.read_all(len(data), 0) == data
        assert r.pread(1000, 70000) == data[70000:71000]
        got, n_ok = r.preadv([(int(d_off[k]) + 3, 100) for k in (5, 2, 7)])
        assert n_ok == 3 and got == [data[int(d_off[k]) + 3:][:100] for k in (5, 2, 7)]
    want[5] ^= 1
    bad = zs.with_frame_checksums(plain, want).tobytes()
    t, ptr = _place(gpu, bad, 2)
    with zs.Reader.open_device(ptr, len(bad), cache) as r:      # default off
        assert r.read_all(len(data), 0) == data
    with zs.Reader.open_device(ptr, len(bad), cache) as r, zs.Reader(bad, cache) as h:
        for rd in (r, h):
            rd.set_verify_checksums(True)
            rd.set_batch_bytes(192 << 10)
        for q in ({"count": len(data), "offset": 0}, {"count": 100, "offset": int(d_off[5]) + 7},
                  {"count": 100, "offset": int(d_off[6])}, {"count": 70000, "offset": int(d_off[4]) + 5}):
            ret, out, err = _pread(r, q)
            hret, hout, herr = _pread(h, q)
            assert (ret, err, bytes(out[: max(ret, 0)])) == (hret, herr, bytes(hout[: max(ret, 0)])), q
        ret, out, err = _pread(r, {"count": len(data), "offset": 0})
        assert ret == int(d_off[5]) and bytes(out[:ret]) == data[:ret]
        ret, out, err = _pread(r, {"count": 100, "offset": int(d_off[5]) + 7})
        assert ret == -1 and err.endswith(": frame checksum mismatch")
        got, n_ok = r.preadv([(int(d_off[4]), 10), (int(d_off[5]), 10)])
        assert n_ok == 1 and got[1] is None and r.error.endswith(": frame checksum mismatch")
        assert r.gpu_stats()["bytes_uploaded"] == 0


# ---------------------------------------------------------------------------
# lanes
# ---------------------------------------------------------------------------
def test_lanes(gpu, zs, payloads):
    import torch
    name = "lz4_64k_direct"
    img, data = golden_file(name), payloads[name]
    t, ptr = _place(gpu, img, 0)
    dev = gpu.index
    with zs.Reader.open_device(ptr, len(img), 0) as r:
        assert r.devices() == [dev]                  # before any read
        assert r.gpu_stats()["device"] == dev
        r.set_devices([dev])
        for bad in ([dev, dev], [torch.cuda.device_count()], [dev + 1], [-1], []):
            with pytest.raises(zs.ZseekError):
                r.set_devices(bad)
        assert r.devices() == [dev]
        r.set_io_threads(8)                          # accepted, no effect
        assert r.pread(len(data), 0) == data
        assert r.read(1000) == data[:1000] and r.read(70000) == data[1000:71000]   # zseek_read's cursor
        assert r.devices() == [dev]
        assert r.gpu_stats()["bytes_uploaded"] == 0


def test_not_device_memory(gpu, zs):
    img = np.frombuffer(golden_file("lz4_64k_direct"), np.uint8).copy()
    with pytest.raises(zs.ZseekError) as e:
        zs.Reader.open_device(img.ctypes.data, img.size, 0)
    assert str(e.value) == "open device image: not device memory"
    with pytest.raises(zs.ZseekError) as e:
        zs.Reader.open_device(None, 100, 0)
    assert str(e.value) == "open device image: not device memory"
