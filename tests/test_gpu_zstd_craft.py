"""The zstd decoder (zsk_zstd_decode_frames' routes) and the read paths on
tests/zstd_craft.py's hand-built entries: every frame-header form, block
type, literals form, Huffman description, sequence-table mode, count form and
repeat-offset rule -- inputs no compressor writes.

The yardsticks: expand's bytes (a byte-by-byte model, zstd_craft.py), libzstd
1.4.9's recorded error code per entry and the compiled reference reader's
recorded answers (golden/zstd_craft.json).  Live libzstd is not called here.
An accepted entry has status 0 and expand's bytes; a rejected one exactly
ZSK_STATUS_ZSTD | libzstd's code (ZSK_ERR_SHORT_FRAME where it only decodes
short of its declared size); the entries of zstd_craft.DIVERGENT, where this
decoder departs from libzstd on purpose, the status pinned
there.

zsk_preadv_device_async and zsk_preadv_device_indirect refuse a zstd reader
(test_gpu_preadv_async.py, test_gpu_preadv_indirect.py pin that), so the image
in device memory is read through zsk_preadv_device instead."""
from __future__ import annotations

import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import zstd_craft
from conftest import GOLDEN, sha
from zstd_craft import CASES, DIVERGENT, DIVERGENT_BYTES, NO_CACHE_DIVERGENT, SHORT, ZSK_STATUS_ZSTD, decode

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENT = 0xA5
UNSET = -7777
ZSK_ERR_SHORT_FRAME = 101


def want_status(c) -> int:
    if c[0] in DIVERGENT:
        return DIVERGENT[c[0]]
    if c[3] is not None:
        return 0
    return ZSK_ERR_SHORT_FRAME if c[4] == SHORT else ZSK_STATUS_ZSTD | c[4]


def want_bytes(c):
    """expand's bytes; where the decoder departs from libzstd with status 0,
    the bytes its own rule gives (worked out by the model too)"""
    return c[3] if c[3] is not None else DIVERGENT_BYTES.get(c[0])


def accepted(c) -> bool:
    """status 0 and bytes to compare"""
    return want_status(c) == 0 and want_bytes(c) is not None


SMALL = [c for c in CASES if c[2] <= 4096 and len(c[1]) <= 8192]
VALID = [c for c in CASES if accepted(c)]


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_zstd_craft", os.path.join(GOLDEN, "make_zstd_craft.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def record(maker):
    with open(os.path.join(GOLDEN, "zstd_craft.json")) as f:
        rec = maker.unpack(json.load(f))
    assert [(r["name"], r["entry_sha"], r["dsize"]) for r in rec] == [(c[0], sha(c[1]), c[2]) for c in CASES]
    for c, r in zip(CASES, rec):      # the table's verdicts are the record's
        assert r["code"] == (0 if c[4] == SHORT else c[4]), c[0]
        assert c[3] is None or r["sha"] == sha(c[3]), c[0]
    return rec


def check_batch(zs, gpu, batch):
    """the batch decoded: every entry's exact status, every accepted entry's
    bytes (so a rejected entry's neighbours are untouched)"""
    got, st = decode(zs, gpu, [c[1] for c in batch], [c[2] for c in batch])
    bad = [(i, c[0], zs.status_string(s), zs.status_string(want_status(c)))
           for i, (c, s) in enumerate(zip(batch, st)) if s != want_status(c)]
    bad += [(i, c[0], "bytes differ") for i, (c, g) in enumerate(zip(batch, got)) if accepted(c) and g != want_bytes(c)]
    if bad:
        print(len(bad), "wrong:", bad)
    return bad


def test_one_frame_route(gpu, zs, record):
    """batches of 64 entries or fewer (the one-frame route), each case once"""
    bad = []
    for at in range(0, len(CASES), 64):
        bad += check_batch(zs, gpu, CASES[at: at + 64])
    assert not bad, bad[:12]


def test_lane_route(gpu, zs, record):
    """all cases in one batch (the lane route: 65 entries or more)"""
    bad = check_batch(zs, gpu, CASES)
    assert not bad, bad[:12]


@pytest.mark.parametrize("n", [4096 + 130, 16384 + 130])
def test_chunked_batches(gpu, zs, record, n):
    """a seeded shuffle of the small cases repeated past 4,096 entries (two
    pipelined chunks) and past 16,384 (three)"""
    rng = np.random.default_rng(n)
    pool = [SMALL[i] for i in rng.permutation(len(SMALL))]
    pool += [SMALL[i] for i in rng.integers(0, len(SMALL), n - len(pool))]
    assert len(pool) == n and sum(not accepted(c) for c in pool) > n // 10
    bad = check_batch(zs, gpu, pool)
    assert not bad, bad[:12]


@pytest.mark.parametrize("per_batch", [64, 2000])
def test_random_valid(gpu, zs, per_batch):
    """the generator's 2,000 valid entries (every table mode, treeless
    literals, several frames and header forms in an entry), 64 per batch (the
    one-frame route) and in one batch (the lane route): status 0 and expand's
    bytes"""
    entries = zstd_craft.random_valid(1, 2000)
    bad = []
    for lo in range(0, len(entries), per_batch):
        part = entries[lo: lo + per_batch]
        got, st = decode(zs, gpu, [e for e, _ in part], [len(w) for _, w in part])
        bad += [(lo + i, zs.status_string(s)) for i, s in enumerate(st) if s != 0]
        bad += [(lo + i, "bytes differ") for i, ((_, w), g) in enumerate(zip(part, got)) if g != w]
    assert not bad, bad[:12]


@pytest.mark.parametrize("k", [1, 2, 31, 33, 65])
def test_partial_waves_after_full_batch(gpu, zs, record, k):
    """k crafted entries right after a 64-entry batch: what the pooled buffers
    keep of the larger batch must not reach the smaller one"""
    rng = np.random.default_rng(k)
    first = [SMALL[i] for i in rng.integers(0, len(SMALL), 64)]
    then = [SMALL[i] for i in rng.integers(0, len(SMALL), k)]
    bad = check_batch(zs, gpu, first) + check_batch(zs, gpu, then)
    assert not bad, bad[:12]


@pytest.mark.parametrize("per_batch", [64, 0])
def test_output_guard(gpu, zs, record, per_batch):
    """the accepted entries into a buffer of 0xA5 with 64 guard bytes at both
    ends, a gap of 1..16 bytes before each entry and entry starts at every
    alignment modulo 16: no byte outside an entry's [d_off, d_off + d_size)
    changes.  per_batch 64: the one-frame route; 0: one batch, the lane route."""
    import torch
    n = len(VALID)
    desc = np.zeros(n, zs.FRAME_DESC_DTYPE)
    at, c_at = 64, 0
    for i, (_, f, ds, _, _) in enumerate(VALID):
        d_off = at + 1 + (i - (at + 1)) % 16
        assert d_off > at and d_off % 16 == i % 16
        desc[i] = (c_at, d_off, len(f), ds)
        at, c_at = d_off + ds, c_at + len(f)
    total = at + 64
    want = np.full(total, SENT, np.uint8)
    for d, c in zip(desc, VALID):
        want[int(d["d_off"]): int(d["d_off"]) + c[2]] = np.frombuffer(want_bytes(c), np.uint8)
    comp = torch.zeros(c_at + 256, dtype=torch.uint8, device=gpu)
    comp[:c_at].copy_(torch.from_numpy(np.frombuffer(b"".join(c[1] for c in VALID), np.uint8).copy()))
    out = torch.full((total,), SENT, dtype=torch.uint8, device=gpu)
    status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    step = per_batch or n
    for lo in range(0, n, step):
        td = torch.from_numpy(desc[lo: lo + step].view(np.uint8).copy()).to(gpu)
        zs.zstd_decode_frames(td, comp, out, status[lo: lo + step])
        torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    bad = np.nonzero(out.cpu().numpy() != want)[0]
    if bad.size:
        ends = desc["d_off"] + desc["d_size"]
        where = [(int(b), VALID[int(np.searchsorted(ends, b, side="right"))][0] if b < ends[-1] else "guard")
                 for b in bad[:8]]
        pytest.fail(f"{bad.size} bytes differ, first (offset, entry at or after it): {where}")


# ---------------------------------------------------------------------------
# the fallback switches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["ZSEEK_ONE_FUSE=0", "ZSEEK_FRAME_HELP=0", "ZSEEK_ONE_ROUTE=0"])
def test_switches(gpu, record, switch):
    """each switch changes the kernels the small batches run on; in a fresh
    process (zstd_craft_probe.py) the statuses and bytes are the record's"""
    env = dict(os.environ)
    k, v = switch.split("=")
    env[k] = v
    p = subprocess.run([sys.executable, os.path.join(HERE, "zstd_craft_probe.py")], env=env, capture_output=True,
                       text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert list(got) == [c[0] for c in CASES]
    bad = [(c[0], got[c[0]][0], want_status(c)) for c in CASES if got[c[0]][0] != want_status(c)]
    bad += [(c[0], "bytes differ") for c in CASES if accepted(c) and got[c[0]][1] != sha(want_bytes(c))]
    if bad:
        print(switch, len(bad), "wrong:", bad)
    assert not bad, bad[:12]


# ---------------------------------------------------------------------------
# the read paths
# ---------------------------------------------------------------------------
ANY = object()      # an entry delivered with bytes that are not looked at


def readable(c) -> bool:
    """the reader delivers the entry (one of no bytes is never decoded)"""
    return want_status(c) == 0 or c[2] == 0


def content(c):
    return want_bytes(c) if accepted(c) else b"" if c[2] == 0 else ANY


def _pread_loop(r, total):
    out = np.empty(total + 1, np.uint8)
    pos = 0
    while True:
        n = r.pread_raw(out.ctypes.data + pos, max(total - pos, 1), pos)
        if n <= 0:
            return out[:pos].tobytes(), n
        pos += n


@pytest.mark.parametrize("cache", [0, 1])
def test_pread_loop(gpu, zs, record, cache):
    """Each case between two intact entries in a seekable file, through
    zseek_pread under a caller's loop: the reference reader's recorded bytes,
    last return value and error text.  The reference spins where an entry's
    seek-table size is more than it decodes to; there the oracle's verdict
    (held to libzstd's in test_zstd_craft.py) decides: refused.  Without a
    cache the reference decodes with libzstd's streaming calls; the entries of
    NO_CACHE_DIVERGENT, where this reader gives the one-call decoder's verdict
    instead, are held to the answers pinned there."""
    (fa, a), (fb, b) = zstd_craft.NEIGHBOURS
    bad = []
    for c, rec in zip(CASES, record):
        name, entry, dsize = c[0], c[1], c[2]
        img = zstd_craft.seekable([fa, entry, fb], [len(a), dsize, len(b)])
        total = len(a) + dsize + len(b)
        with zs.Reader(img, cache) as r:
            got, last = _pread_loop(r, total)
            err = r.error if last < 0 else ""
        refused = {"bytes": len(a), "sha": sha(a), "last": -1, "error": None}
        if name in DIVERGENT:
            w = refused if DIVERGENT[name] else {"bytes": total, "sha": sha(a + want_bytes(c) + b), "last": 0, "error": ""}
        elif cache == 0 and name in NO_CACHE_DIVERGENT:
            all_, rv, text = NO_CACHE_DIVERGENT[name]
            w = {"bytes": total if all_ else len(a), "sha": sha(a + c[3] + b) if all_ else sha(a), "last": rv, "error": text}
        elif rec["reference"] == "hang":
            w = refused
        else:
            w = rec["reference"][cache]
        if (len(got), last) != (w["bytes"], w["last"]) or (w["sha"] is not None and sha(got) != w["sha"]) \
                or (w["error"] is not None and err != w["error"]):
            bad.append((name, len(got), last, err, w["bytes"], w["last"], w["error"]))
    if bad:
        print(len(bad), "wrong (name, got bytes, last, error, wanted bytes, last, error):", bad)
    assert not bad, bad[:8]


def _ranges(zs, sizes):
    """one range per entry, destinations apart -> (ranges, buffer bytes)"""
    rg = np.zeros(len(sizes), zs.RANGE_DTYPE)
    off = np.cumsum([0] + list(sizes))
    rg["offset"], rg["count"] = off[:-1], sizes
    at = 3
    for i, s in enumerate(sizes):
        rg["dst_off"][i] = at
        at += s + 1 + i % 7
    return rg, at + 7


def _expect(rg, nbytes, parts):
    """parts: per range its bytes, or None where the range is refused ->
    (expected buffer, the bytes to look at, results, ranges delivered)"""
    exp = np.full(nbytes, SENT, np.uint8)
    look = np.ones(nbytes, bool)
    results = []
    for q, part in zip(rg, parts):
        d, n = int(q["dst_off"]), int(q["count"])
        if part is None or part is ANY:
            look[d: d + n] = False      # a refused entry's own destination
            results.append(-1 if part is None else n)
        else:
            exp[d: d + n] = np.frombuffer(part, np.uint8)
            results.append(n)
    return exp, look, results, sum(p is not None for p in parts)


def test_preadv(gpu, zs, record):
    """zsk_preadv with one range per entry of the three-entry image: a
    refused entry's range is -1, the others complete; the error text is the
    cached read's"""
    (fa, a), (fb, b) = zstd_craft.NEIGHBOURS
    bad = []
    for c, rec in zip(CASES, record):
        name, entry, dsize = c[0], c[1], c[2]
        sizes = [len(a), dsize, len(b)]
        img = zstd_craft.seekable([fa, entry, fb], sizes)
        rg, nbytes = _ranges(zs, sizes)
        exp, look, results, n_ok = _expect(rg, nbytes, [a, content(c) if readable(c) else None, b])
        with zs.Reader(img, 0) as r:
            buf = np.full(nbytes, SENT, np.uint8)
            ret = r.preadv_raw(buf.ctypes.data, rg)
            if (ret, rg["result"].tolist()) != (n_ok, results):
                bad.append((name, ret, rg["result"].tolist(), r.error))
            elif ((buf != exp) & look).any():
                bad.append((name, "bytes differ"))
            elif not readable(c) and name not in DIVERGENT and rec["reference"] != "hang" \
                    and r.error != rec["reference"][1]["error"]:
                bad.append((name, r.error, rec["reference"][1]["error"]))
    if bad:
        print(len(bad), "wrong:", bad)
    assert not bad, bad[:8]


def _device_read(zs, gpu, img, rg, nbytes):
    """zsk_preadv_device on the image in device memory -> (return value,
    results, the destination buffer and 64 bytes after it)"""
    import torch
    keep = torch.from_numpy(np.frombuffer(img, np.uint8).copy()).to(gpu)
    d_buf = torch.full((nbytes + 64,), SENT, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    r = zs.Reader.open_device(keep.data_ptr(), len(img), 0)
    try:
        ret = r.preadv_raw(d_buf.data_ptr(), rg, device=True)
    finally:
        r.close()
    return ret, rg["result"].tolist(), d_buf.cpu().numpy()


def test_preadv_device(gpu, zs, record):
    """the three-entry image in device memory (zsk_reader_open_device)
    through zsk_preadv_device: the same results, left in device memory, nothing
    written outside the destination"""
    (fa, a), (fb, b) = zstd_craft.NEIGHBOURS
    bad = []
    for c in CASES:
        name, entry, dsize = c[0], c[1], c[2]
        sizes = [len(a), dsize, len(b)]
        img = zstd_craft.seekable([fa, entry, fb], sizes)
        rg, nbytes = _ranges(zs, sizes)
        exp, look, results, n_ok = _expect(rg, nbytes, [a, content(c) if readable(c) else None, b])
        ret, res, h = _device_read(zs, gpu, img, rg, nbytes)
        if (ret, res) != (n_ok, results):
            bad.append((name, ret, res, results))
        elif not (h[nbytes:] == SENT).all() or ((h[:nbytes] != exp) & look).any():
            bad.append((name, "bytes differ"))
    if bad:
        print(len(bad), "wrong:", bad)
    assert not bad, bad[:8]


@pytest.mark.parametrize("path", ["host", "device"])
def test_long_images(gpu, zs, record, maker, path):
    """each small case with 33 intact entries on each side (67 entries: past
    the one-frame route, so the reader's host plan, zstd_host_plan, sees
    the crafted entry among others; the device plan, zstd_plan_kernel, sees it
    in every zsk_zstd_decode_frames batch above), one range per entry in one
    vectored read, from a host image and from one in device memory"""
    nb = zstd_craft.NEIGHBOURS
    bad = []
    for c in SMALL:
        name, entry, dsize = c[0], c[1], c[2]
        img, sizes = maker.case_image(entry, dsize, around=33)
        parts = [nb[i % 2][1] for i in range(33)] + [content(c) if readable(c) else None] + \
                [nb[(i + 1) % 2][1] for i in range(33)]
        rg, nbytes = _ranges(zs, sizes)
        exp, look, results, n_ok = _expect(rg, nbytes, parts)
        if path == "host":
            with zs.Reader(img, 0) as r:
                buf = np.full(nbytes, SENT, np.uint8)
                ret = r.preadv_raw(buf.ctypes.data, rg)
                if (ret, rg["result"].tolist()) != (n_ok, results):
                    bad.append((name, ret, rg["result"].tolist()[33], r.error))
                elif ((buf != exp) & look).any():
                    bad.append((name, "bytes differ"))
            continue
        ret, res, h = _device_read(zs, gpu, img, rg, nbytes)
        if (ret, res) != (n_ok, results):
            bad.append((name, ret, res[33], results[33]))
        elif not (h[nbytes:] == SENT).all() or ((h[:nbytes] != exp) & look).any():
            bad.append((name, "bytes differ"))
    if bad:
        print(len(bad), "wrong:", bad)
    assert not bad, bad[:8]
