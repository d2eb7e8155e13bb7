"""The seven LZ4 decode engines and the four read paths on tests/lz4_craft.py's
hand-built frames: sequence streams that sit on the block format's end-of-block
rules, history floor and capacity, on every length-encoding edge and on the
sizes where the engines change path -- inputs no compressor writes.

The yardsticks: expand's bytes (a byte-by-byte model, lz4_craft.py), the
oracle (held to liblz4 1.9.3's record on the same frames by test_lz4_craft.py)
and the compiled reference reader's recorded answers (golden/lz4_craft.json)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import lz4_craft
from conftest import GOLDEN, sha
from lz4_craft import CASES, check, decode

pytestmark = pytest.mark.gpu

ENGINES = [None, "wave", "lean", "scan", "chunk", "block", "one"]
SENT = 0xA5
UNSET = -7777

VALID = [c for c in CASES if c[3] is not None]
REJECTED = [c for c in CASES if c[3] is None]


@pytest.fixture(scope="module")
def verdicts(oracle):
    """the oracle on every case, once: accepted cases to expand's bytes,
    rejected ones refused"""
    for name, f, ds, want in CASES:
        st, got, _, _ = oracle.decode_frame(f, ds)
        assert (st == 0 and len(got) == ds) == (want is not None), name
        assert want is None or got == want, name
    return True


def _names(idx, cases):
    return [cases[i][0] for i in idx][:12]


@pytest.mark.parametrize("engine", ENGINES)
def test_valid_cases(gpu, zs, verdicts, engine):
    """every accepted case in one batch: status 0 and the oracle's bytes"""
    got, st = decode(zs, gpu, [c[1] for c in VALID], [c[2] for c in VALID], engine)
    bad = [i for i, s in enumerate(st) if s != 0]
    assert not bad, [(VALID[i][0], zs.status_string(st[i])) for i in bad][:12]
    bad = [i for i, c in enumerate(VALID) if got[i] != c[3]]
    assert not bad, _names(bad, VALID)


@pytest.mark.parametrize("engine", ENGINES)
def test_valid_cases_shuffled(gpu, zs, oracle, verdicts, engine):
    """the accepted cases (the small ones repeated to 300 frames, the big ones
    once) and 200 generated frames in a seeded shuffle: the lanes of one wave
    hold very different frames, frame counts cross 64 and 256"""
    rng = np.random.default_rng(11)
    small = [c for c in VALID if len(c[1]) <= 8192]
    pool = small + [small[i] for i in rng.integers(0, len(small), 300 - len(small))]
    pool += [c for c in VALID if len(c[1]) > 8192]
    pool += [(f"random{i}", f, len(w), w) for i, (f, w) in enumerate(lz4_craft.random_valid(7, 200))]
    pool = [pool[i] for i in rng.permutation(len(pool))]
    assert len(pool) > 500
    got, st = decode(zs, gpu, [c[1] for c in pool], [c[2] for c in pool], engine)
    bad = [i for i, s in enumerate(st) if s != 0]
    assert not bad, [(pool[i][0], zs.status_string(st[i])) for i in bad][:12]
    bad = [i for i, c in enumerate(pool) if got[i] != c[3]]
    assert not bad, _names(bad, pool)


@pytest.mark.parametrize("engine", ENGINES)
def test_rejected_cases(gpu, zs, oracle, verdicts, engine):
    """every rejected case between accepted ones: refused frames have a
    nonzero status (the wave engine's), accepted frames status 0 and their
    bytes -- the neighbours of a refused frame included.  (What a refused
    frame left in its own slot is not looked at.)"""
    small = [c for c in VALID if len(c[1]) <= 8192]
    batch = []
    for i, c in enumerate(REJECTED):
        batch += [small[(7 * i) % len(small)], c]
    batch.append(small[3])
    frames, dsizes = [c[1] for c in batch], [c[2] for c in batch]
    st = check(zs, oracle, gpu, frames, dsizes, engine)
    assert [s != 0 for s in st] == [c[3] is None for c in batch], \
        [(c[0], zs.status_string(s)) for c, s in zip(batch, st) if (s != 0) != (c[3] is None)]
    got, _ = decode(zs, gpu, frames, dsizes, engine)
    bad = [i for i, c in enumerate(batch) if c[3] is not None and got[i] != c[3]]
    assert not bad, _names(bad, batch)


@pytest.mark.parametrize("engine", ENGINES)
def test_output_guard(gpu, zs, verdicts, engine):
    """the accepted frames into a buffer of 0xA5 with 64 guard bytes at both
    ends, a gap of 1..16 bytes before each frame and frame starts at every
    alignment modulo 16: no byte outside a frame's [d_off, d_off + d_size)
    changes (an over-store of one byte lands in a gap or a guard)"""
    import torch
    n = len(VALID)
    desc = np.zeros(n, dtype=[("c_off", "<u8"), ("d_off", "<u8"), ("c_size", "<u4"), ("d_size", "<u4")])
    at, c_at = 64, 0
    for i, (_, f, ds, _) in enumerate(VALID):
        d_off = at + 1 + (i - (at + 1)) % 16
        assert d_off > at and d_off % 16 == i % 16
        desc[i] = (c_at, d_off, len(f), ds)
        at, c_at = d_off + ds, c_at + len(f)
    total = at + 64
    want = np.full(total, SENT, np.uint8)
    for d, c in zip(desc, VALID):
        want[int(d["d_off"]): int(d["d_off"]) + c[2]] = np.frombuffer(c[3], np.uint8)
    td = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    comp = torch.zeros(c_at + 256, dtype=torch.uint8, device=gpu)
    comp[:c_at].copy_(torch.from_numpy(np.frombuffer(b"".join(c[1] for c in VALID), np.uint8).copy()))
    out = torch.full((total,), SENT, dtype=torch.uint8, device=gpu)
    status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    zs.decode_frames(td, comp, out, status, engine=engine)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    bad = np.nonzero(out.cpu().numpy() != want)[0]
    if bad.size:
        ends = desc["d_off"] + desc["d_size"]
        where = [(int(b), VALID[int(np.searchsorted(ends, b, side="right"))][0] if b < ends[-1] else "guard")
                 for b in bad[:8]]
        pytest.fail(f"{bad.size} bytes differ, first (offset, frame at or after it): {where}")


# ---------------------------------------------------------------------------
# the read paths
# ---------------------------------------------------------------------------
def _pread_loop(r, total):
    out = np.empty(total + 1, np.uint8)
    pos = 0
    while True:
        n = r.pread_raw(out.ctypes.data + pos, max(total - pos, 1), pos)
        if n <= 0:
            return out[:pos].tobytes(), n
        pos += n


def test_reader_paths(gpu, zs, oracle, verdicts):
    """Each case between two intact frames in a seekable file, through
    zseek_pread under a caller's loop (cache 0 and 1: the reference reader's
    recorded bytes, last return value and error text), zsk_preadv with one
    range per frame (a refused frame's range is -1, the others complete, the
    error text the cached read's) and, on the same image in device memory,
    zsk_preadv_device_async and zsk_preadv_device_indirect (the same results,
    left in device memory).  The reference spins where a frame's seek-table
    size disagrees with what it decodes; there the oracle decides: refused."""
    import torch
    with open(os.path.join(GOLDEN, "lz4_craft.json")) as f:
        record = json.load(f)["cases"]
    (fa, a), (fb, b) = lz4_craft.NEIGHBOURS
    S = torch.cuda.Stream(device=gpu)
    for (name, frame, dsize, want), rec in zip(CASES, record):
        assert rec["name"] == name and rec["frame_sha"] == sha(frame)
        ref = rec["reference"]
        img = lz4_craft.seekable([fa, frame, fb], [len(a), dsize, len(b)])
        total = len(a) + dsize + len(b)
        whole = a + want + b if want is not None else None
        for cache in (0, 1):
            with zs.Reader(img, cache) as r:
                got, last = _pread_loop(r, total)
                if want is not None:
                    assert (got, last) == (whole, 0), (name, cache)
                else:
                    assert (got, last) == (a, -1), (name, cache, last)
                if ref != "hang":
                    w = ref[f"cache{cache}"]
                    assert (len(got), sha(got), last) == (w["bytes"], w["sha"], w["last"]), (name, cache)
                    assert last == 0 or r.error == w["error"], (name, cache, r.error)
        # one range per frame, destinations apart
        rg = np.zeros(3, zs.RANGE_DTYPE)
        rg["offset"], rg["count"] = [0, len(a), len(a) + dsize], [len(a), dsize, len(b)]
        rg["dst_off"] = [3, 3 + len(a) + 5, 3 + len(a) + 5 + dsize + 2]
        nbytes = int(rg["dst_off"][2]) + len(b) + 7
        results = [len(a), dsize if want is not None else -1, len(b)]
        n_ok = 3 if want is not None else 2
        exp = np.full(nbytes, SENT, np.uint8)
        look = np.ones(nbytes, bool)
        for q, part in zip(rg, (a, want, b)):
            if part is None:
                look[int(q["dst_off"]): int(q["dst_off"]) + dsize] = False     # a refused frame's own destination
            else:
                exp[int(q["dst_off"]): int(q["dst_off"]) + len(part)] = np.frombuffer(part, np.uint8)
        with zs.Reader(img, 0) as r:
            buf = np.full(nbytes, SENT, np.uint8)
            ret = r.preadv_raw(buf.ctypes.data, rg)
            assert (ret, rg["result"].tolist()) == (n_ok, results), (name, r.error)
            assert not ((buf != exp) & look).any(), name
            if want is None and ref != "hang":
                assert r.error == ref["cache1"]["error"], name
        keep = torch.from_numpy(np.frombuffer(img, np.uint8).copy()).to(gpu)
        d_rg = torch.from_numpy(rg.view(np.uint8).copy()).to(gpu)
        r = zs.Reader.open_device(keep.data_ptr(), len(img), 0)
        try:
            for path in ("async", "indirect"):
                d_buf = torch.full((nbytes + 64,), SENT, dtype=torch.uint8, device=gpu)
                d_res = torch.full((4,), UNSET, dtype=torch.int64, device=gpu)
                torch.cuda.synchronize()
                if path == "async":
                    r.preadv_device_async(d_buf.data_ptr(), rg, d_res.data_ptr(), S.cuda_stream)
                else:
                    r.preadv_device_indirect(d_buf.data_ptr(), nbytes, d_rg.data_ptr(), 3, 3, d_res.data_ptr(),
                                             S.cuda_stream)
                S.synchronize()
                assert d_res.cpu().tolist() == results + [n_ok], (name, path)
                h = d_buf.cpu().numpy()
                assert (h[nbytes:] == SENT).all(), (name, path)
                assert not ((h[:nbytes] != exp) & look).any(), (name, path)
        finally:
            r.close()
