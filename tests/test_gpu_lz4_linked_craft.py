"""The seven LZ4 decode engines and the read paths on tests/lz4_linked_craft.py's
hand-built linked frames of full 64 KiB blocks: the inputs of the block route
and of the one-frame route's block-parallel execute (seq_exec_blocks_kernel),
whose tainted bytes -- copies from before a block, resolved by following
origins back block by block -- no compressor-made frame puts on their edges.

The yardsticks: expand's bytes (lz4_craft.py's byte-by-byte model), the oracle
(held to liblz4 1.9.3's record by test_lz4_linked_craft.py) and the compiled
reference reader's recorded answers (golden/lz4_linked_craft.json).  Every
decode goes into a buffer prefilled with 0xA5, so a tainted byte that is never
resolved, or never stored, cannot pass as a zero."""
from __future__ import annotations

import json
import os
import re

import numpy as np
import pytest

import lz4_craft
import lz4_linked_craft as lc
from conftest import GOLDEN, ROOT, sha
from lz4_linked_craft import B, SENT, case, decode, first_diff

pytestmark = pytest.mark.gpu

ENGINES = [None, "wave", "lean", "scan", "chunk", "block", "one"]
UNSET = -7777


@pytest.fixture(scope="module")
def table(oracle):
    """the table, built once, each case's verdict checked with the oracle:
    (accepted cases, rejected cases)"""
    cases = list(lc.CASES)
    for name, f, ds, want in cases:
        st, got, _, _ = oracle.decode_frame(f, ds)
        assert (st == 0 and len(got) == ds) == (want is not None), name
        assert want is None or got == want, name
    return [c for c in cases if c[3] is not None], [c for c in cases if c[3] is None]


@pytest.fixture(scope="module")
def generated(oracle):
    out = []
    for i, (f, want, _) in enumerate(lc.random_linked(5, 200)):
        st, got, _, _ = oracle.decode_frame(f, len(want))
        assert st == 0 and got == want, i
        out.append((f"random{i}", f, len(want), want))
    return out


def _hold(zs, gpu, cases, engine):
    """one batch: every status 0, every frame expand's bytes"""
    got, st = decode(zs, gpu, [c[1] for c in cases], [c[2] for c in cases], engine)
    bad = [i for i, s in enumerate(st) if s != 0]
    assert not bad, [(cases[i][0], zs.status_string(st[i])) for i in bad][:12]
    bad = [i for i, c in enumerate(cases) if got[i] != c[3]]
    # (per failing frame: how many bytes differ, the first one's block and position)
    assert not bad, [(cases[i][0], first_diff(got[i], cases[i][3])) for i in bad][:12]


@pytest.mark.parametrize("family", "abcdef")
@pytest.mark.parametrize("engine", ENGINES)
def test_valid_cases(gpu, zs, table, engine, family):
    """a family's accepted cases in one batch: status 0 and expand's bytes"""
    _hold(zs, gpu, [c for c in table[0] if c[0].startswith(family + "_")], engine)


@pytest.mark.parametrize("engine", ENGINES)
def test_valid_cases_shuffled(gpu, zs, table, generated, engine):
    """the accepted cases and 200 generated frames in a seeded shuffle, as two
    batches (about 65 MiB decoded each): frames of 2 and of 64 blocks next to
    each other, jobs of many frames in one grid"""
    rng = np.random.default_rng(23)
    pool = table[0] + generated
    pool = [pool[i] for i in rng.permutation(len(pool))]
    assert len(pool) > 700
    _hold(zs, gpu, pool[0::2], engine)
    _hold(zs, gpu, pool[1::2], engine)


@pytest.mark.parametrize("engine", ENGINES)
def test_rejected_cases(gpu, zs, oracle, table, engine):
    """every rejected case between accepted ones: a nonzero status exactly
    there (the wave engine's), the accepted neighbours status 0 and their
    bytes"""
    between = [case(n) for n in ("e_chain5_off65535", "a_straddle_k7_e15_gt", "d_tainted1025_v0", "f_dense_before",
                                 "c_chain_depth10_lanes")]
    batch = []
    for i, c in enumerate(table[1]):
        batch += [between[i], c]
    batch.append(between[4])
    assert len(table[1]) == 4
    frames, dsizes = [c[1] for c in batch], [c[2] for c in batch]
    st = lz4_craft.check(zs, oracle, gpu, frames, dsizes, engine)
    assert [s != 0 for s in st] == [c[3] is None for c in batch], \
        [(c[0], zs.status_string(s)) for c, s in zip(batch, st) if (s != 0) != (c[3] is None)]
    got, st2 = decode(zs, gpu, frames, dsizes, engine)
    assert st2 == st
    bad = [i for i, c in enumerate(batch) if c[3] is not None and got[i] != c[3]]
    assert not bad, [(batch[i][0], first_diff(got[i], batch[i][3])) for i in bad]


@pytest.mark.parametrize("engine", ["block", "one", None])
def test_output_guard(gpu, zs, table, engine):
    """the accepted frames into a buffer of 0xA5 with 64 guard bytes at both
    ends, a gap of 1..16 bytes before each frame and frame starts at every
    alignment modulo 16: no byte outside a frame's [d_off, d_off + d_size)
    changes, every byte inside is expand's"""
    import torch
    valid = table[0]
    n = len(valid)
    desc = np.zeros(n, dtype=[("c_off", "<u8"), ("d_off", "<u8"), ("c_size", "<u4"), ("d_size", "<u4")])
    at, c_at = 64, 0
    for i, (_, f, ds, _) in enumerate(valid):
        d_off = at + 1 + (i - (at + 1)) % 16
        assert at < d_off <= at + 16 and d_off % 16 == i % 16
        desc[i] = (c_at, d_off, len(f), ds)
        at, c_at = d_off + ds, c_at + len(f)
    total = at + 64
    want = np.full(total, SENT, np.uint8)
    for d, c in zip(desc, valid):
        want[int(d["d_off"]): int(d["d_off"]) + c[2]] = np.frombuffer(c[3], np.uint8)
    td = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    comp = torch.zeros(c_at + 256, dtype=torch.uint8, device=gpu)
    comp[:c_at].copy_(torch.from_numpy(np.frombuffer(b"".join(c[1] for c in valid), np.uint8).copy()))
    out = torch.full((total,), SENT, dtype=torch.uint8, device=gpu)
    status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    zs.decode_frames(td, comp, out, status, engine=engine)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    bad = np.nonzero(out.cpu().numpy() != want)[0]
    if bad.size:
        ends = desc["d_off"] + desc["d_size"]
        where = []
        for b in bad[:8]:
            i = int(np.searchsorted(ends, b, side="right"))
            where.append((int(b), "guard") if i == n else
                         (int(b), valid[i][0], "gap" if b < desc["d_off"][i] else int(b - desc["d_off"][i])))
        pytest.fail(f"{bad.size} bytes differ, first (offset, frame at or after it, position in it): {where}")


def test_origin_scratch_limit(gpu, zs, table):
    """Frames of 64 blocks, one more than fill the block-parallel execute's
    origin scratch (kOriginJobsMax jobs), in one batch of the one-frame route:
    the frames whose jobs lie inside the scratch go block-parallel, the rest
    through the windowed execute (seq_exec_big_kernel); all bytes right."""
    with open(os.path.join(ROOT, "libzseek_amd", "csrc", "lz4_route.h")) as f:
        limit = int(re.search(r"constexpr uint32_t kOriginJobsMax = (\d+);", f.read()).group(1))
    n = limit // 64 + 1
    assert (n - 1) * 64 <= limit < n * 64 and n == 17
    kinds = [c for c in table[0] if c[2] == 64 * B and c[0].startswith("e_")]
    assert len(kinds) == 4, [c[0] for c in kinds]      # the three chain offsets and the zeros
    _hold(zs, gpu, [kinds[i % 4] for i in range(n)], "one")


# ---------------------------------------------------------------------------
# the read paths
# ---------------------------------------------------------------------------
READ_VALID = ["e_chain5_off65535", "e_chain64_off65535", "c_t2u_ph7", "c_chain_depth10_lanes", "c_off3_run_prev"]


def _pread_loop(r, total):
    out = np.empty(total + 1, np.uint8)
    pos = 0
    while True:
        n = r.pread_raw(out.ctypes.data + pos, max(total - pos, 1), pos)
        if n <= 0:
            return out[:pos].tobytes(), n
        pos += n


def _read_ends(name, dsize):
    """where single reads from the frame's start end: 1 byte into block k, on
    its boundary and inside its first tainted run, for k in {1, 2, last}; and
    1 byte before the frame's end"""
    st = lc.taint_stats(lc.BLOCKS[name])
    ends = {dsize - 1}
    for k in {1, 2, len(st) - 1} & set(range(1, len(st))):
        ends |= {k * B, k * B + 1}
        if st[k]["matches"]:
            mb, _, ml, _, _ = st[k]["matches"][0]
            assert (st[k]["origin"][mb: mb + ml] >= 0).all()
            ends.add(k * B + mb + ml // 2)
    return sorted(ends)


def test_reader_paths(gpu, zs, table):
    """Chain frames of 5 and 64 blocks, three frames with later generations
    and the refused frames, each between lz4_craft's two intact neighbours in
    a seekable file.  zseek_pread under a caller's loop, cache 0 and 1: the
    reference reader's recorded bytes, last return value and error text.
    Single reads that end inside the frame (the last frame's stop: blocks past
    it skip, the block it is in goes out in part): the model's slice.  One
    zsk_preadv with a range per block, and the same through
    zsk_preadv_device_async on the image in device memory."""
    import torch
    with open(os.path.join(GOLDEN, "lz4_linked_craft.json")) as f:
        record = {c["name"]: c for c in json.load(f)["cases"]}
    (fa, a), (fb, b) = lz4_craft.NEIGHBOURS
    S = torch.cuda.Stream(device=gpu)
    for name, frame, dsize, want in [case(n) for n in READ_VALID] + table[1]:
        rec = record[name]
        assert rec["frame_sha"] == sha(frame)[:16]
        img = lz4_craft.seekable([fa, frame, fb], [len(a), dsize, len(b)])
        total = len(a) + dsize + len(b)
        for cache in (0, 1):
            with zs.Reader(img, cache) as r:
                got, last = _pread_loop(r, total)
                w = rec["reference"][f"cache{cache}"]
                assert (len(got), sha(got)[:16], last) == (w["bytes"], w["sha"], w["last"]), (name, cache)
                assert last == 0 or r.error == w["error"], (name, cache, r.error)
                assert got == (a + want + b if want is not None else a), (name, cache)
        if want is None:
            continue
        for cache in (0, 1):
            for end in _read_ends(name, dsize):
                with zs.Reader(img, cache) as r:       # (a fresh reader: nothing cached)
                    buf = np.full(end + 64, SENT, np.uint8)
                    n = r.pread_raw(buf.ctypes.data, end, len(a))
                    assert n == end, (name, cache, end, n, r.error)
                    assert buf[:end].tobytes() == want[:end], (name, cache, end, first_diff(buf[:end].tobytes(),
                                                                                            want[:end]))
                    assert (buf[end:] == SENT).all(), (name, cache, end)
        # a range per block, destinations apart
        nb = (dsize + B - 1) // B
        rg = np.zeros(nb, zs.RANGE_DTYPE)
        rg["offset"] = len(a) + B * np.arange(nb)
        rg["count"] = [min(B, dsize - B * k) for k in range(nb)]
        rg["dst_off"] = 3 + (B + 5) * np.arange(nb)
        nbytes = 3 + (B + 5) * nb
        exp = np.full(nbytes, SENT, np.uint8)
        for q in rg:
            o = int(q["offset"]) - len(a)
            exp[int(q["dst_off"]): int(q["dst_off"]) + int(q["count"])] = \
                np.frombuffer(want[o: o + int(q["count"])], np.uint8)
        with zs.Reader(img, 0) as r:
            buf = np.full(nbytes, SENT, np.uint8)
            ret = r.preadv_raw(buf.ctypes.data, rg)
            assert (ret, rg["result"].tolist()) == (nb, rg["count"].tolist()), (name, r.error)
            assert (buf == exp).all(), name
        keep = torch.from_numpy(np.frombuffer(img, np.uint8).copy()).to(gpu)
        r = zs.Reader.open_device(keep.data_ptr(), len(img), 0)
        try:
            d_buf = torch.full((nbytes + 64,), SENT, dtype=torch.uint8, device=gpu)
            d_res = torch.full((nb + 1,), UNSET, dtype=torch.int64, device=gpu)
            torch.cuda.synchronize()
            r.preadv_device_async(d_buf.data_ptr(), rg, d_res.data_ptr(), S.cuda_stream)
            S.synchronize()
            assert d_res.cpu().tolist() == rg["count"].tolist() + [nb], name
            h = d_buf.cpu().numpy()
            assert (h[nbytes:] == SENT).all() and (h[:nbytes] == exp).all(), name
        finally:
            r.close()
