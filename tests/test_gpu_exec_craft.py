"""The execute kernels on tests/exec_craft.py's hand-built dependency
structures: every decode goes into a buffer prefilled with 0xA5, and the only
yardstick is status 0 and exact equality with expand's bytes (held to the
oracle, the libraries and the reference reader by test_exec_craft.py, which
also proves from the model that every case reaches what it is named for).

Which execute an engine of zsk_lz4_decode_frames reaches:
  lean, scan, chunk   seq_exec_kernel<kExecStage = 3072, false>: the cases
                      built for W = 3072 are on its edges (scan pads a pair
                      off slot 63: the model's pad=True)
  block               seq_exec_kernel<4096, true> over the block route's job
                      lists: the cases built for W = 4096
  one                 seq_exec_frame_kernel (frames up to 64 KiB: families a-f),
                      seq_exec_big_kernel (family g; its first block decodes
                      short, so the block plan declines the frame) and
                      seq_exec_blocks_kernel
  None, wave          the default route and the one-wave decoder: no aimed
                      case, the same bytes
zstd: batches of up to 64 frames take seq_exec_frame_kernel, bigger ones
seq_exec_kernel<4096, false> with the literal scratch (W = 4096 cases); a
frame over 64 KiB in a small batch takes the wave kernel through min_dsize.
Every case must pass everywhere."""
from __future__ import annotations

import numpy as np
import pytest

import exec_craft as ec
import lz4_craft
import zstd_craft
from exec_craft import NAMES, case, zget
from lz4_linked_craft import decode

pytestmark = pytest.mark.gpu

ENGINES = [None, "wave", "lean", "scan", "chunk", "block", "one"]
SENT = 0xA5
FAMILIES = "abcdefg"
Z_FAMILIES = "acdfh"


def _check(zs, rows, got, st):
    bad = [(c[0], zs.status_string(s)) for c, s in zip(rows, st) if s != 0]
    assert not bad, bad[:12]
    bad = [c[0] for c, g in zip(rows, got) if g != c[3]]
    assert not bad, (len(bad), bad[:12])


@pytest.fixture(scope="module")
def randoms():
    return [(f"random{i}", f, len(w), w) for i, (f, w, _) in enumerate(ec.random_exec(3, 300))]


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("engine", ENGINES)
def test_lz4_family(gpu, zs, engine, fam):
    """each family as one batch, all seven engines"""
    rows = [case(n) for n in NAMES if n[0] == fam]
    if fam == "g":      # the stuck path: an item longer than the window
        rows.append(lz4_craft.CASE["a_bsid5_match_end_cap-6"])
    got, st = decode(zs, gpu, [c[1] for c in rows], [c[2] for c in rows], engine)
    _check(zs, rows, got, st)


@pytest.mark.parametrize("engine", ENGINES)
def test_lz4_shuffled(gpu, zs, randoms, engine):
    """the table and 300 random_exec frames in a seeded shuffle: neighbouring
    waves of a workgroup hold very different batches"""
    pool = [case(n) for n in NAMES] + randoms
    rng = np.random.default_rng(17)
    pool = [pool[i] for i in rng.permutation(len(pool))]
    got, st = decode(zs, gpu, [c[1] for c in pool], [c[2] for c in pool], engine)
    _check(zs, pool, got, st)


def _guard_layout(rows, desc_dtype):
    """64 guard bytes at both ends, a gap of 1..16 bytes before each frame,
    frame starts at every alignment modulo 16"""
    n = len(rows)
    desc = np.zeros(n, desc_dtype)
    at, c_at = 64, 0
    for i, (_, f, ds, _) in enumerate(rows):
        d_off = at + 1 + (i - (at + 1)) % 16
        assert d_off > at and d_off % 16 == i % 16
        desc[i] = (c_at, d_off, len(f), ds)
        at, c_at = d_off + ds, c_at + len(f)
    total = at + 64
    want = np.full(total, SENT, np.uint8)
    for d, c in zip(desc, rows):
        want[int(d["d_off"]): int(d["d_off"]) + c[2]] = np.frombuffer(c[3], np.uint8)
    return desc, c_at, total, want


def _guard_report(rows, desc, out, want):
    bad = np.nonzero(out != want)[0]
    if bad.size:
        ends = desc["d_off"] + desc["d_size"]
        where = [(int(b), rows[int(np.searchsorted(ends, b, side="right"))][0] if b < ends[-1] else "guard")
                 for b in bad[:8]]
        pytest.fail(f"{bad.size} bytes differ, first (offset, frame at or after it): {where}")


LZ4_DESC = [("c_off", "<u8"), ("d_off", "<u8"), ("c_size", "<u4"), ("d_size", "<u4")]


@pytest.mark.parametrize("engine", ["lean", "one"])
def test_lz4_output_guard(gpu, zs, engine):
    """the craft suites' guard test on this table (every output alignment is
    every a0 of the model): no byte outside a frame's [d_off, d_off + d_size)
    changes, every byte inside is expand's"""
    import torch
    rows = [case(n) for n in NAMES]
    desc, c_at, total, want = _guard_layout(rows, LZ4_DESC)
    td = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    comp = torch.zeros(c_at + 256, dtype=torch.uint8, device=gpu)
    comp[:c_at].copy_(torch.from_numpy(np.frombuffer(b"".join(c[1] for c in rows), np.uint8).copy()))
    out = torch.full((total,), SENT, dtype=torch.uint8, device=gpu)
    status = torch.full((len(rows),), -1, dtype=torch.int32, device=gpu)
    zs.decode_frames(td, comp, out, status, engine=engine)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(rows)
    _guard_report(rows, desc, out.cpu().numpy(), want)


# ---------------------------------------------------------------------------
# zstd
# ---------------------------------------------------------------------------
def _zrows(fam):
    return [zget(n) for n in ec.ZALL if n[0] == fam]


def _zdecode(zs, gpu, rows, form):
    """the rows back to back into 0xA5 through zsk_zstd_decode_frames or its
    async form -> (each row's output slot, statuses)"""
    import torch
    if form == "sync":
        return zstd_craft.decode(zs, gpu, [c[1] for c in rows], [c[2] for c in rows], fill=SENT)
    n = len(rows)
    c = np.cumsum([0] + [len(r[1]) for r in rows])
    d = np.cumsum([0] + [r[2] for r in rows])
    desc = np.zeros(n, zs.FRAME_DESC_DTYPE)
    desc["c_off"], desc["d_off"] = c[:-1], d[:-1]
    desc["c_size"], desc["d_size"] = np.diff(c), np.diff(d)
    td = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    comp = torch.zeros(int(c[-1]) + 256, dtype=torch.uint8, device=gpu)
    comp[: int(c[-1])].copy_(torch.from_numpy(np.frombuffer(b"".join(r[1] for r in rows), np.uint8).copy()))
    out = torch.full((max(int(d[-1]), 1),), SENT, dtype=torch.uint8, device=gpu)
    status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    zs.zstd_decode_frames_async(td, comp, out, status)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return [o[int(d[i]): int(d[i + 1])].tobytes() for i in range(n)], status.cpu().tolist()


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("fam", Z_FAMILIES)
def test_zstd_family_small_batches(gpu, zs, fam, form):
    """each family in batches of up to 64 frames: seq_exec_frame_kernel; the
    h frames over 64 KiB take the wave kernel through min_dsize"""
    rows = _zrows(fam)
    assert rows
    for at in range(0, len(rows), 64):
        got, st = _zdecode(zs, gpu, rows[at: at + 64], form)
        _check(zs, rows[at: at + 64], got, st)


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("fam", Z_FAMILIES)
def test_zstd_family_wave(gpu, zs, fam, form):
    """the same frames repeated past 64 per batch: seq_exec_kernel<4096, false>
    with the literal scratch"""
    rows = _zrows(fam)
    rows = rows * (-(-70 // len(rows)))
    assert len(rows) > 64
    got, st = _zdecode(zs, gpu, rows, form)
    _check(zs, rows, got, st)


def test_zstd_shuffled(gpu, zs):
    """the zstd table and 100 random_exec frames in a seeded shuffle, one
    batch"""
    pool = [zget(n) for n in ec.ZALL]
    pool += [(f"random{i}", f, len(w), w) for i, (f, w, _) in enumerate(ec.random_exec(5, 100, "zstd"))]
    rng = np.random.default_rng(19)
    pool = [pool[i] for i in rng.permutation(len(pool))]
    got, st = _zdecode(zs, gpu, pool, "sync")
    _check(zs, pool, got, st)


@pytest.mark.parametrize("per_batch", [64, 0])
def test_zstd_output_guard(gpu, zs, per_batch):
    """the guard layout for the zstd table; per_batch 64: the frame kernel, 0:
    one batch, the wave execute"""
    import torch
    rows = [zget(n) for n in ec.ZALL]
    desc, c_at, total, want = _guard_layout(rows, zs.FRAME_DESC_DTYPE)
    comp = torch.zeros(c_at + 256, dtype=torch.uint8, device=gpu)
    comp[:c_at].copy_(torch.from_numpy(np.frombuffer(b"".join(c[1] for c in rows), np.uint8).copy()))
    out = torch.full((total,), SENT, dtype=torch.uint8, device=gpu)
    status = torch.full((len(rows),), -1, dtype=torch.int32, device=gpu)
    step = per_batch or len(rows)
    for lo in range(0, len(rows), step):
        td = torch.from_numpy(desc[lo: lo + step].view(np.uint8).copy()).to(gpu)
        zs.zstd_decode_frames(td, comp, out, status[lo: lo + step])
        torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(rows)
    _guard_report(rows, desc, out.cpu().numpy(), want)


# ---------------------------------------------------------------------------
# stop_last: a cache-0 read that ends inside the image's last frame
# ---------------------------------------------------------------------------
TINY = 70
STOP_CASES = {
    # 70 tiny frames before it: the wave execute; its model batch ends
    "wave": (["d_chain63_ml16_w3072", "b_ovl_ml5000_off17_after", "a_pair_unfit_twice_w3072"], TINY),
    # alone: the frame kernel; its 2,048-item windows' ends
    "frame": (["f_items4097", "f_pair_at2047", "f_chain64k"], 0),
    # alone, over 64 KiB: the window kernel; its batches' decoded ends
    "big": (["g_three_quarters+0", "g_sources_at_h", "g_pair_is_cut"], 0),
}


def _stop_ends(name, kind):
    st = ec.stats(name, ec.W_LZ4)
    if kind == "wave":
        ends = [b["end"] for b in st["batches"]]
    elif kind == "frame":
        ends = [p for _, p in st["frame"]["windows"][1:]]
    else:
        ends = [b["P"] for b in st["big"]["batches"]]
    ends = sorted({e for e in ends if 1 < e < st["total"]})
    assert ends, name
    if len(ends) > 8:      # the first, the last and six spread between them
        ends = sorted({ends[i] for i in np.linspace(0, len(ends) - 1, 8).astype(int)})
    return ends


@pytest.mark.parametrize("kind", list(STOP_CASES))
def test_stop_last(gpu, zs, kind):
    """A craft frame last in a seekable image, read without a cache by
    requests that end at a model batch end (window end), one byte before and
    one byte after it: the count comes back and the bytes are expand's."""
    names, ntiny = STOP_CASES[kind]
    tiny = [lz4_craft._build([[(lz4_craft.lits(9 + i % 5, i), 3, 6), (lz4_craft.lits(5, i), None, None)]])
            for i in range(ntiny)]
    for name in names:
        _, f, ds, want = case(name)
        img = lz4_craft.seekable([t[0] for t in tiny] + [f], [len(t[1]) for t in tiny] + [ds])
        whole = b"".join(t[1] for t in tiny) + want
        pre = len(whole) - ds
        with zs.Reader(img, 0) as r:
            for e in _stop_ends(name, kind):
                for end in (e - 1, e, e + 1):
                    buf = np.full(pre + end + 64, SENT, np.uint8)
                    n = r.pread_raw(buf.ctypes.data, pre + end, 0)
                    assert n == pre + end, (name, end, n, r.error)
                    assert buf[: n].tobytes() == whole[: n], (name, end)
                    assert (buf[n:] == SENT).all(), (name, end)
