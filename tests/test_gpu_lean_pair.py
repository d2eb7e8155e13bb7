"""The frame route's lean parse as parser and mover waves
(lz4_lean_pair_kernel): every frame through `engine="lean"`, decoded bytes
against the oracle, statuses against the wave engine.

The cases aim at what the split adds: partly filled and empty waves, the ring
restart after a long literal run (the mover learns of it one hand-off late),
the exact step beside a mover that runs ahead, item counts around the
16-item lines and the 32-slot buffer the two waves share, lanes of one wave
drifting apart, and failures at any point of a frame.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = 65536


def _exec_model():
    spec = importlib.util.spec_from_file_location("exec_model", os.path.join(ROOT, "scripts", "exec_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _image(zs, payloads) -> np.ndarray:
    """A seekable LZ4 image with one frame per payload (each 1..64 KiB)."""
    w = zs.Writer(min_frame_size=1)
    for p in payloads:
        w.write(np.ascontiguousarray(p, dtype=np.uint8).tobytes())
    return np.frombuffer(w.close(), np.uint8)


def _decode(zs, gpu, img, c_off, d_off, n, engine):
    import torch
    b = zs.frame_batch(c_off, d_off, 0, n)
    desc = torch.from_numpy(b.desc.view(np.uint8).copy()).to(gpu)
    comp = torch.zeros(b.comp_end + 256, dtype=torch.uint8, device=gpu)
    comp[: b.comp_end].copy_(torch.from_numpy(img[: b.comp_end].copy()))
    out = torch.zeros(max(b.out_bytes, 1), dtype=torch.uint8, device=gpu)
    status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    zs.decode_frames(desc, comp, out, status, engine=engine)
    torch.cuda.synchronize()
    return out.cpu().numpy()[: b.out_bytes], status.cpu().tolist()


def _check_image(zs, oracle, gpu, img):
    """Every frame valid: lean bytes == the oracle's, lean statuses == wave's == 0."""
    c_off, d_off = zs.seek_table_of(img)
    n = len(c_off) - 1
    out, st = _decode(zs, gpu, img, c_off, d_off, n, "lean")
    _, st_w = _decode(zs, gpu, img, c_off, d_off, n, "wave")
    assert st == st_w
    assert st == [0] * n
    assert out.tobytes() == oracle.decode_file(img.tobytes())


@pytest.fixture(scope="module")
def synth(zs):
    """513 compressible 64 KiB frames of the synthetic buffer (its first
    64 KiB are random bytes, a stored block: skipped here)."""
    return zs.synth_buffer(514 * FRAME)[FRAME:]


@pytest.fixture(scope="module")
def synth_case(zs, oracle, synth):
    img = zs.lz4_seekable(synth, FRAME)
    c_off, d_off = zs.seek_table_of(img)
    assert len(c_off) - 1 == 513
    ref = oracle.decode_file(img.tobytes())
    assert ref == synth.tobytes()
    return img, c_off, d_off, ref


@pytest.fixture(scope="module")
def kinds(zs, synth):
    """Payloads by kind, each at most 64 KiB."""
    rng = np.random.default_rng(7)
    rnd = rng.integers(0, 256, FRAME, dtype=np.uint8)
    rep = rng.integers(0, 256, FRAME, dtype=np.uint8)   # random, a short repeat every ~300 bytes
    at = 300
    while at + 24 < FRAME:
        m = int(rng.integers(6, 20))
        rep[at: at + m] = rep[at - 40: at - 40 + m]
        at += int(rng.integers(250, 350))
    em = _exec_model()
    base = synth[20 * FRAME: 21 * FRAME]

    def items(n):
        img = zs.lz4_seekable(base[:n], FRAME)
        c_off, _ = zs.seek_table_of(img)
        return sum(2 if (lit > 255 or ml > 258) else 1 for lit, ml, _ in em.sequences(img, c_off, 0))

    # truncations of one synthetic frame: item counts (about 1,500) in every
    # wanted residue modulo the 32-slot buffer, and small absolute counts
    # around one and two 16-item lines
    by_res, by_cnt = {}, {}
    n = FRAME
    while len(by_res) < 6 and n > FRAME // 2:
        r = items(n) % 32
        if r in (0, 1, 15, 16, 17, 31):
            by_res.setdefault(r, n)
        n -= 16
    n = 16
    while len(by_cnt) < 7 and n < FRAME // 2:
        c = items(n)
        if c in (1, 15, 16, 17, 31, 32, 33):
            by_cnt.setdefault(c, n)
        n += 8
    assert sorted(by_res) == [0, 1, 15, 16, 17, 31], by_res
    assert sorted(by_cnt) == [1, 15, 16, 17, 31, 32, 33], by_cnt
    return {
        "synth": [synth[i * FRAME: (i + 1) * FRAME] for i in range(8)],
        "jump": [rnd, rep],
        "exact": [np.full(FRAME, 7, np.uint8),
                  np.tile(rng.integers(0, 256, 5, dtype=np.uint8), FRAME // 5 + 1)[:FRAME],
                  np.tile(rng.integers(0, 256, 37, dtype=np.uint8), FRAME // 37 + 1)[:FRAME]],
        "edges": [base[:n] for n in list(by_res.values()) + list(by_cnt.values())] + [base[:1], base[:13]],
    }


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_frame_counts(gpu, zs, synth_case, n):
    """Partly filled waves, a mover with inactive lanes, wave and workgroup
    edges, a last workgroup with empty waves."""
    img, c_off, d_off, ref = synth_case
    out, st = _decode(zs, gpu, img, c_off, d_off, n, "lean")
    _, st_w = _decode(zs, gpu, img, c_off, d_off, n, "wave")
    assert st == st_w
    assert st == [0] * n
    assert out.tobytes() == ref[: n * FRAME]


@pytest.mark.parametrize("kind", ["jump", "exact", "edges"])
def test_kinds(gpu, zs, oracle, kinds, kind):
    """jump: literal runs longer than the ring (a stored block; random bytes
    with a short repeat every ~300).  exact: long extension chains (one byte
    value, periods 5 and 37).  edges: item counts 0, 1, 15, 16, 17, 31 modulo
    32, counts of exactly 1, 15, 16, 17, 31, 32, 33, frames of 1 and 13
    bytes."""
    _check_image(zs, oracle, gpu, _image(zs, kinds[kind]))


def test_empty_frame(gpu, zs, oracle):
    """A frame of 0 decoded bytes (header and end mark), alone and as the
    last lane beside a full frame."""
    empty = np.frombuffer(oracle.lz4f_compress_frame(b""), np.uint8)
    st0, data0, used, _ = oracle.decode_frame(empty.tobytes(), 0)
    assert (st0, data0, used) == (0, b"", empty.size)
    full = zs.synth_buffer(2 * FRAME)[FRAME:]
    fimg = zs.lz4_seekable(full, FRAME)
    fc, _ = zs.seek_table_of(fimg)
    fsz = int(fc[1])
    for with_full in (False, True):
        img = np.concatenate([fimg[:fsz], empty]) if with_full else empty
        cs = [fsz, empty.size] if with_full else [empty.size]
        ds = [FRAME, 0] if with_full else [0]
        c_off = np.concatenate([[0], np.cumsum(cs)]).astype(np.uint64)
        d_off = np.concatenate([[0], np.cumsum(ds)]).astype(np.uint64)
        out, st = _decode(zs, gpu, img, c_off, d_off, len(cs), "lean")
        _, st_w = _decode(zs, gpu, img, c_off, d_off, len(cs), "wave")
        assert st == st_w == [0] * len(cs)
        assert out.tobytes() == (full.tobytes() if with_full else b"")


def test_mixed_batch(gpu, zs, oracle, kinds):
    """About 300 frames alternating every kind: lanes of one wave drift far
    apart, one waiting on a flush while its neighbour waits on bytes."""
    pool = kinds["synth"] + kinds["jump"] + kinds["exact"] + kinds["edges"]
    order = np.random.default_rng(3).permutation(300) % len(pool)
    _check_image(zs, oracle, gpu, _image(zs, [pool[i] for i in order]))


def test_corruption(gpu, zs, synth):
    """Single-byte mutations across the frames' compressed blocks (twelve
    positions, four kinds of byte) on a 2 MiB image: the wave engine's
    status per frame, and its bytes for every frame it decodes."""
    rng = np.random.default_rng(21)
    data = np.concatenate([synth[: 24 * FRAME],
                           np.tile(rng.integers(0, 256, 11, dtype=np.uint8), 8 * FRAME // 11 + 1)[: 8 * FRAME]])
    img = zs.lz4_seekable(data, FRAME)
    c_off, d_off = zs.seek_table_of(img)
    n = len(c_off) - 1
    assert n == 32
    m = img.copy()
    fracs = [0.05, 0.3, 0.44, 0.47, 0.5, 0.52, 0.55, 0.6, 0.75, 0.9, 0.97, 0.995]
    for k, fr in enumerate(fracs * 4):
        f = 1 + (5 * k) % 31   # frame 0 stays intact; some frames take two mutations
        a, b = int(c_off[f]) + 11, int(c_off[f + 1]) - 4   # past the headers, before the end mark
        at = a + int((b - a) * fr)
        m[at] = [m[at] ^ 0x5A, 0xFF, 0x00, m[at] ^ 0x01][k // len(fracs)]
    out_w, st_w = _decode(zs, gpu, m, c_off, d_off, n, "wave")
    out_e, st_e = _decode(zs, gpu, m, c_off, d_off, n, "lean")
    assert st_e == st_w
    assert st_w[0] == 0 and any(s != 0 for s in st_w)
    for i in range(n):
        if st_w[i] == 0:
            a, b = int(d_off[i]), int(d_off[i + 1])
            assert (out_w[a:b] == out_e[a:b]).all(), i
