"""zsk_zstd_compress_frames_ex and ZSK_IMAGE_ZSTD_FULL (csrc/zstd_compress.hip,
csrc/zstd_enc_full_dev.h) on the GPU: the full format, and the subset path
beside it.

Judges, in order: libzstd 1.4.9 (zstd_util.decode) and the compiled reference
reader for whole files; oracle.zstd_decode; the project's GPU decoder.  Beyond
that the kernel's bytes must be the CPU shim's (tests/native/
zstd_enc_full_shim.cpp drives the same format layer serially), for both
formats, and the subset call must not have moved.

The helpers are test_gpu_zstd_compress.py's; every test asks for the `gpu`
fixture first, as there."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import zstd_util
from test_gpu_zstd_compress import CK, GUARD, MIB, SENT, _build, _contents, _frames, _judge, _source, _table

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
FULL_IMAGE = 4   # ZSK_IMAGE_ZSTD_FULL


@pytest.fixture(scope="module")
def zstd():
    z = zstd_util.load()
    if z is None:
        pytest.skip("libzstd 1.4.9 not present")
    return z


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("zstd_enc_full_gpu") / "libzstd_enc_full.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/zstd_enc_full_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.zenc_frame_bound.restype = C.c_uint64
    L.zenc_frame_bound.argtypes = [C.c_uint64]
    for fn in (L.zenc_compress, L.zenc_full_compress):
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64]

    def run(content: np.ndarray, checksum: bool, full: bool) -> bytes:
        src = np.ascontiguousarray(content) if content.size else np.zeros(1, np.uint8)
        cap = L.zenc_frame_bound(content.size)
        out = np.empty(cap, np.uint8)
        n = (L.zenc_full_compress if full else L.zenc_compress)(src.ctypes.data, content.size, int(checksum),
                                                               out.ctypes.data, cap)
        assert 0 < n <= cap
        return out[:n].tobytes()
    return run


def _compress(zs, gpu, src: np.ndarray, sizes, offsets=None, flags=None, guard=GUARD, runs=1, how="full"):
    """test_gpu_zstd_compress.py's _compress through one of the three calls: "full" (_ex, format 1),
    "ex0" (_ex, format 0) or "subset" (zsk_zstd_compress_frames)."""
    import torch
    desc, _ = zs.zstd_compress_layout(sizes, offsets, flags)
    slots = np.array([zs.zstd_compress_bound(int(n)) for n in desc["src_size"]], np.uint64)
    desc["dst_off"] = np.concatenate(([0], np.cumsum(slots + np.uint64(guard))[:-1])) if len(slots) else slots
    total = int((slots + np.uint64(guard)).sum())
    d_src = torch.from_numpy(np.ascontiguousarray(src)).to(gpu)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    fmt = {"full": 1, "ex0": 0}.get(how)
    scratch = torch.empty(max(zs.zstd_compress_scratch_size(len(desc), src.size, full=how == "full"), 1),
                          dtype=torch.uint8, device=gpu)
    outs, cs = [], None
    for _ in range(runs):
        d_dst = torch.full((max(total, 1),), SENT, dtype=torch.uint8, device=gpu)
        csize = torch.full((len(desc),), -1, dtype=torch.int32, device=gpu)
        args = (d_desc.data_ptr(), len(desc), d_src.data_ptr(), d_dst.data_ptr(), csize.data_ptr(),
                scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream)
        r = zs.lib().zsk_zstd_compress_frames(*args) if fmt is None else zs.lib().zsk_zstd_compress_frames_ex(*args, fmt)
        assert r == 0
        torch.cuda.synchronize()
        outs.append(d_dst.cpu().numpy())
        c = csize.cpu().numpy()
        assert cs is None or np.array_equal(cs, c)
        cs = c
    return desc, cs, outs


def _ten_contents(oracle, rng, n: int):
    """The existing eight contents of one size and two binary ones: the synthetic data with the top
    bit flipped, and the little-endian float32 of a smooth series."""
    synth = oracle.synth(max(n, 1) + 65536, 7)[65536:][:n]
    t = np.arange(n // 4 + 1, dtype=np.float64)
    smooth = (np.sin(t / 97.0) * 1000.0 + t * 0.25).astype("<f4").view(np.uint8)[:n]
    return _contents(oracle, rng, n) + [synth ^ np.uint8(0x80), smooth.copy()]


@pytest.fixture(scope="module")
def batch(oracle, zs):
    """The edge batch's input: the existing file's sizes with ten contents each, 100 random sizes with
    one content each, frames at odd addresses, the checksum flag on every other frame."""
    zb = zs.ZSTD_BLOCK
    rng = np.random.default_rng(99)
    fixed = [0, 1, 2, 3, 4, 5, 8, 255, 256, 257, 4096, zb - 1, zb, zb + 1, 2 * zb + 999, 65535, 65536, 65537]
    rand = [int(2 ** rng.uniform(0, 18)) for _ in range(30)] + [int(2 ** rng.uniform(0, 13)) for _ in range(70)]
    parts = []
    for n in fixed:
        parts += _ten_contents(oracle, rng, n)
    for i, n in enumerate(rand):
        parts.append(_ten_contents(oracle, rng, n)[i % 10])
    sizes = [p.size for p in parts]
    src = np.concatenate([np.full(3, 0x11, np.uint8)] + parts)
    assert src.size <= 12 * MIB
    offsets = 3 + np.concatenate(([0], np.cumsum(sizes)[:-1]))
    flags = [(f & 1) * CK for f in range(len(sizes))]
    return {"parts": parts, "sizes": sizes, "src": src, "offsets": offsets, "flags": flags}


@pytest.fixture(scope="module")
def edge(gpu, zs, batch):
    desc, cs, outs = _compress(zs, gpu, batch["src"], batch["sizes"], batch["offsets"], batch["flags"], runs=2)
    return {"desc": desc, "cs": cs, "outs": outs}


def test_full_edge_batch(gpu, zs, zstd, oracle, shim, batch, edge):
    frames = _frames(zs, edge["desc"], edge["cs"], edge["outs"][0])          # (inside the slot, guards intact)
    assert np.array_equal(edge["outs"][0], edge["outs"][1]), "two runs are byte-identical"
    for f, (frame, part) in enumerate(zip(frames, batch["parts"])):
        assert bool(frame[4] & 4) == bool(f & 1), "the content-checksum bit only where asked for"
        _judge(zstd, oracle, frame, part.tobytes(), (f, part.size))
        assert frame == shim(part, bool(f & 1), True), (f, part.size, "GPU bytes != CPU shim bytes")
    assert len(frames[0]) == 9 and batch["parts"][0].size == 0
    # the binary contents compress: the row of 2 * zb + 999 bytes
    n = 2 * zs.ZSTD_BLOCK + 999
    base = 10 * 14
    assert batch["parts"][base].size == n
    # (the flipped text as the text itself; of a float the exponent byte and part of the next code short)
    assert len(frames[base + 8]) < n // 2 and len(frames[base + 9]) < n


def test_subset_path_untouched(gpu, zs, shim, batch, edge):
    """zsk_zstd_compress_frames and _ex with format 0 give the same bytes: the subset shim's."""
    args = (batch["src"], batch["sizes"], batch["offsets"], batch["flags"])
    desc, cs, outs = _compress(zs, gpu, *args, how="subset")
    desc0, cs0, outs0 = _compress(zs, gpu, *args, how="ex0")
    assert np.array_equal(cs, cs0) and np.array_equal(outs[0], outs0[0])
    frames = _frames(zs, desc, cs, outs[0])
    for f, (frame, part) in enumerate(zip(frames, batch["parts"])):
        assert frame == shim(part, bool(f & 1), False), (f, part.size)
    assert not np.array_equal(outs[0], edge["outs"][0]), "the two formats differ"


def test_ratio(gpu, zs, oracle):
    """128 frames of 64 KiB of the synthetic data, plain and with the top bit of every byte flipped."""
    fs = 65536
    data = oracle.synth(8 * MIB, 1)
    total = {}
    for name, src in (("plain", data), ("xor", data ^ np.uint8(0x80))):
        for how in ("subset", "full"):
            _, cs, _ = _compress(zs, gpu, src, [fs] * 128, guard=0, how=how)
            assert (cs > 0).all()
            total[name, how] = int(cs.sum())
            print("%-5s %-6s %9d bytes  %.4f of the input" % (name, how, total[name, how], total[name, how] / src.size))
    print("full xor / full plain = %.5f" % (total["xor", "full"] / total["plain", "full"]))
    assert total["plain", "full"] < total["plain", "subset"]
    assert total["xor", "full"] <= 1.01 * total["plain", "full"]
    assert total["xor", "full"] < total["xor", "subset"]


@pytest.mark.parametrize("nframes", [40, 300])
def test_full_round_trip_through_the_gpu_decoder(gpu, zs, oracle, nframes):
    import torch
    fs = 65536
    data = oracle.synth(8 * MIB, 1)[: min(nframes, 128) * fs] ^ np.uint8(0x80 if nframes == 40 else 0)
    sizes = [fs] * nframes
    offsets = [(i % 128) * fs for i in range(nframes)]
    desc, _ = zs.zstd_compress_layout(sizes, offsets)
    total = int(desc["dst_off"][-1]) + zs.zstd_compress_bound(fs)
    d_src = torch.from_numpy(data).to(gpu)
    d_dst = torch.zeros(total + 256, dtype=torch.uint8, device=gpu)
    csize = torch.zeros(nframes, dtype=torch.int32, device=gpu)
    zs.zstd_compress_frames(torch.from_numpy(desc.view(np.uint8).copy()).to(gpu), d_src, d_dst, csize, full=True)
    torch.cuda.synchronize()
    cs = csize.cpu().numpy()
    assert (cs > 0).all() and int(cs.sum()) < nframes * fs // 2
    fd = np.zeros(nframes, zs.FRAME_DESC_DTYPE)
    fd["c_off"], fd["c_size"], fd["d_size"] = desc["dst_off"], cs, fs
    fd["d_off"] = np.arange(nframes, dtype=np.uint64) * fs
    out = torch.full((nframes * fs,), SENT, dtype=torch.uint8, device=gpu)
    status = torch.full((nframes,), -1, dtype=torch.int32, device=gpu)
    zs.zstd_decode_frames(torch.from_numpy(fd.view(np.uint8).copy()).to(gpu), d_dst, out, status)
    torch.cuda.synchronize()
    assert int((status != 0).sum()) == 0
    got = out.view(nframes, fs)
    want = d_src.view(-1, fs)[torch.tensor([i % 128 for i in range(nframes)], device=gpu)]
    assert torch.equal(got, want)


@pytest.mark.parametrize("frame_size", [65536, MIB])
@pytest.mark.parametrize("flags", [0, 1, 3])
def test_build_image_full(gpu, zs, oracle, ref, zstd, frame_size, flags):
    import torch
    host, dev = _source(oracle, gpu)
    length = host.size
    n, err, t, cap, at = _build(zs, gpu, dev, length, frame_size, flags | FULL_IMAGE)
    assert 0 < n <= cap, err
    assert cap == zs.lib().zsk_zstd_image_bound(length, frame_size, flags), "the bound does not depend on the format"
    whole = t.cpu().numpy()
    assert (whole[: GUARD + at] == SENT).all() and (whole[GUARD + at + cap:] == SENT).all()
    image = whole[GUARD + at: GUARD + at + n].tobytes()
    nframes = -(-length // frame_size)
    entries, has_ck = _table(image)
    assert len(entries) == nframes and has_ck == bool(flags & 1)
    assert int(entries[:, 1].sum()) == length and int(entries[:, 0].sum()) + 17 + entries.size * 4 == n
    n_sub, _, _, _, _ = _build(zs, gpu, dev, length, frame_size, flags)
    assert n < n_sub, "the full format's file is the smaller one"
    c_at = 0
    for f in range(nframes):                                             # libzstd, frame by frame
        piece = host[f * frame_size: (f + 1) * frame_size].tobytes()
        frame = image[c_at: c_at + int(entries[f, 0])]
        assert bool(frame[4] & 4) == bool(flags & 2)
        if has_ck:
            assert int(entries[f, 2]) == oracle.xxh64(piece) & 0xFFFFFFFF
        assert zstd_util.decode(zstd, frame, len(piece)) == (piece, 0)
        c_at += int(entries[f, 0])
    for cache in (0, 1):                                                 # the reference reader
        r = ref.open(image, cache)
        assert r.h, r.error
        got = bytearray()
        while len(got) < length:
            k, b = r.pread(length - len(got), len(got))
            assert k > 0, r.error
            got += b
        r.close()
        assert bytes(got) == host.tobytes()
    d_image = t[GUARD + at: GUARD + at + n]                              # where it was built
    with zs.Reader.open_device(d_image.data_ptr(), n, 0) as r:
        assert r.type == zs.ZSEEK_ZSTD
        r.set_verify_checksums(True)
        out = torch.full((length + 32,), SENT, dtype=torch.uint8, device=gpu)
        assert r.pread_device(out.data_ptr(), length + 32, 0) == length
        assert torch.equal(out[:length], dev) and bool((out[length:] == SENT).all())
    # the wrapper's keyword, and the LZ4 builder ignores the bit
    image2 = zs.zstd_build_image(dev, frame_size, checksums=bool(flags & 1), content_checksums=bool(flags & 2),
                                 full=True)
    assert image2.cpu().numpy().tobytes() == image
    if frame_size == 65536 and flags == 0:
        import ctypes
        bound = zs.lib().zsk_lz4_image_bound(length, frame_size, 0)
        a = torch.zeros(bound, dtype=torch.uint8, device=gpu)
        b = torch.zeros(bound, dtype=torch.uint8, device=gpu)
        e = ctypes.create_string_buffer(80)
        na = zs.lib().zsk_lz4_build_image(dev.data_ptr(), length, frame_size, 0, 0, 0, a.data_ptr(), bound, e)
        nb = zs.lib().zsk_lz4_build_image(dev.data_ptr(), length, frame_size, 0, FULL_IMAGE, 0, b.data_ptr(), bound, e)
        assert na == nb > 0 and torch.equal(a[:na], b[:nb])


def test_refusals(gpu, zs, zstd, oracle):
    import torch
    L = zs.lib()
    t = torch.full((4096,), SENT, dtype=torch.uint8, device=gpu)
    desc, _ = zs.zstd_compress_layout([100])
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    csize = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    scratch = torch.empty(zs.zstd_compress_scratch_size(1, 100, full=True), dtype=torch.uint8, device=gpu)
    args = (d_desc.data_ptr(), 1, t.data_ptr(), t.data_ptr() + 2048, csize.data_ptr(), scratch.data_ptr())
    # an unknown format: -1, nothing queued
    for fmt in (2, -1, 99):
        assert L.zsk_zstd_compress_frames_ex(*args, scratch.numel(), None, fmt) == -1
    torch.cuda.synchronize()
    assert int(csize[0]) == -1 and bool((t == SENT).all())
    # a scratch one byte short
    assert L.zsk_zstd_compress_frames_ex(*args, L.zsk_zstd_compress_scratch_size_ex(1, 100, 1) - 1, None, 1) == -1
    torch.cuda.synchronize()
    assert int(csize[0]) == -1 and bool((t == SENT).all())
    assert L.zsk_zstd_compress_frames_ex(None, 0, None, None, None, None, 0, None, 1) == 0
    # a frame above 4 MiB: c_size 0 and the slot untouched; its neighbours are compressed
    cap = zs.ZSTD_COMPRESS_MAX_FRAME
    data = oracle.synth(cap + 1, 2)
    desc, cs, outs = _compress(zs, gpu, data, [cap, cap + 1, 100], offsets=[0, 0, 5], flags=[CK, 0, 0])
    host = outs[0]
    assert cs[1] == 0
    at = int(desc["dst_off"][1])
    assert (host[at: at + zs.zstd_compress_bound(cap + 1) + GUARD] == SENT).all(), "a refused slot is untouched"
    keep = [0, 2]
    frames = _frames(zs, desc[keep], cs[keep], host)
    _judge(zstd, oracle, frames[0], data[:cap].tobytes(), "4 MiB")
    _judge(zstd, oracle, frames[1], data[5:105].tobytes(), "100 bytes")
