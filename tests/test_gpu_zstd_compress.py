"""zsk_zstd_compress_frames and zsk_zstd_build_image (csrc/zstd_compress.hip,
csrc/image_build.hip) on the GPU.

Judges, in order: libzstd 1.4.9 itself (zstd_util.decode) and the compiled
reference reader for whole files; oracle.zstd_decode; the project's GPU
decoder.  The frames are not libzstd's bytes, so nothing here compares
compressed bytes with a library's: every frame must decode to its input, be
consumed whole, stay inside its slot, and be the same on every run.

Every test asks for the `gpu` fixture first, as the other GPU files do: torch
(and its HIP runtime) is loaded before the library."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

import zstd_util

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 64
MIB = 1 << 20
CK = 2   # ZSK_COMPRESS_CONTENT_CHECKSUM


@pytest.fixture(scope="module")
def zstd():
    z = zstd_util.load()
    if z is None:
        pytest.skip("libzstd 1.4.9 not present")
    return z


def _compress(zs, gpu, src: np.ndarray, sizes, offsets=None, flags=None, guard=GUARD, runs=1):
    """-> (descriptors, csize, [the whole dst on the host per run]): every slot
    is followed by `guard` bytes of 0xA5, the last one too."""
    import torch
    desc, _ = zs.zstd_compress_layout(sizes, offsets, flags)
    slots = np.array([zs.zstd_compress_bound(int(n)) for n in desc["src_size"]], np.uint64)
    desc["dst_off"] = np.concatenate(([0], np.cumsum(slots + np.uint64(guard))[:-1])) if len(slots) else slots
    total = int((slots + np.uint64(guard)).sum())
    d_src = torch.from_numpy(np.ascontiguousarray(src)).to(gpu)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    outs, cs = [], None
    for _ in range(runs):
        d_dst = torch.full((max(total, 1),), SENT, dtype=torch.uint8, device=gpu)
        csize = torch.full((len(desc),), -1, dtype=torch.int32, device=gpu)
        zs.zstd_compress_frames(d_desc, d_src, d_dst, csize)
        torch.cuda.synchronize()
        outs.append(d_dst.cpu().numpy())
        c = csize.cpu().numpy()
        assert cs is None or np.array_equal(cs, c)
        cs = c
    return desc, cs, outs


def _frames(zs, desc, cs, host, guard=GUARD):
    """The frames of one run, with the bound and the guard bytes checked."""
    out = []
    for f in range(len(desc)):
        at, n = int(desc["dst_off"][f]), int(desc["src_size"][f])
        bound = zs.zstd_compress_bound(n)
        assert 0 < cs[f] <= bound, (f, n, cs[f])
        assert (host[at + bound: at + bound + guard] == SENT).all(), (f, "guard")
        assert (host[at + cs[f]: at + bound] == SENT).all(), (f, "past the frame")
        out.append(host[at: at + cs[f]].tobytes())
    return out


def _judge(zstd, oracle, frame: bytes, content: bytes, what):
    got, err = zstd_util.decode(zstd, frame, len(content))
    assert err == 0 and got == content, ("libzstd", err, what)
    got, err = oracle.zstd_decode(frame, len(content))
    assert err == 0 and got == content, ("oracle", err, what)


def _contents(oracle, rng, n: int):
    """The eight contents of one size."""
    synth = oracle.synth(max(n, 1) + 65536, 7)[65536:][:n]
    rep = lambda k: np.tile(rng.integers(0, 256, k, dtype=np.uint8), n // k + 1)[:n]   # noqa: E731
    return [rng.integers(0, 256, n, dtype=np.uint8), np.zeros(n, np.uint8),
            rng.integers(0, 3, n, dtype=np.uint8) + 65, synth,
            np.repeat(rng.integers(128, 256, n // 5 + 1, dtype=np.uint8), 5)[:n], rep(14), rep(270), rep(70000)]


@pytest.fixture(scope="module")
def edge(gpu, zs, oracle):
    """The edge batch, compressed twice in one launch each: sizes at every
    boundary with all eight contents, 100 random sizes up to 256 KiB with one
    content each; the checksum flag on every other frame."""
    zb = zs.ZSTD_BLOCK
    rng = np.random.default_rng(99)
    fixed = [0, 1, 2, 3, 4, 5, 8, 255, 256, 257, 4096, zb - 1, zb, zb + 1, 2 * zb + 999, 65535, 65536, 65537]
    rand = [int(2 ** rng.uniform(0, 18)) for _ in range(30)] + [int(2 ** rng.uniform(0, 13)) for _ in range(70)]
    parts = []
    for n in fixed:
        parts += _contents(oracle, rng, n)
    for i, n in enumerate(rand):
        parts.append(_contents(oracle, rng, n)[i % 8])
    sizes = [p.size for p in parts]
    src = np.concatenate([np.full(3, 0x11, np.uint8)] + parts)          # frames start at odd addresses too
    assert src.size <= 8 * MIB
    offsets = 3 + np.concatenate(([0], np.cumsum(sizes)[:-1]))
    flags = [(f & 1) * CK for f in range(len(sizes))]
    desc, cs, outs = _compress(zs, gpu, src, sizes, offsets, flags, runs=2)
    return {"parts": parts, "desc": desc, "cs": cs, "outs": outs}


def test_edge_batch_decodes_everywhere(gpu, zs, zstd, oracle, edge):
    frames = _frames(zs, edge["desc"], edge["cs"], edge["outs"][0])
    for f, (frame, part) in enumerate(zip(frames, edge["parts"])):
        assert bool(frame[4] & 4) == bool(f & 1), "the content-checksum bit only where asked for"
        _judge(zstd, oracle, frame, part.tobytes(), (f, part.size))
    zero = frames[0]
    assert len(zero) == 9 and edge["parts"][0].size == 0


def test_edge_batch_is_deterministic(gpu, edge):
    assert np.array_equal(edge["outs"][0], edge["outs"][1])


def test_edge_batch_compresses_what_it_should(gpu, zs, edge):
    """zeros, the 3-symbol alphabet and the repeats shrink; nothing exceeds the bound (checked with the guards)."""
    frames = _frames(zs, edge["desc"], edge["cs"], edge["outs"][0])
    zb = zs.ZSTD_BLOCK
    base = 8 * 14                                    # the 2 * zb + 999 row
    n = 2 * zb + 999
    assert edge["parts"][base].size == n
    sizes = [len(frames[base + k]) for k in range(8)]
    assert sizes[0] > n                              # random: Raw blocks
    assert sizes[1] <= 9 + 3 * 4 + 4                 # zeros: three RLE blocks
    assert sizes[2] < n * 0.6 and sizes[3] < n // 2 and sizes[5] < n // 50 and sizes[6] < n // 50
    # (a 70000-byte period is beyond what the 4,096-entry table remembers: Raw, and still within the bound)


def test_checksum_flag_is_verified_by_libzstd(gpu, zs, zstd, edge):
    frames = _frames(zs, edge["desc"], edge["cs"], edge["outs"][0])
    f = next(i for i in range(1, len(frames), 2) if edge["parts"][i].size >= 255)
    frame, content = frames[f], edge["parts"][f].tobytes()
    assert frame[4] & 4
    assert zstd_util.decode(zstd, frame, len(content)) == (content, 0)
    bad = bytearray(frame)
    bad[len(bad) - 4] ^= 0x10                        # the stored checksum itself
    assert zstd_util.decode(zstd, bytes(bad), len(content)) == (b"", 22)   # ZSTD_error_checksum_wrong


def test_flipped_content_byte_is_a_checksum_error(gpu, zs, zstd):
    data = np.random.default_rng(3).integers(0, 256, 3000, dtype=np.uint8)     # a Raw block: content bytes in the clear
    desc, cs, outs = _compress(zs, gpu, data, [3000], flags=[CK])
    frame = _frames(zs, desc, cs, outs[0])[0]
    assert zstd_util.decode(zstd, frame, 3000) == (data.tobytes(), 0)
    bad = bytearray(frame)
    bad[7 + 3 + 1500] ^= 1
    assert zstd_util.decode(zstd, bytes(bad), 3000) == (b"", 22)


def test_largest_frame_and_refusal(gpu, zs, zstd, oracle):
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
    assert len(frames[0]) < cap // 2


def test_matches_stay_inside_their_frame(gpu, zs, zstd, oracle):
    """Sixteen identical frames back to back at odd addresses: a match into the frame before decodes wrong."""
    one = oracle.synth(65536 + 5000, 4)[65536:]
    src = np.concatenate([np.zeros(1, np.uint8)] + [one] * 16)
    desc, cs, outs = _compress(zs, gpu, src, [5000] * 16, offsets=[1 + 5000 * i for i in range(16)])
    frames = _frames(zs, desc, cs, outs[0])
    assert len(set(frames)) == 1
    _judge(zstd, oracle, frames[0], one.tobytes(), "frame")
    # scratch too small: refused before anything is queued
    import torch
    t = torch.zeros(64, dtype=torch.uint8, device=gpu)
    small = zs.zstd_compress_scratch_size(1, 64) - 1
    assert zs.lib().zsk_zstd_compress_frames(t.data_ptr(), 1, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                             small, None) == -1
    assert zs.lib().zsk_zstd_compress_frames(None, 0, None, None, None, None, 0, None) == 0


@pytest.mark.parametrize("nframes", [40, 300])
def test_round_trip_through_the_gpu_decoder(gpu, zs, oracle, nframes):
    import torch
    fs = 65536
    data = oracle.synth(8 * MIB, 1)[: min(nframes, 128) * fs]
    sizes = [fs] * nframes
    offsets = [(i % 128) * fs for i in range(nframes)]
    desc, _ = zs.zstd_compress_layout(sizes, offsets)
    total = int(desc["dst_off"][-1]) + zs.zstd_compress_bound(fs)
    d_src = torch.from_numpy(data).to(gpu)
    d_dst = torch.zeros(total + 256, dtype=torch.uint8, device=gpu)
    csize = torch.zeros(nframes, dtype=torch.int32, device=gpu)
    zs.zstd_compress_frames(torch.from_numpy(desc.view(np.uint8).copy()).to(gpu), d_src, d_dst, csize)
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


# -- zsk_zstd_build_image -------------------------------------------------------
_SRC = {}


def _source(oracle, gpu):
    import torch
    if not _SRC:
        _SRC["host"] = oracle.synth(3 * MIB + 777, 1)
        _SRC["dev"] = torch.from_numpy(_SRC["host"]).to(gpu)
        torch.cuda.synchronize()
    return _SRC["host"], _SRC["dev"]


def _build(zs, gpu, d_src, length, frame_size, flags=0, capacity=None, at=1):
    import torch
    if capacity is None:
        capacity = zs.lib().zsk_zstd_image_bound(length, frame_size, flags)
    t = torch.full((GUARD + at + capacity + GUARD,), SENT, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    err = C.create_string_buffer(80)
    n = zs.lib().zsk_zstd_build_image(d_src.data_ptr() if length else None, length, frame_size, flags, 0,
                                      t.data_ptr() + GUARD + at, capacity, err)
    return n, err.value.decode(), t, capacity, at


def _table(image: bytes):
    """-> (entries as rows of u32, has checksums) of the seek table at the file's end."""
    frames, desc, magic = struct.unpack("<IBI", image[-9:])
    assert magic == 0x8F92EAB1
    ew = 3 if desc & 0x80 else 2
    body = image[-9 - 4 * ew * frames: -9]
    assert struct.unpack("<II", image[-9 - len(body) - 8: -9 - len(body)]) == (0x184D2A5E, len(body) + 9)
    return np.frombuffer(body, "<u4").reshape(frames, ew), ew == 3


@pytest.mark.parametrize("frame_size", [65536, MIB])
@pytest.mark.parametrize("flags", [0, 1, 3])
def test_build_image(gpu, zs, oracle, ref, zstd, frame_size, flags):
    import torch
    host, dev = _source(oracle, gpu)
    length = host.size
    n, err, t, cap, at = _build(zs, gpu, dev, length, frame_size, flags)
    assert 0 < n <= cap, err
    whole = t.cpu().numpy()
    assert (whole[: GUARD + at] == SENT).all() and (whole[GUARD + at + cap:] == SENT).all()
    image = whole[GUARD + at: GUARD + at + n].tobytes()
    nframes = -(-length // frame_size)
    entries, has_ck = _table(image)
    assert len(entries) == nframes and has_ck == bool(flags & 1)
    assert int(entries[:, 1].sum()) == length and int(entries[:, 0].sum()) + 17 + entries.size * 4 == n
    c_at = 0
    for f in range(nframes):
        piece = host[f * frame_size: (f + 1) * frame_size].tobytes()
        frame = image[c_at: c_at + int(entries[f, 0])]
        assert bool(frame[4] & 4) == bool(flags & 2)
        if has_ck:                                                       # 5. the table's checksums
            assert int(entries[f, 2]) == oracle.xxh64(piece) & 0xFFFFFFFF
        if f in (0, nframes - 1):
            assert zstd_util.decode(zstd, frame, len(piece)) == (piece, 0)   # (libzstd checks the in-frame word)
        c_at += int(entries[f, 0])
    # 1. the reference reader reads the downloaded file back whole
    for cache in (0, 1):
        r = ref.open(image, cache)
        assert r.h, r.error
        got = bytearray()
        while len(got) < length:
            k, b = r.pread(length - len(got), len(got))
            assert k > 0, r.error
            got += b
        r.close()
        assert bytes(got) == host.tobytes()
    # 2.-4. opened where it was built, verification on, nothing uploaded
    d_image = t[GUARD + at: GUARD + at + n]
    with zs.Reader.open_device(d_image.data_ptr(), n, 0) as r:
        assert r.type == zs.ZSEEK_ZSTD
        r.set_verify_checksums(True)
        out = torch.full((length + 32,), SENT, dtype=torch.uint8, device=gpu)
        assert r.pread_device(out.data_ptr(), length + 32, 0) == length
        assert torch.equal(out[:length], dev) and bool((out[length:] == SENT).all())
        assert r.gpu_stats()["bytes_uploaded"] == 0


def test_build_image_python_and_edges(gpu, zs, oracle):
    import torch
    host, dev = _source(oracle, gpu)
    # len 0: the empty table alone
    n, err, t, cap, at = _build(zs, gpu, dev, 0, 65536, 1)
    assert n == 17 == cap, err
    assert t.cpu().numpy()[GUARD + at:][:17].tobytes() == struct.pack("<IIIBI", 0x184D2A5E, 9, 0, 0x80, 0x8F92EAB1)
    # one byte short: refused before anything is written
    bound = zs.zstd_image_bound(500_000, 65536, True)
    n, err, t, cap, at = _build(zs, gpu, dev, 500_000, 65536, 1, capacity=bound - 1)
    assert n == -1 and err == "build image: buffer too small" and bool((t == SENT).all())
    for fs in (0, (4 << 20) + 1):
        n, err, t, cap, at = _build(zs, gpu, dev, 500_000, fs, 0, capacity=600_000)
        assert n == -1 and err == "build image: invalid frame size" and bool((t == SENT).all())
    buf = np.zeros(600_000, np.uint8)
    e = C.create_string_buffer(80)
    assert zs.lib().zsk_zstd_build_image(dev.data_ptr(), 500_000, 65536, 0, 0, buf.ctypes.data, buf.size, e) == -1
    assert e.value == b"build image: not device memory of one device"
    # the wrapper; small batches chain to the same bytes
    image = zs.zstd_build_image(dev[:500_000], 65536, checksums=True, content_checksums=True)
    again = zs.zstd_build_image(dev[:500_000], 65536, checksums=True, content_checksums=True, batch_bytes=3 * 65536)
    assert image.is_cuda and torch.equal(image, again)
    with zs.Reader(image.cpu().numpy(), 0) as r:
        assert r.type == zs.ZSEEK_ZSTD and r.pread(500_000, 0) == host[:500_000].tobytes()


# -- the reason to choose zstd --------------------------------------------------
def test_ratio_beats_lz4(gpu, zs, oracle, zstd):
    """64 frames of 64 KiB of synth(4 MiB, seed 1): smaller than liblz4's frames for the same data."""
    data = oracle.synth(4 * MIB, 1)
    rows = {}
    for fs in (65536, 4096):
        nf = data.size // fs
        desc, cs, _ = _compress(zs, gpu, data, [fs] * nf, guard=0)
        c_off, _ = zs.seek_table_of(zs.lz4_seekable(data, fs))
        lib = {lv: sum(len(zstd_util.compress(zstd, data[i * fs: (i + 1) * fs].tobytes(), {zstd_util.P_LEVEL: lv}))
                       for i in range(nf)) for lv in (1, -1)}
        rows[fs] = (int(cs.sum()), int(c_off[-1]), lib[1], lib[-1])
        print("frame %6d: GPU zstd %d (%.4f)  liblz4 %d (%.4f)  libzstd 1: %d (%.4f)  libzstd -1: %d (%.4f)"
              % ((fs,) + tuple(x for v in rows[fs] for x in (v, v / data.size))))
    gpu_bytes, lz4_bytes = rows[65536][:2]
    assert gpu_bytes < lz4_bytes
