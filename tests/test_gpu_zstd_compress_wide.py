"""ZSK_ZSTD_FORMAT_FULL_WIDE and ZSK_IMAGE_ZSTD_WIDE (csrc/zstd_compress.hip's
third instantiation, csrc/zstd_enc_wide_dev.h) on the GPU.

The kernel's bytes must be the CPU shim's (tests/native/zstd_enc_wide_shim.cpp
restates the search serially and drives the same format layer), frame by
frame: on the edge batch, across the frames of persistent workgroups -- where a
table that is not cleared, or not cleared whole, shows -- and on the largest
frame.  Every frame of the edge batch is also decoded by libzstd 1.4.9, and the
files of zsk_zstd_build_image by the reference reader, the oracle and the
project's own GPU decoder, to which offsets into earlier blocks are new input
from the project's own writer.  The two other formats must not have moved.

The helpers are test_gpu_zstd_compress.py's; every test asks for the `gpu`
fixture first, as there."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import zstd_util
import zstd_wide_util as wu
from test_gpu_zstd_compress import CK, GUARD, MIB, SENT, _build, _frames, _judge, _table

pytestmark = pytest.mark.gpu
ZB = wu.ZB
WIDE, FULL_IMAGE, WIDE_IMAGE = 5, 4, 8   # ZSK_ZSTD_FORMAT_FULL_WIDE, ZSK_IMAGE_ZSTD_FULL, ZSK_IMAGE_ZSTD_WIDE


@pytest.fixture(scope="module")
def zstd():
    z = zstd_util.load()
    if z is None:
        pytest.skip("libzstd 1.4.9 not present")
    return z


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = wu.load_shim(tmp_path_factory.mktemp("zstd_enc_wide_gpu"))
    return lambda content, checksum=False, how="wide": wu.compress(L, content, checksum, how)


def _compress(zs, gpu, src: np.ndarray, sizes, offsets=None, flags=None, guard=GUARD, runs=1, fmt=WIDE):
    """test_gpu_zstd_compress.py's _compress through zsk_zstd_compress_frames_ex with `fmt`."""
    import torch
    desc, _ = zs.zstd_compress_layout(sizes, offsets, flags)
    slots = np.array([zs.zstd_compress_bound(int(n)) for n in desc["src_size"]], np.uint64)
    desc["dst_off"] = np.concatenate(([0], np.cumsum(slots + np.uint64(guard))[:-1])) if len(slots) else slots
    total = int((slots + np.uint64(guard)).sum())
    d_src = torch.from_numpy(np.ascontiguousarray(src)).to(gpu)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    need = zs.lib().zsk_zstd_compress_scratch_size_ex(len(desc), src.size, fmt)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=gpu)
    outs, cs = [], None
    for _ in range(runs):
        d_dst = torch.full((max(total, 1),), SENT, dtype=torch.uint8, device=gpu)
        csize = torch.full((len(desc),), -1, dtype=torch.int32, device=gpu)
        r = zs.lib().zsk_zstd_compress_frames_ex(d_desc.data_ptr(), len(desc), d_src.data_ptr(), d_dst.data_ptr(),
                                                 csize.data_ptr(), scratch.data_ptr(), need,
                                                 torch.cuda.current_stream().cuda_stream, fmt)
        assert r == 0, ("zsk_zstd_compress_frames_ex", fmt, r)
        torch.cuda.synchronize()
        outs.append(d_dst.cpu().numpy())
        c = csize.cpu().numpy()
        assert cs is None or np.array_equal(cs, c)
        cs = c
    return desc, cs, outs


def _packed(parts):
    """parts back to back behind 3 bytes, so that frames start at odd addresses too;
    the checksum flag on every other frame."""
    sizes = [p.size for p in parts]
    src = np.concatenate([np.full(3, 0x11, np.uint8)] + parts)
    offsets = 3 + np.concatenate(([0], np.cumsum(sizes)[:-1]))
    return src, sizes, offsets, [(f & 1) * CK for f in range(len(sizes))]


# -- bytes equal the shim's ------------------------------------------------------------------------
def test_wide_edge_batch(gpu, zs, zstd, oracle, shim):
    text = oracle.synth(2 * MIB, 7)
    cross = wu.cross_block_inputs()
    parts = [text[11: 11 + n].copy() for n in (0, 1, 100, wu.WIDE_MIN, wu.WIDE_MIN + 1, ZB, ZB + 1, 2 * ZB + 5)]
    parts += [oracle.synth(MIB, 1), cross["a"], cross["b"], cross["c"], text[5: 5 + 33333] ^ np.uint8(0x80)]
    src, sizes, offsets, flags = _packed(parts)
    desc, cs, outs = _compress(zs, gpu, src, sizes, offsets, flags, runs=2)
    assert np.array_equal(outs[0], outs[1]), "two runs are byte-identical"
    frames = _frames(zs, desc, cs, outs[0])                              # (inside the slot, guards intact)
    for f, (frame, part) in enumerate(zip(frames, parts)):
        assert bool(frame[4] & 4) == bool(f & 1), "the content-checksum bit only where asked for"
        _judge(zstd, oracle, frame, part.tobytes(), (f, part.size))
        assert frame == shim(part, bool(f & 1)), (f, part.size, "GPU bytes != CPU shim bytes")
    assert len(frames[9]) < 0.55 * parts[9].size, "block 1 found in block 0"
    assert len(frames[11]) < parts[11].size // 8, "block 31 found in block 0, 31 blocks back"


def test_persistent_workgroups_clear_the_table(gpu, zs, oracle, shim):
    """More frames than resident workgroups, longer and shorter ones in turn, all above 16 KiB: a
    workgroup's second frame is shorter than its first, whose table it must not see."""
    nframes = 1792 + 9
    text = oracle.synth(8 * MIB, 3)
    sizes = [40000 if (f % 2 == 0) == (f < 1792) else 16400 for f in range(nframes)]   # (1,792 workgroups walk the batch)
    assert sizes[0] > sizes[1792] > wu.WIDE_MIN and sizes[1] < sizes[1793]
    rng = np.random.default_rng(5)
    offsets = rng.integers(0, text.size - 40000, nframes)
    offsets[1792:] = offsets[:9]                                         # (the same start, another length)
    desc, cs, outs = _compress(zs, gpu, text, sizes, offsets, guard=16)
    frames = _frames(zs, desc, cs, outs[0], guard=16)
    want = {}
    for f, frame in enumerate(frames):
        key = (int(offsets[f]), sizes[f])
        if key not in want:
            want[key] = shim(text[key[0]: key[0] + key[1]])
        assert frame == want[key], (f, key, "GPU bytes != CPU shim bytes")


def test_largest_frame_and_refusal(gpu, zs, zstd, oracle, shim):
    cap = zs.ZSTD_COMPRESS_MAX_FRAME
    data = oracle.synth(cap + 1, 2)
    desc, cs, outs = _compress(zs, gpu, data, [cap, cap + 1], offsets=[0, 0], flags=[CK, 0])
    host = outs[0]
    assert cs[1] == 0
    at = int(desc["dst_off"][1])
    assert (host[at: at + zs.zstd_compress_bound(cap + 1) + GUARD] == SENT).all(), "a refused slot is untouched"
    frame = _frames(zs, desc[:1], cs[:1], host)[0]
    assert frame == shim(data[:cap], True), "GPU bytes != CPU shim bytes"
    _judge(zstd, oracle, frame, data[:cap].tobytes(), "4 MiB")


def test_other_formats_unmoved(gpu, zs, oracle, shim):
    text = oracle.synth(MIB, 8)
    parts = [text[7: 7 + n].copy() for n in (0, 100, 5000, wu.WIDE_MIN + 1, 65536, ZB + 1)]
    parts.append(text[:40000] ^ np.uint8(0x80))
    src, sizes, offsets, flags = _packed(parts)
    got = {}
    for how, fmt in (("subset", 0), ("full", 1), ("wide", WIDE)):
        desc, cs, outs = _compress(zs, gpu, src, sizes, offsets, flags, fmt=fmt)
        got[how] = _frames(zs, desc, cs, outs[0])
        for f, (frame, part) in enumerate(zip(got[how], parts)):
            assert frame == shim(part, bool(f & 1), how), (how, f, part.size)
    assert got["wide"][:3] == got["full"][:3] and got["wide"][3:] != got["full"][3:]


# -- refusals ------------------------------------------------------------------------------------
def test_wide_refusals(gpu, zs):
    import torch
    L = zs.lib()
    t = torch.full((4096,), SENT, dtype=torch.uint8, device=gpu)
    desc, _ = zs.zstd_compress_layout([100])
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    csize = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    need = L.zsk_zstd_compress_scratch_size_ex(1, 100, WIDE)
    assert need == L.zsk_zstd_compress_scratch_size_ex(1, 100, 1) + (64 << 10) == zs.zstd_compress_scratch_size(1, 100, wide=True)
    scratch = torch.empty(need, dtype=torch.uint8, device=gpu)
    args = (d_desc.data_ptr(), 1, t.data_ptr(), t.data_ptr() + 2048, csize.data_ptr(), scratch.data_ptr())
    for fmt in (3, 4):                                                   # bit 2 alone, or over the subset: unknown
        assert L.zsk_zstd_compress_scratch_size_ex(1, 100, fmt) == 0
        assert L.zsk_zstd_compress_frames_ex(*args, need, None, fmt) == -1
    assert L.zsk_zstd_compress_frames_ex(*args, need - 1, None, WIDE) == -1, "a scratch one byte short"
    assert L.zsk_zstd_compress_frames_ex(*args, L.zsk_zstd_compress_scratch_size_ex(1, 100, 1), None, WIDE) == -1
    roomy = torch.empty(need + 32, dtype=torch.uint8, device=gpu)       # the tables want a 16-byte aligned scratch
    assert roomy.data_ptr() % 16 == 0
    assert L.zsk_zstd_compress_frames_ex(*args[:5], roomy.data_ptr() + 1, need, None, WIDE) == -1
    torch.cuda.synchronize()
    assert int(csize[0]) == -1 and bool((t == SENT).all()), "nothing was queued"
    assert L.zsk_zstd_compress_frames_ex(*args[:5], roomy.data_ptr() + 16, need, None, WIDE) == 0
    torch.cuda.synchronize()
    assert int(csize[0]) > 0
    assert L.zsk_zstd_compress_frames_ex(None, 0, None, None, None, None, 0, None, WIDE) == 0


# -- zsk_zstd_build_image -----------------------------------------------------------------------------
_SRC = {}


def _source(oracle, gpu):
    import torch
    if not _SRC:
        _SRC["host"] = oracle.synth(6 * MIB + 12345, 1)
        _SRC["dev"] = torch.from_numpy(_SRC["host"]).to(gpu)
        torch.cuda.synchronize()
    return _SRC["host"], _SRC["dev"]


@pytest.mark.parametrize("frame_size", [65536, MIB])
@pytest.mark.parametrize("flags", [WIDE_IMAGE, WIDE_IMAGE | FULL_IMAGE | 1, WIDE_IMAGE | 1 | 2])
def test_build_image_wide(gpu, zs, oracle, ref, zstd, shim, frame_size, flags):
    import torch
    host, dev = _source(oracle, gpu)
    length = host.size
    n, err, t, cap, at = _build(zs, gpu, dev, length, frame_size, flags)
    assert 0 < n <= cap, err
    assert cap == zs.lib().zsk_zstd_image_bound(length, frame_size, flags & 3), "the bound is the flagless one"
    whole = t.cpu().numpy()
    assert (whole[: GUARD + at] == SENT).all() and (whole[GUARD + at + cap:] == SENT).all()
    image = whole[GUARD + at: GUARD + at + n].tobytes()
    nframes = -(-length // frame_size)
    entries, has_ck = _table(image)
    assert len(entries) == nframes and has_ck == bool(flags & 1)
    assert int(entries[:, 1].sum()) == length and int(entries[:, 0].sum()) + 17 + entries.size * 4 == n
    n_full, _, _, _, _ = _build(zs, gpu, dev, length, frame_size, (flags & 3) | FULL_IMAGE)
    print("frames of %d: wide file %d, full file %d (%.4f)" % (frame_size, n, n_full, n / n_full))
    assert n < n_full, "the wide search's file is the smaller one"
    c_off = np.concatenate(([0], np.cumsum(entries[:, 0].astype(np.uint64))))
    for f in range(nframes):                                             # the oracle, frame by frame; the shim
        piece = host[f * frame_size: (f + 1) * frame_size]
        frame = image[int(c_off[f]): int(c_off[f + 1])]
        assert bool(frame[4] & 4) == bool(flags & 2)
        if has_ck:
            assert int(entries[f, 2]) == oracle.xxh64(piece.tobytes()) & 0xFFFFFFFF
        _judge(zstd, oracle, frame, piece.tobytes(), f)
        if f in (0, nframes - 1):
            assert frame == shim(piece, bool(flags & 2)), (f, "GPU bytes != CPU shim bytes")
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
    d_image = t[GUARD + at: GUARD + at + n]                              # this project's reader, where it was built
    with zs.Reader.open_device(d_image.data_ptr(), n, 0) as r:
        assert r.type == zs.ZSEEK_ZSTD
        r.set_verify_checksums(True)
        out = torch.full((length + 32,), SENT, dtype=torch.uint8, device=gpu)
        assert r.pread_device(out.data_ptr(), length + 32, 0) == length
        assert torch.equal(out[:length], dev) and bool((out[length:] == SENT).all())
        ranges = [(1, 70001), (frame_size - 3, 7), (2 * MIB + 5, MIB + 131073), (length - 4099, 4099), (ZB - 1, 2)]
        total = sum(c for _, c in ranges)
        out = torch.full((total + 32,), SENT, dtype=torch.uint8, device=gpu)
        rg, n_ok = r.preadv_device(out.data_ptr(), ranges)
        assert n_ok == len(ranges) and rg["result"].tolist() == [c for _, c in ranges]
        want = np.concatenate([host[o: o + c] for o, c in ranges])
        assert out[:total].cpu().numpy().tobytes() == want.tobytes() and bool((out[total:] == SENT).all())
    # one asynchronous decode over all the frames with the default bounds
    fd = np.zeros(nframes, zs.FRAME_DESC_DTYPE)
    fd["c_off"], fd["c_size"] = c_off[:-1], entries[:, 0]
    fd["d_size"] = entries[:, 1]
    fd["d_off"] = np.arange(nframes, dtype=np.uint64) * frame_size
    out = torch.full((length + 32,), SENT, dtype=torch.uint8, device=gpu)
    status = torch.full((nframes,), -1, dtype=torch.int32, device=gpu)
    comp = torch.zeros(n + 256, dtype=torch.uint8, device=gpu)
    comp[:n].copy_(d_image)
    zs.zstd_decode_frames_async(torch.from_numpy(fd.view(np.uint8).copy()).to(gpu), comp, out[:length], status,
                                zs.zstd_bounds_default(nframes, length))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * nframes
    assert torch.equal(out[:length], dev) and bool((out[length:] == SENT).all())
    # the wrapper's keyword, and the LZ4 builder ignores the bit
    image2 = zs.zstd_build_image(dev, frame_size, checksums=bool(flags & 1), content_checksums=bool(flags & 2),
                                 full=bool(flags & FULL_IMAGE), wide=True)
    assert image2.cpu().numpy().tobytes() == image
    if frame_size == 65536 and flags == WIDE_IMAGE:
        bound = zs.lib().zsk_lz4_image_bound(length, frame_size, 0)
        a = torch.zeros(bound, dtype=torch.uint8, device=gpu)
        b = torch.zeros(bound, dtype=torch.uint8, device=gpu)
        e = ctypes.create_string_buffer(80)
        na = zs.lib().zsk_lz4_build_image(dev.data_ptr(), length, frame_size, 0, 0, 0, a.data_ptr(), bound, e)
        nb = zs.lib().zsk_lz4_build_image(dev.data_ptr(), length, frame_size, 0, WIDE_IMAGE, 0, b.data_ptr(), bound, e)
        assert na == nb > 0 and torch.equal(a[:na], b[:nb])
