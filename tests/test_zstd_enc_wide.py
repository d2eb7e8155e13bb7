"""The wide match search of the GPU zstd compressor (ZSK_ZSTD_FORMAT_FULL_WIDE)
on the CPU: libzseek_amd/csrc/zstd_enc_wide_dev.h behind the serial restatement
of tests/native/zstd_enc_wide_shim.cpp, which hands its sequences to the full
format's layer.  As in test_zstd_enc_full.py every frame is decoded by libzstd
1.4.9 and by oracle.zstd_decode to the exact input.  Beyond that: a frame of at
most 16384 bytes is the full format's frame; matches reach earlier blocks of
the frame (a copied block, a source across a block boundary, an offset of 31
blocks), blocks that are not searched leave the table and the offset history
alone; the totals on the synthetic data against the full format's; and the
bytes are pinned from the first commit (tests/golden/zstd_enc_wide.json).

A frame's only empty block is the one of a 0-byte frame, which the full search
takes; what an unsearched block leaves behind is shown on one-byte runs."""
from __future__ import annotations

import hashlib
import importlib.util
import json
import re

import numpy as np
import pytest

import zstd_util
import zstd_wide_util as wu
from test_zstd_enc import parse
from test_zstd_enc_full import rfc_offsets

ROOT = wu.ROOT
ZB, MIB = wu.ZB, 1 << 20


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    L = wu.load_shim(tmp_path_factory.mktemp("zstd_enc_wide"))
    assert (L.zenc_zblock(), L.zenc_wide_min_frame(), L.zenc_wide_hash_log()) == (ZB, wu.WIDE_MIN, 14)
    return L


@pytest.fixture(scope="module")
def zstd():
    z = zstd_util.load()
    if z is None:
        pytest.skip("libzstd 1.4.9 not present")
    return z


@pytest.fixture(scope="module")
def judge(zstd, oracle):
    def check(frame: bytes, content: bytes, what=None):
        got, err = zstd_util.decode(zstd, frame, len(content))
        assert err == 0 and got == content, ("libzstd", err, len(content), what)
        got, err = oracle.zstd_decode(frame, len(content))
        assert err == 0 and got == content, ("oracle", err, len(content), what)
    return check


@pytest.fixture(scope="module")
def edge(enc, oracle):
    """name -> (content, checksum flag, the wide frame): compressed once for the tests below."""
    return {name: (c, ck, wu.compress(enc, c, ck)) for name, c, ck in wu.edge_inputs(oracle)}


@pytest.fixture(scope="module")
def cross(enc):
    """name -> (content, the wide frame, the full frame, per block the wide search's sequences)"""
    return {k: (c, wu.compress(enc, c), wu.compress(enc, c, how="full"), wu.sequences(enc, c))
            for k, c in wu.cross_block_inputs().items()}


# -- decoding ---------------------------------------------------------------------------------
def test_edge_frames_decode(enc, judge, edge):
    assert {len(c) for c, _, _ in edge.values()} == set(wu.EDGE_LENGTHS) and len(edge) == 3 * len(wu.EDGE_LENGTHS)
    for name, (content, ck, frame) in edge.items():
        assert len(frame) <= enc.zenc_frame_bound(len(content)) and bool(frame[4] & 4) == bool(ck), name
        judge(frame, content.tobytes(), name)
        if name.startswith("noise") and len(content) > 64:
            assert 2 not in {b[0] for b in parse(frame)[1]}, "noise is stored Raw (a block of one byte: RLE)"
        elif len(content) >= wu.WIDE_MIN:
            assert len(frame) < len(content), (name, "text compresses, whatever its top bit")


# -- identity to the full format ---------------------------------------------------------------
def test_small_frames_are_the_full_format(enc, oracle, edge):
    for name, (content, ck, frame) in edge.items():
        if len(content) <= wu.WIDE_MIN:
            assert frame == wu.compress(enc, content, ck, how="full"), name
    text = oracle.synth(wu.WIDE_MIN + 1, 9)
    for n in (100, 4096, wu.WIDE_MIN - 1, wu.WIDE_MIN):
        assert wu.compress(enc, text[:n]) == wu.compress(enc, text[:n], how="full"), n
    # one byte more and the search is the wide one: other sequences, so another frame
    assert wu.compress(enc, text) != wu.compress(enc, text, how="full")


# -- matches into earlier blocks -----------------------------------------------------------------
def test_copied_block(judge, cross):
    content, wide, full, per = cross["a"]
    assert len(content) == 2 * ZB
    print("block 1 a copy of block 0: wide %d, full %d of %d" % (len(wide), len(full), len(content)))
    assert len(wide) < 0.55 * len(content) and len(full) >= len(content)
    assert [b[0] for b in parse(wide)[1]] == [0, 2] and [b[0] for b in parse(full)[1]] == [0, 0]
    assert per[0] == [] or sum(ml for _, ml, _ in per[0]) < 100
    assert any(off == ZB and ml > ZB // 2 for _, ml, off in per[1]), "block 1 is one long match at offset 128 KiB"
    judge(wide, content.tobytes())


def test_source_across_a_block_boundary(judge, cross):
    content, wide, _, per = cross["b"]
    at = 2 * ZB                                                            # block 2's sequences, placed
    found = []
    for ll, ml, off in per[2]:
        at += ll
        found.append((at, ml, at - off))
        at += ml
    hit = [(p, ml, s) for p, ml, s in found if s < ZB < s + ml]
    assert len(hit) == 1, found
    p, ml, s = hit[0]
    assert (p, s) == (2 * ZB + 300, wu.STRADDLE_AT) and ml >= wu.STRADDLE_LEN
    assert [b[0] for b in parse(wide)[1]] == [0, 2, 2]
    judge(wide, content.tobytes())


def test_far_offset(judge, cross):
    content, wide, full, per = cross["c"]
    assert len(content) == 32 * ZB == 1 << 22
    types = [b[0] for b in parse(wide)[1]]
    assert types == [0] + [1] * 30 + [2], "the one-byte runs are RLE blocks; block 31 is Compressed"
    assert all(per[b] == [] for b in range(1, 31)), "an RLE block is not searched"
    off = 31 * ZB
    assert any(o == off and ml > ZB // 2 for _, ml, o in per[31]), "block 0's entries survived 30 unsearched blocks"
    assert (off + 3).bit_length() - 1 == 21, "offset code 21"
    print("far offset: wide %d, full %d" % (len(wide), len(full)))
    assert len(full) - len(wide) > 0.9 * ZB, "smaller than the full format's frame by most of a block"
    judge(wide, content.tobytes())


def test_unsearched_blocks_leave_table_and_history(enc, judge, cross):
    content, wide, _, per = cross["d"]
    types = [b[0] for b in parse(wide)[1]]
    assert types == [2, 1, 2, 2], types
    assert per[1] == [], "the RLE block has no sequences"
    half = ZB // 2
    assert [off for _, ml, off in per[0] if ml > half // 2] == [half]
    # block 3 repeats block 0's halves behind the run and block 2: its match reaches over both
    # (into the nearer half, whose positions came last)
    assert any(off == 3 * ZB - half and ml > half // 2 for _, ml, off in per[3])
    # the history moves on over the blocks written Compressed only (RFC 8878 3.1.1.5 restated):
    # block 2's long match lies 64 KiB back as block 0's last one did, which the run has not disturbed
    frame, ofv = wu.offset_values(enc, content, per)
    assert frame == wide
    assert ofv == rfc_offsets(per, {0, 2, 3})
    long2 = [(ll, off, v) for (ll, ml, off), v in zip(per[2], ofv[2]) if ml > half // 2]
    assert len(long2) == 1 and long2[0][0] > 0 and long2[0][1:] == (half, 1), long2
    assert per[0][-1][2] == half, "block 0 ends on that offset"
    judge(wide, content.tobytes())


# -- ratios ----------------------------------------------------------------------------------------
def test_ratio_against_the_full_format(enc, oracle):
    data = oracle.synth(8 * MIB, 1)
    total = {}
    for fs, bound in ((65536, 0.98), (MIB, 0.96)):
        for how in ("full", "wide"):
            total[fs, how] = sum(len(wu.compress(enc, data[at: at + fs], how=how)) for at in range(0, data.size, fs))
        print("synth(8 MiB, 1) at %7d-byte frames: full %d, wide %d (%.4f)" %
              (fs, total[fs, "full"], total[fs, "wide"], total[fs, "wide"] / total[fs, "full"]))
        assert total[fs, "wide"] <= bound * total[fs, "full"], (fs, total)
    assert total[65536, "full"] == 3211834, "the full format's total is DESIGN.md's"


# -- pinned bytes ----------------------------------------------------------------------------------
def test_wide_bytes_pinned(enc, oracle, edge, cross):
    spec = importlib.util.spec_from_file_location("make_zstd_enc_wide", ROOT / "tests/golden/make_zstd_enc_wide.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    want = json.loads((ROOT / "tests/golden/zstd_enc_wide.json").read_text())
    names = [name for name, _, _ in mk.inputs(oracle)]
    assert set(names) == set(want) and len(want) == 3 * len(wu.EDGE_LENGTHS) + 4
    for name in names:
        content, ck, frame = edge[name] if name in edge else (cross[name[6:]][0], 0, cross[name[6:]][1])
        assert hashlib.sha256(content.tobytes()).hexdigest() == want[name]["input_sha256"], (name, "input")
        assert (len(frame), int(ck)) == (want[name]["size"], want[name]["checksum"]), name
        assert hashlib.sha256(frame).hexdigest() == want[name]["sha256"], name


# -- the host entry points on the built library -------------------------------------------------------
def test_wide_entries(zs):
    text = open(ROOT / "include" / "zseek_hip.h").read()
    for macro, value in (("ZSK_ZSTD_FORMAT_FULL_WIDE", "5"), ("ZSK_IMAGE_ZSTD_WIDE", "8u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), text), macro
    import libzseek_amd
    assert (zs.ZSTD_FORMAT_FULL_WIDE, zs.IMAGE_ZSTD_WIDE) == (5, 8)
    assert (libzseek_amd.ZSTD_FORMAT_FULL_WIDE, libzseek_amd.IMAGE_ZSTD_WIDE) == (5, 8)
    assert zs.ZSTD_FORMAT_FULL_WIDE == zs.ZSTD_FORMAT_FULL | 4
    L = zs.lib()
    for nframes in (1, 3, 1792, 5000):
        base = L.zsk_zstd_compress_scratch_size_ex(nframes, 100, 1)
        assert base == L.zsk_zstd_compress_scratch_size_ex(nframes, 100, 0) == L.zsk_zstd_compress_scratch_size(nframes, 100)
        wide = L.zsk_zstd_compress_scratch_size_ex(nframes, 100, 5)
        assert wide == base + min(nframes, 1792) * (4 << 14), "a 64 KiB table per resident workgroup"
        assert zs.zstd_compress_scratch_size(nframes, 100, wide=True) == wide
        assert zs.zstd_compress_scratch_size(nframes, 100, full=True, wide=True) == wide
        assert zs.zstd_compress_scratch_size(nframes, 100, full=True) == base
    assert L.zsk_zstd_compress_scratch_size_ex(0, 0, 5) == 0
    for fmt in (2, 3, 4, 6, 7):
        assert L.zsk_zstd_compress_scratch_size_ex(3, 100, fmt) == 0
        assert L.zsk_zstd_compress_frames_ex(None, 0, None, None, None, None, 0, None, fmt) == -1
    assert L.zsk_zstd_compress_frames_ex(None, 0, None, None, None, None, 0, None, 5) == 0
    assert L.zsk_zstd_image_bound(3 * 65536 + 5, 65536, 8) == L.zsk_zstd_image_bound(3 * 65536 + 5, 65536, 0)
    assert L.zsk_zstd_image_bound(3 * 65536 + 5, 65536, 8 | 1) == L.zsk_zstd_image_bound(3 * 65536 + 5, 65536, 1)
