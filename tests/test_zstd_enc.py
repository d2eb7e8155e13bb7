"""The format layer of the GPU zstd compressor on the CPU:
libzseek_amd/csrc/zstd_enc_dev.h driven serially through
tests/native/zstd_enc_shim.cpp.  Every frame is decoded by libzstd 1.4.9
(zstd_util) and by oracle.zstd_decode to the exact input; a small parser here
reads back which header forms the encoder chose, so each size-form boundary is
known to have been crossed.

Two of the listed edges cannot exist in a frame and are checked where they can:
  * match length 131074 (the largest the ML codes express) exceeds every block
    (kZBlock <= 128 KiB = 131072): the code mapping is checked up to 131074,
    and a frame carries the largest match a block holds (131070 bytes behind
    two literals; one literal would make the block a one-byte run);
  * a 3-byte match cannot start later than frame size - 3, so "offset frame
    size - 1" is taken as the farthest reach there is: offset n - 3, whose
    source is the frame's first byte.
"""
from __future__ import annotations

import ctypes as C
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest

import zstd_util

ROOT = pathlib.Path(__file__).resolve().parents[1]
NEW = ["zsk_zstd_compress_scratch_size", "zsk_zstd_compress_frames", "zsk_zstd_image_bound", "zsk_zstd_build_image"]


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    so = tmp_path_factory.mktemp("zstd_enc") / "libzstd_enc.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/zstd_enc_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.zenc_zblock.restype = C.c_uint32
    L.zenc_frame_bound.restype = C.c_uint64
    L.zenc_frame_bound.argtypes = [C.c_uint64]
    L.zenc_huf_lengths.restype = C.c_uint32
    L.zenc_huf_lengths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.zenc_frame.restype = C.c_int64
    L.zenc_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
    L.zenc_compress.restype = C.c_int64
    L.zenc_compress.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64]
    for fn in (L.zenc_ll_code, L.zenc_ml_code):
        fn.restype = None
        fn.argtypes = [C.c_uint32, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def zstd():
    z = zstd_util.load()
    if z is None:
        pytest.skip("libzstd 1.4.9 not present")
    return z


@pytest.fixture(scope="module")
def judge(zstd, oracle):
    """frame, content -> both decoders give the content back."""
    def check(frame: bytes, content: bytes):
        got, err = zstd_util.decode(zstd, frame, len(content))
        assert err == 0 and got == content, ("libzstd", err, len(content))
        got, err = oracle.zstd_decode(frame, len(content))
        assert err == 0 and got == content, ("oracle", err, len(content))
    return check


class Content:
    """Frame content built from literals and matches; the sequences per block."""

    def __init__(self, zblock):
        self.zb, self.data, self.seqs = zblock, bytearray(), []

    def lit(self, b: bytes):
        self.data += b
        self._ll = getattr(self, "_ll", 0) + len(b)
        return self

    def cut(self):
        """A block ends here: the literals so far are its trailing ones."""
        assert len(self.data) % self.zb == 0
        self._ll = 0
        return self

    def match(self, ml: int, off: int):
        at = len(self.data)
        assert 1 <= off <= at and ml >= 3
        if off >= ml:
            self.data += self.data[at - off: at - off + ml]
        else:
            pat = bytes(self.data[at - off: at])
            self.data += (pat * (ml // off + 1))[:ml]
        self.seqs.append((at, getattr(self, "_ll", 0), ml, off))
        self._ll = 0
        return self

    def frame(self, enc, checksum=False):
        n = len(self.data)
        nb = max(1, -(-n // self.zb))
        per = [[] for _ in range(nb)]
        for at, ll, ml, off in self.seqs:
            b = (at - ll) // self.zb if ll else at // self.zb
            assert (at - ll) // self.zb == (at + ml - 1) // self.zb, "a sequence stays in its block"
            per[b].append((ll, ml, off))
        seq3 = np.ascontiguousarray([t for blk in per for t in blk], np.uint32).reshape(-1, 3)
        nseq = np.ascontiguousarray([len(blk) for blk in per], np.uint32)
        src = np.frombuffer(bytes(self.data), np.uint8) if n else np.zeros(1, np.uint8)
        cap = enc.zenc_frame_bound(n)
        out = np.empty(cap, np.uint8)
        r = enc.zenc_frame(src.ctypes.data, n, seq3.ctypes.data if len(seq3) else None, nseq.ctypes.data,
                           1 if checksum else 0, out.ctypes.data, cap)
        assert r > 0, r
        return out[:r].tobytes(), bytes(self.data)


def parse(frame: bytes):
    """-> (header bytes, [(type, block size, body)]) of one frame."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    assert fhd & 0x20 and not fhd & 3, "single segment, no dictionary id"
    at = 5 + {0: 1, 1: 2, 2: 4, 3: 8}[fhd >> 6]
    hdr, blocks = at, []
    while True:
        h = int.from_bytes(frame[at:at + 3], "little")
        typ, size = (h >> 1) & 3, h >> 3
        take = 1 if typ == 1 else size
        blocks.append((typ, size, frame[at + 3: at + 3 + take]))
        at += 3 + take
        if h & 1:
            break
    assert at + (4 if fhd & 4 else 0) == len(frame)
    return hdr, blocks


def lit_info(body: bytes):
    """-> (type, header bytes, regenerated size, compressed size, streams) of a block's literals."""
    typ, sf = body[0] & 3, (body[0] >> 2) & 3
    if typ < 2:
        hl = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        n = int.from_bytes(body[:hl], "little") >> (3 if hl == 1 else 4)
        return typ, hl, n, (n if typ == 0 else 1), 0
    hl, bits = {0: (3, 10), 1: (3, 10), 2: (4, 14), 3: (5, 18)}[sf]
    v = int.from_bytes(body[:hl], "little") >> 4
    return typ, hl, v & ((1 << bits) - 1), v >> bits, 1 if sf == 0 else 4


def seq_count(body: bytes):
    """-> (nbSeq, header bytes) of the block's sequences section."""
    _, hl, _, comp, _ = lit_info(body)
    s = body[hl + comp:]
    if s[0] < 128:
        return s[0], 1
    if s[0] < 255:
        return ((s[0] - 128) << 8) + s[1], 2
    return s[1] + (s[2] << 8) + 0x7F00, 3


RNG = np.random.default_rng(20240611)


def sym64(n: int) -> bytes:
    """n bytes of 64 equally likely symbols 32..95 (6-bit Huffman codes)."""
    return (RNG.integers(0, 64, n, dtype=np.uint8) + 32).tobytes()


def high(n: int) -> bytes:
    """n random bytes, all above 128: never Huffman-coded here."""
    return RNG.integers(129, 256, n, dtype=np.uint8).tobytes()


# -- the public entries ------------------------------------------------------
def test_zstd_entries_declared_listed_exported(zs):
    text = open(os.path.join(ROOT, "include", "zseek_hip.h")).read()
    mapped = open(os.path.join(ROOT, "libzseek_amd", "csrc", "libzseek.map")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", zs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"ZSEEK_EXPORT\s+\w+\s+%s\s*\(" % name, text), name
        assert re.search(r"^\s*%s;" % name, mapped, re.M), name
        assert name in zs.EXPORTED and hasattr(zs.lib(), name)
        assert any(ln.split()[-1] == name and ln.split()[-2] == "T" for ln in out.splitlines()), name
    for macro in ("ZSK_ZSTD_COMPRESS_MAX_FRAME", "ZSK_COMPRESS_CONTENT_CHECKSUM", "ZSK_ZSTD_COMPRESS_BOUND",
                  "ZSK_IMAGE_CONTENT_CHECKSUMS"):
        assert re.search(r"#define\s+%s\b" % macro, text), macro


def test_bound_and_layout_agree(zs, enc):
    zb = enc.zenc_zblock()
    assert zb == zs.ZSTD_BLOCK and zb <= 128 << 10
    for n in (0, 1, 255, zb - 1, zb, zb + 1, 2 * zb + 999, 1 << 22):
        want = (9 + 3 * max(1, -(-n // zb)) + n + 4 + 15) & ~15
        assert enc.zenc_frame_bound(n) == want == zs.zstd_compress_bound(n)
    d, total = zs.zstd_compress_layout([0, 5, zb + 1])
    assert d["dst_off"].tolist() == [0, 16, 16 + 32] and total == 48 + zs.zstd_compress_bound(zb + 1)
    assert zs.zstd_image_bound(0, 65536) == 17 and zs.zstd_image_bound(100, 0) == 0
    assert zs.zstd_image_bound(3 * 65536 + 5, 65536, True) == \
        3 * zs.zstd_compress_bound(65536) + zs.zstd_compress_bound(5) + 17 + 12 * 4
    assert zs.zstd_compress_scratch_size(0) == 0 and zs.zstd_compress_scratch_size(3, 100) > 0


def test_build_image_refusals_without_a_device(zs):
    """The argument checks of zsk_zstd_build_image that need no GPU: zsk_lz4_build_image's texts."""
    L = zs.lib()
    err = C.create_string_buffer(zs.ERRBUF)
    buf = np.zeros(1 << 12, np.uint8)
    for fs in (0, (4 << 20) + 1):
        assert L.zsk_zstd_build_image(buf.ctypes.data, 100, fs, 0, 0, buf.ctypes.data, buf.size, err) == -1
        assert err.value == b"build image: invalid frame size"
    assert L.zsk_zstd_build_image(buf.ctypes.data, 100, 65536, 0, 0, buf.ctypes.data, buf.size, err) == -1
    assert err.value in (b"no HIP device available", b"build image: not device memory of one device")


# -- frame and block forms ----------------------------------------------------
@pytest.mark.parametrize("n,hdr", [(0, 6), (1, 6), (255, 6), (256, 7), (65791, 7), (65792, 9)])
def test_content_size_forms(enc, judge, n, hdr):
    for checksum in (False, True):
        frame, content = Content(enc.zenc_zblock()).lit(high(n)).frame(enc, checksum)
        got_hdr, blocks = parse(frame)
        assert got_hdr == hdr and bool(frame[4] & 4) == checksum
        assert [b[0] for b in blocks] == [1 if n == 1 else 0], "random bytes: a Raw block (one byte: a run)"
        assert len(frame) == hdr + 3 + n + (4 if checksum else 0)
        judge(frame, content)
    if n == 0:
        assert len(frame) - 4 == 9


def test_checksum_is_verified(enc, zstd):
    frame, content = Content(enc.zenc_zblock()).lit(sym64(5000)).frame(enc, True)
    assert zstd_util.decode(zstd, frame, len(content)) == (content, 0)
    bad = bytearray(frame)
    bad[-1] ^= 1
    assert zstd_util.decode(zstd, bytes(bad), len(content)) == (b"", 22)   # ZSTD_error_checksum_wrong


def test_block_types(enc, judge):
    zb = enc.zenc_zblock()
    for content, types in ((high(1000), [0]), (b"\x07" * 1000, [1]), (b"\xEE" * (zb + 10), [1, 1]),
                           (sym64(3000), [2]), (b"ab" * 20, [0])):   # (a 50-byte tree description does not pay for 40 bytes)
        frame, content = Content(zb).lit(content).frame(enc)
        _, blocks = parse(frame)
        assert [b[0] for b in blocks] == types
        for typ, size, body in blocks:
            assert typ != 2 or size < min(zb, len(content)), "Compressed only when smaller"
        judge(frame, content)


@pytest.mark.parametrize("n,hl", [(31, 1), (32, 2), (4095, 2), (4096, 3)])
def test_raw_and_rle_literal_size_forms(enc, judge, n, hl):
    zb = enc.zenc_zblock()
    # Raw literals (bytes above 128) in a Compressed block: a long match pays for the block
    frame, content = Content(zb).lit(high(n)).match(400, n).frame(enc)
    _, blocks = parse(frame)
    assert blocks[0][0] == 2 and lit_info(blocks[0][2])[:3] == (0, hl, n) and seq_count(blocks[0][2])[0] == 1
    judge(frame, content)
    # RLE literals: the block's only literals are one byte, its matches reach into the block before it
    c = Content(zb).lit(high(zb)).cut().lit(b"Q" * n).match(500, zb + n - 7)
    frame, content = c.frame(enc)
    _, blocks = parse(frame)
    assert blocks[0][0] == 0 and blocks[1][0] == 2 and lit_info(blocks[1][2])[:3] == (1, hl, n)
    judge(frame, content)


def test_huffman_literal_size_forms(enc, judge):
    """Compressed-literal headers: 10-, 14- and 18-bit fields on both sides of 1024 and 16384, for the
    regenerated and for the compressed size."""
    zb = enc.zenc_zblock()
    seen = {}
    pool = sym64(22100)
    for n in [1023, 1024, 16383, 16384] + list(range(1270, 1310)) + list(range(21730, 21810)):
        frame, content = Content(zb).lit(pool[:n]).frame(enc)
        _, blocks = parse(frame)
        typ, hl, regen, comp, streams = lit_info(blocks[0][2])
        assert blocks[0][0] == 2 and typ == 2 and regen == n and streams == 4
        assert hl == (3 if n < 1024 and comp < 1024 else 4 if n < 16384 and comp < 16384 else 5)
        assert seq_count(blocks[0][2]) == (0, 1)
        seen[(n, comp)] = hl
        judge(frame, content)
    for lo, hi, edge in ((1270, 1310, 1024), (21730, 21810, 16384)):
        comps = [c for n, c in seen if lo <= n < hi]
        assert min(comps) < edge <= max(comps), "the compressed size crosses %d within the scan" % edge
        assert edge - 1 in comps or edge in comps
    assert seen[(1023, next(c for n, c in seen if n == 1023))] == 3 and \
        seen[(1024, next(c for n, c in seen if n == 1024))] == 4
    assert seen[(16383, next(c for n, c in seen if n == 16383))] == 4 and \
        seen[(16384, next(c for n, c in seen if n == 16384))] == 5


@pytest.mark.parametrize("n,streams", [(255, 1), (256, 4)])
def test_one_and_four_streams(enc, judge, n, streams):
    frame, content = Content(enc.zenc_zblock()).lit((b"aaab" * 64)[:n]).frame(enc)
    _, blocks = parse(frame)
    assert blocks[0][0] == 2 and lit_info(blocks[0][2])[0] == 2 and lit_info(blocks[0][2])[4] == streams
    judge(frame, content)


@pytest.mark.parametrize("nseq,hl", [(0, 1), (1, 2), (127, 2), (128, 3), (0x7EFF, 3), (0x7F00, 4)])
def test_sequence_count_forms(enc, judge, nseq, hl):
    """nbSeq in its 1 / 2 / 3-byte form (+ the modes byte when there are sequences): ll 1, ml 3 each."""
    c = Content(enc.zenc_zblock()).lit(sym64(400))   # (Huffman on these pays for a block of few sequences)
    lits = sym64(max(nseq, 1))
    for i in range(nseq):
        c.lit(lits[i:i + 1]).match(3, 1 + i % 37)
    frame, content = c.frame(enc)
    _, blocks = parse(frame)
    assert len(blocks) == 1 and blocks[0][0] == 2
    n, count_bytes = seq_count(blocks[0][2])
    assert n == nseq and count_bytes + (1 if nseq else 0) == hl
    judge(frame, content)


def test_length_and_offset_edges(enc, judge):
    zb = enc.zenc_zblock()
    # ml 3 and the largest match a block holds; offsets 1 and 2
    frame, content = Content(zb).lit(b"ab").match(zb - 2, 2).frame(enc)
    judge(frame, content)
    frame, content = Content(zb).lit(sym64(600)).match(3, 1).lit(b"x").match(3, 9).frame(enc)
    assert parse(frame)[1][0][0] == 2 and seq_count(parse(frame)[1][0][2])[0] == 2
    judge(frame, content)
    # ll 0 behind a match, and a literal run above 65536 (LL code 35)
    if zb > 70000 + 200:
        c = Content(zb).lit(sym64(70000)).match(100, 70000).match(50, 1).match(3, 69000)
        frame, content = c.frame(enc)
        assert parse(frame)[1][0][0] == 2 and seq_count(parse(frame)[1][0][2])[0] == 3
        judge(frame, content)
    # the farthest reach: from the frame's last 3 bytes to its first, two blocks back
    n = 2 * zb + 999
    c = Content(zb).lit(sym64(zb)).cut().lit(high(zb)).cut().lit(sym64(996)).match(3, n - 3)
    frame, content = c.frame(enc)
    assert len(content) == n and content[-3:] == content[:3]
    judge(frame, content)
    with pytest.raises(AssertionError):   # one byte farther is before the frame: the shim refuses it
        bad = Content(zb).lit(sym64(100))
        bad.seqs.append((100, 100, 3, 101))
        bad.data += b"abc"
        bad.frame(enc)


def test_length_codes_cover_their_range(enc):
    """ll / ml -> (code, base, extra bits) against RFC 8878's tables, up to the largest lengths the codes hold."""
    ll_base = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192,
                                 16384, 32768, 65536]
    ll_bits = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
    ml_base = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099,
                                    8195, 16387, 32771, 65539]
    ml_bits = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
    out = (C.c_uint32 * 3)()
    for fn, base, bits, lo, hi in ((enc.zenc_ll_code, ll_base, ll_bits, 0, 131071),
                                   (enc.zenc_ml_code, ml_base, ml_bits, 3, 131074)):
        values = set(range(lo, 300)) | {hi}
        for b, k in zip(base, bits):
            values |= {b, b + (1 << k) - 1}
        for v in sorted(values):
            fn(v, out)
            code = max(c for c in range(len(base)) if base[c] <= v)
            assert (out[0], out[1], out[2]) == (code, base[code], bits[code]), v
            assert v - out[1] < (1 << out[2]) or out[2] == 0 and v == out[1], v


# -- code lengths --------------------------------------------------------------
def _lengths(enc, count):
    cnt = np.zeros(129, np.uint32)
    cnt[: len(count)] = count
    ln, code = np.zeros(129, np.uint8), np.zeros(129, np.uint16)
    mb = enc.zenc_huf_lengths(cnt.ctypes.data, ln.ctypes.data, code.ctypes.data)
    return mb, ln, code


def _check_code(mb, ln, code, count):
    used = [s for s in range(129) if s < len(count) and count[s]]
    assert all(1 <= ln[s] <= 11 for s in used) and all(ln[s] == 0 for s in range(129) if s not in used)
    assert mb == max(ln[s] for s in used) <= 11
    assert sum(2 ** (11 - int(ln[s])) for s in used) == 2 ** 11, "Kraft sum exactly 1"
    words = sorted(format(int(code[s]), "0%db" % ln[s]) for s in used)
    assert all(not b.startswith(a) for a, b in zip(words, words[1:])), "prefix-free"


def _shuffled(count) -> bytes:
    data = np.repeat(np.arange(len(count), dtype=np.uint8), count)
    RNG.shuffle(data)
    return data.tobytes()


def test_code_lengths_fibonacci(enc, judge):
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])            # an unlimited tree would be 23 deep
    count = [0] * 40 + fib
    mb, ln, code = _lengths(enc, count)
    _check_code(mb, ln, code, count)
    assert mb == 11
    frame, content = Content(enc.zenc_zblock()).lit(_shuffled(count)).frame(enc)
    blocks = parse(frame)[1]
    assert blocks[0][0] == 2 and lit_info(blocks[0][2])[0] == 2
    judge(frame, content)


def test_code_lengths_two_symbols(enc, judge):
    count = [0] * 128 + [1]
    count[3] = 999
    mb, ln, code = _lengths(enc, count)
    _check_code(mb, ln, code, count)
    assert mb == 1 and ln[3] == ln[128] == 1
    frame, content = Content(enc.zenc_zblock()).lit(_shuffled(count)).frame(enc)
    assert lit_info(parse(frame)[1][0][2])[0] == 2          # byte 128 is the last the weights describe
    judge(frame, content)
    assert _lengths(enc, [0, 5])[0] == 0                      # one symbol: no code


def test_code_lengths_one_rare_symbol(enc, judge):
    zb = enc.zenc_zblock()
    count = [0] * 129
    for s in range(32, 95):
        count[s] = (zb - 1) // 63
    count[32] += (zb - 1) - sum(count)
    count[100] = 1                                            # once among 128 Ki others
    mb, ln, code = _lengths(enc, count)
    _check_code(mb, ln, code, count)
    assert sum(count) == zb
    frame, content = Content(zb).lit(_shuffled(count)).frame(enc)
    assert lit_info(parse(frame)[1][0][2])[0] == 2
    judge(frame, content)


def test_byte_above_128_is_raw(enc, judge):
    vals = list(range(128)) + [200]                           # 129 distinct values
    lits = bytes(vals) * 3
    frame, content = Content(enc.zenc_zblock()).lit(lits).match(600, len(lits)).frame(enc)
    blocks = parse(frame)[1]
    assert blocks[0][0] == 2 and lit_info(blocks[0][2])[0] == 0, "literals with a byte above 128 are stored Raw"
    judge(frame, content)
    lits = bytes(range(129)) * 40                             # 129 values the weights do describe
    frame, content = Content(enc.zenc_zblock()).lit(lits).frame(enc)
    assert lit_info(parse(frame)[1][0][2])[0] == 2
    judge(frame, content)


# -- the whole pipeline behind the match search's restatement -------------------
def test_pipeline_round_trip(enc, judge, oracle):
    zb = enc.zenc_zblock()
    synth = oracle.synth(3 * zb, 5).tobytes()
    cases = [b"", b"a", b"abcd" * 3, synth[:70000], synth[: 2 * zb + 999], bytes(2 * zb + 5),
             (high(270) * 600)[: zb + 77], (sym64(70000) * 3)[: 2 * zb + 1],
             (RNG.integers(0, 3, zb + 3, dtype=np.uint8) + 65).tobytes(),
             np.repeat(RNG.integers(128, 256, 9000, dtype=np.uint8), 7).tobytes()]
    for i, content in enumerate(cases):
        src = np.frombuffer(content, np.uint8) if content else np.zeros(1, np.uint8)
        cap = enc.zenc_frame_bound(len(content))
        out = np.empty(cap, np.uint8)
        n = enc.zenc_compress(src.ctypes.data, len(content), i & 1, out.ctypes.data, cap)
        assert 0 < n <= cap
        judge(out[:n].tobytes(), content)
    # the corpus compresses: 64 KiB of synth well below LZ4's half
    src = np.frombuffer(synth[zb: zb + 65536], np.uint8)
    out = np.empty(enc.zenc_frame_bound(65536), np.uint8)
    assert enc.zenc_compress(src.ctypes.data, 65536, 0, out.ctypes.data, out.size) < 65536 * 0.45
