"""The full format of the GPU zstd compressor on the CPU:
libzseek_amd/csrc/zstd_enc_full_dev.h driven serially through
tests/native/zstd_enc_full_shim.cpp (which holds the subset shim's entries
too).  As in test_zstd_enc.py every frame is decoded by libzstd 1.4.9 and by
oracle.zstd_decode to the exact input, and small parsers read back which forms
the encoder chose: the tree description's, the three table modes, an FSE
description's shares.

The subset must not move: the hashes of tests/golden/zstd_enc_subset.json were
recorded from the subset shim before the full format existed
(tests/golden/make_zstd_enc_subset.py) and are recomputed here.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import json
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest

import zstd_util
from test_zstd_enc import Content, lit_info, parse, seq_count

ROOT = pathlib.Path(__file__).resolve().parents[1]
NEW = ["zsk_zstd_compress_scratch_size_ex", "zsk_zstd_compress_frames_ex"]
RNG = np.random.default_rng(20250303)
PRE, RLE, FSE = 0, 1, 2


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    so = tmp_path_factory.mktemp("zstd_enc_full") / "libzstd_enc_full.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(so),
                    str(ROOT / "tests/native/zstd_enc_full_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.zenc_zblock.restype = C.c_uint32
    L.zenc_full_custom_min.restype = C.c_uint32
    L.zenc_frame_bound.restype = C.c_uint64
    L.zenc_frame_bound.argtypes = [C.c_uint64]
    for fn in (L.zenc_huf_lengths, L.zenc_full_huf_lengths):
        fn.restype = C.c_uint32
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.zenc_frame.restype = C.c_int64
    L.zenc_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
    L.zenc_full_frame.restype = C.c_int64
    L.zenc_full_frame.argtypes = L.zenc_frame.argtypes + [C.c_void_p]
    for fn in (L.zenc_compress, L.zenc_full_compress):
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64]
    L.zenc_full_offsets.restype = None
    L.zenc_full_offsets.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def zstd():
    z = zstd_util.load()
    if z is None:
        pytest.skip("libzstd 1.4.9 not present")
    return z


@pytest.fixture(scope="module")
def judge(zstd, oracle):
    def check(frame: bytes, content: bytes):
        got, err = zstd_util.decode(zstd, frame, len(content))
        assert err == 0 and got == content, ("libzstd", err, len(content))
        got, err = oracle.zstd_decode(frame, len(content))
        assert err == 0 and got == content, ("oracle", err, len(content))
    return check


def full_frame(enc, c: Content, checksum=False):
    """Content (test_zstd_enc.py) through zenc_full_frame -> (frame, content, per block the
    (ll, ml, off) triples, per block the offset values chosen)."""
    n = len(c.data)
    nb = max(1, -(-n // c.zb))
    per = [[] for _ in range(nb)]
    for at, ll, ml, off in c.seqs:
        assert (at - ll) // c.zb == (at + ml - 1) // c.zb, "a sequence stays in its block"
        per[(at - ll) // c.zb if ll else at // c.zb].append((ll, ml, off))
    flat = [t for blk in per for t in blk]
    seq3 = np.ascontiguousarray(flat, np.uint32).reshape(-1, 3)
    nseq = np.ascontiguousarray([len(blk) for blk in per], np.uint32)
    src = np.frombuffer(bytes(c.data), np.uint8) if n else np.zeros(1, np.uint8)
    cap = enc.zenc_frame_bound(n)
    out = np.empty(cap, np.uint8)
    ofv = np.zeros(max(len(flat), 1), np.uint32)
    r = enc.zenc_full_frame(src.ctypes.data, n, seq3.ctypes.data if len(flat) else None, nseq.ctypes.data,
                            1 if checksum else 0, out.ctypes.data, cap, ofv.ctypes.data)
    assert 0 < r <= cap, r
    cuts = np.cumsum([0] + [len(blk) for blk in per])
    return out[:r].tobytes(), bytes(c.data), per, [ofv[a:b].tolist() for a, b in zip(cuts, cuts[1:])]


def compress(enc, content: bytes, checksum=0, full=True) -> bytes:
    src = np.frombuffer(content, np.uint8) if content else np.zeros(1, np.uint8)
    cap = enc.zenc_frame_bound(len(content))
    out = np.empty(cap, np.uint8)
    fn = enc.zenc_full_compress if full else enc.zenc_compress
    n = fn(src.ctypes.data, len(content), checksum, out.ctypes.data, cap)
    assert 0 < n <= cap, n
    return out[:n].tobytes()


def tree_form(body: bytes):
    """-> ('direct', weights listed) | ('fse', description bytes) of a Huffman literals section."""
    typ, hl, _, _, _ = lit_info(body)
    assert typ == 2
    hb = body[hl]
    return ("direct", hb - 127) if hb >= 128 else ("fse", hb)


def modes_of(body: bytes):
    """-> (LL, OF, ML modes, the table descriptions' first byte offset in body)"""
    _, hl, _, comp, _ = lit_info(body)
    n, cb = seq_count(body)
    assert n > 0
    at = hl + comp + cb
    m = body[at]
    assert m & 3 == 0
    return (m >> 6, (m >> 4) & 3, (m >> 2) & 3), at + 1


def read_ncount(data: bytes):
    """An FSE table description (RFC 8878 4.1.1) -> (accuracy log, shares, bytes used)."""
    val, pos = int.from_bytes(data, "little"), 0

    def rd(nb):
        nonlocal pos
        v = (val >> pos) & ((1 << nb) - 1)
        pos += nb
        return v

    log = rd(4) + 5
    remaining, norm = (1 << log) + 1, []
    while remaining > 1:
        nb = remaining.bit_length()
        mx = (1 << nb) - 1 - remaining
        v = rd(nb - 1)
        if v >= mx:                      # not one of the short values: one more bit
            hi = rd(1)
            v |= hi << (nb - 1)
            if v >= 1 << (nb - 1):
                v -= mx
        p = v - 1
        remaining -= abs(p)
        norm.append(p)
        if p == 0:
            while True:
                r = rd(2)
                norm += [0] * r
                if r != 3:
                    break
    assert remaining == 1
    return log, norm, (pos + 7) // 8


def sym64(n: int, lo: int = 32) -> bytes:
    return (RNG.integers(0, 64, n, dtype=np.uint8) + lo).astype(np.uint8).tobytes()


def shuffled(count) -> bytes:
    data = np.repeat(np.arange(len(count), dtype=np.uint8), count)
    RNG.shuffle(data)
    return data.tobytes()


# -- the public entries ------------------------------------------------------
def test_full_entries_declared_listed_exported(zs):
    text = open(os.path.join(ROOT, "include", "zseek_hip.h")).read()
    mapped = open(os.path.join(ROOT, "libzseek_amd", "csrc", "libzseek.map")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", zs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"ZSEEK_EXPORT\s+\w+\s+%s\s*\(" % name, text), name
        assert re.search(r"^\s*%s;" % name, mapped, re.M), name
        assert name in zs.EXPORTED and hasattr(zs.lib(), name)
        assert any(ln.split()[-1] == name and ln.split()[-2] == "T" for ln in out.splitlines()), name
    for macro, value in (("ZSK_ZSTD_FORMAT_SUBSET", "0"), ("ZSK_ZSTD_FORMAT_FULL", "1"), ("ZSK_IMAGE_ZSTD_FULL", "4u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), text), macro
    assert (zs.ZSTD_FORMAT_SUBSET, zs.ZSTD_FORMAT_FULL, zs.IMAGE_ZSTD_FULL) == (0, 1, 4)
    L = zs.lib()
    assert L.zsk_zstd_compress_scratch_size_ex(3, 100, 0) == L.zsk_zstd_compress_scratch_size(3, 100) > 0
    assert L.zsk_zstd_compress_scratch_size_ex(3, 100, 1) >= L.zsk_zstd_compress_scratch_size(3, 100)
    assert L.zsk_zstd_compress_scratch_size_ex(3, 100, 2) == 0 == L.zsk_zstd_compress_scratch_size_ex(3, 100, -1)
    assert zs.zstd_compress_scratch_size(3, 100, full=True) == L.zsk_zstd_compress_scratch_size_ex(3, 100, 1)
    # an unknown format is refused before anything else is looked at
    assert L.zsk_zstd_compress_frames_ex(None, 0, None, None, None, None, 0, None, 7) == -1
    assert L.zsk_zstd_compress_frames_ex(None, 0, None, None, None, None, 0, None, 1) == 0


# -- the subset is what it was ---------------------------------------------------
def test_subset_unchanged():
    spec = importlib.util.spec_from_file_location("make_zstd_enc_subset",
                                                  ROOT / "tests/golden/make_zstd_enc_subset.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    want = json.loads((ROOT / "tests/golden/zstd_enc_subset.json").read_text())
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        got = mk.hashes(mk.load_shim(d))
    assert len(want) >= 12 and set(got) == set(want)
    for name in want:
        assert got[name] == want[name], name


# -- a. literals over all 256 byte values ------------------------------------------
def test_high_byte_literals(enc, judge):
    lits = sym64(4096, 160)                                   # bytes 160..223
    frame, content, _, _ = full_frame(enc, Content(enc.zenc_zblock()).lit(lits))
    blocks = parse(frame)[1]
    assert [b[0] for b in blocks] == [2] and lit_info(blocks[0][2])[0] == 2
    assert len(frame) < 0.8 * 4096
    judge(frame, content)
    subset, _ = Content(enc.zenc_zblock()).lit(lits).frame(enc)
    assert [b[0] for b in parse(subset)[1]] == [0], "the subset stores the same content Raw"
    assert compress(enc, lits, full=False) == subset and len(compress(enc, lits)) < 0.8 * 4096


def _geometric(lo: int, hi: int, n: int) -> bytes:
    """n bytes over lo..hi, the likelihood halving every twelfth of the way"""
    k = hi - lo + 1
    p = 0.5 ** (np.arange(k) / (k / 12))
    v = lo + RNG.choice(k, n, p=p / p.sum())
    v[n // 2] = hi                                              # (the last value is there)
    return v.astype(np.uint8).tobytes()


def test_weight_description_forms(enc, judge):
    zb = enc.zenc_zblock()
    seen = set()

    def one(lits, want, streams=None, tail=None):
        c = Content(zb).lit(lits)
        if tail:
            c.match(*tail)
        frame, content, _, _ = full_frame(enc, c)
        body = parse(frame)[1][0]
        assert body[0] == 2
        typ = lit_info(body[2])[0]
        if want == "raw":
            assert typ == 0
        else:
            form, k = tree_form(body[2])
            assert form == want, (form, k)
            if streams:
                assert lit_info(body[2])[4] == streams
            if form == "fse":
                listed = max(lits)
                seen.add(("listed odd" if listed & 1 else "listed even", max(lits) == 255))
        judge(frame, content)
        return body[2]

    # about 200 symbols, geometric: more than 128 weights, so only the FSE form is legal
    one(_geometric(40, 239, 30000), "fse")                    # 239 listed: odd
    one(_geometric(40, 240, 30000), "fse")                    # 240: even
    one(_geometric(56, 255, 30000), "fse")                    # max_sym 255
    # 128 low symbols in two count tiers: 127 weights listed, 65 bytes direct
    body = one(shuffled([24] * 40 + [3] * 88), "fse")
    assert 1 + tree_form(body)[1] < 65
    # few low symbols: the direct form, as in the subset
    body = one(shuffled([300, 200, 100, 50, 50, 20, 10, 5]), "direct")
    assert tree_form(body) == ("direct", 7)
    # 256 equally likely values: 255 equal weights, neither form; a long match keeps the block Compressed
    lits = shuffled([4] * 256)
    one(lits, "raw", tail=(600, len(lits)))
    # one stream at 255 literals, four at 256, bytes above 128 present
    for n, streams in ((255, 1), (256, 4)):
        one((b"\xc8\xc8\xc8\xc9\x41" * 64)[:n], "fse", streams)
    assert {k for k, _ in seen} == {"listed odd", "listed even"} and (("listed odd", True) in seen)


def test_code_lengths_over_256_symbols(enc, judge):
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])                         # an unlimited tree would be 23 deep
    count = np.zeros(256, np.uint32)
    count[200:224] = fib
    count[255], count[3] = 7, 2
    ln, code = np.zeros(256, np.uint8), np.zeros(256, np.uint16)
    mb = enc.zenc_full_huf_lengths(count.ctypes.data, ln.ctypes.data, code.ctypes.data)
    used = [s for s in range(256) if count[s]]
    assert mb == 11 == max(ln[s] for s in used) and all(ln[s] == 0 for s in range(256) if not count[s])
    assert all(1 <= ln[s] <= 11 for s in used)
    assert sum(2 ** (11 - int(ln[s])) for s in used) == 2 ** 11, "Kraft sum exactly 1"
    words = sorted(format(int(code[s]), "0%db" % ln[s]) for s in used)
    assert all(not b.startswith(a) for a, b in zip(words, words[1:])), "prefix-free"
    frame, content, _, _ = full_frame(enc, Content(enc.zenc_zblock()).lit(shuffled(count.tolist())))
    assert lit_info(parse(frame)[1][0][2])[0] == 2
    judge(frame, content)
    # the same counts on low bytes: the subset's lengths, symbol by symbol
    low = np.zeros(129, np.uint32)
    low[40:64] = fib
    wide = np.zeros(256, np.uint32)
    wide[:129] = low
    ln_s, code_s = np.zeros(129, np.uint8), np.zeros(129, np.uint16)
    assert enc.zenc_huf_lengths(low.ctypes.data, ln_s.ctypes.data, code_s.ctypes.data) == \
        enc.zenc_full_huf_lengths(wide.ctypes.data, ln.ctypes.data, code.ctypes.data)
    assert np.array_equal(ln[:129], ln_s) and np.array_equal(code[:129], code_s)


# -- b. sequence table modes -----------------------------------------------------------
def _uniform_seqs(zb, k, off0=20):
    """k sequences of one LL, one ML and one OF code: ll 40, ml 3, offsets off0, off0 + 1, ..."""
    c = Content(zb)
    for i in range(k):
        c.lit(sym64(40)).match(3, off0 + i)
    return c.lit(sym64(100))


def _skewed_seqs(zb, k, head=None, big_ll=0, rare_ll=False):
    """k sequences whose codes sit on few values: each table is worth a description"""
    c = Content(zb).lit(sym64(400)) if head is None else head
    if big_ll:
        c.lit(sym64(big_ll)).match(4, 100)
    lls = RNG.choice([0, 1, 2], k, p=[0.1, 0.7, 0.2])
    mls = RNG.choice([3, 4, 5], k, p=[0.6, 0.3, 0.1])
    offs = RNG.choice([33, 65, 129, 130], k, p=[0.5, 0.3, 0.1, 0.1])
    for i in range(k):
        ll = 30 if rare_ll and i == k // 2 else int(lls[i])
        c.lit(sym64(ll)).match(int(mls[i]), int(offs[i]) + (i & 7))
    return c


@pytest.fixture(scope="module")
def mode_cases(enc):
    zb, n = enc.zenc_zblock(), enc.zenc_full_custom_min()
    cases = {
        "below": _uniform_seqs(zb, n - 1),
        "at": _uniform_seqs(zb, n),
        "skewed": _skewed_seqs(zb, 3000),
        "rare": _skewed_seqs(zb, 3000, rare_ll=True),
        "ll35": _skewed_seqs(zb, 3000, big_ll=65536),
        "ml52": _skewed_seqs(zb, 3000, head=Content(zb).lit(sym64(300)).match(65539 + 17, 300)),
    }
    out = {name: full_frame(enc, c) for name, c in cases.items()}
    # the largest offset code a 4 MiB frame reaches: its last 3 bytes copied from its first 3 (offset
    # 4 Mi - 3, value 4 Mi, code 22), in a block with sequences enough for a custom table
    big = Content(zb)
    for _ in range(31):
        big.lit(sym64(zb)).cut()
    _skewed_seqs(zb, 3000, head=big.lit(sym64(2000)))
    big.lit(sym64((1 << 22) - 3 - len(big.data))).match(3, (1 << 22) - 3)
    assert len(big.data) == 1 << 22
    out["of_far"] = full_frame(enc, big)
    return out


def test_sequence_table_modes(enc, judge, mode_cases):
    n = enc.zenc_full_custom_min()
    assert n == 8
    seen = set()
    for name, (frame, content, per, _) in mode_cases.items():
        judge(frame, content)
        blocks = parse(frame)[1]
        assert blocks[-1][0] == 2, name
        modes, _ = modes_of(blocks[-1][2])
        seen |= {(t, m) for t, m in zip("LOM", modes)}
        if name == "below":
            assert seq_count(blocks[0][2])[0] == n - 1 and modes == (PRE, PRE, PRE), "fewer than N: Predefined"
        elif name == "at":
            assert seq_count(blocks[0][2])[0] == n and modes == (RLE, RLE, RLE), "N sequences of one code each"
        else:
            assert modes == (FSE, FSE, FSE), (name, modes)
    assert seen == {(t, m) for t in "LOM" for m in (PRE, RLE, FSE)}


def test_custom_tables_hold_the_edges(enc, mode_cases):
    def tables(name):
        body = parse(mode_cases[name][0])[1][-1][2]
        modes, at = modes_of(body)
        out = []
        for _ in range(3):
            log, norm, used = read_ncount(body[at:at + 100])
            out.append((log, norm))
            at += used
        return out

    (ll_log, ll), (of_log, of), (ml_log, ml) = tables("skewed")
    assert 5 <= ll_log <= 9 and 5 <= of_log <= 8 and 5 <= ml_log <= 9
    assert sum(abs(p) for p in ll) == 1 << ll_log
    ll = tables("rare")[0][1]
    assert ll[21] == -1 and ll[1] > 100, "ll 30 (code 21) once among 3000: less than one"
    ll = tables("ll35")[0][1]
    assert len(ll) == 36 and ll[35] == -1, "LL code 35 in a custom table"
    ml = tables("ml52")[2][1]
    assert len(ml) == 53 and ml[52] == -1, "ML code 52 in a custom table"
    of = tables("of_far")[1][1]
    assert len(of) == 23 and of[22] == -1, "offset code 22: the largest a 4 MiB frame reaches"


def test_existing_edge_contents_in_the_full_format(enc, judge):
    zb = enc.zenc_zblock()
    cases = [Content(zb).lit(b"ab").match(zb - 2, 2),
             Content(zb).lit(sym64(600)).match(3, 1).lit(b"x").match(3, 9),
             Content(zb).lit(sym64(70000)).match(100, 70000).match(50, 1).match(3, 69000),
             Content(zb).lit(sym64(zb)).cut().lit(sym64(zb, 160)).cut().lit(sym64(996)).match(3, 2 * zb + 999 - 3)]
    for c in cases:
        for ck in (False, True):
            frame, content, _, _ = full_frame(enc, c, ck)
            judge(frame, content)


# -- c. repeat offsets -------------------------------------------------------------------
def rfc_offsets(per, committed):
    """RFC 8878 3.1.1.5 restated: per block the offset values a greedy encoder writes and the
    history after them; the history moves on only over the blocks in `committed`."""
    rep, out = [1, 4, 8], []
    for b, seqs in enumerate(per):
        h, vals = list(rep), []
        for ll, _, off in seqs:
            # values 1, 2, 3 name these offsets (the first that fits is written)
            named = [h[0], h[1], h[2]] if ll else [h[1], h[2]] + ([h[0] - 1] if h[0] - 1 else [])
            v = named.index(off) + 1 if off in named else off + 3
            vals.append(v)
            # the decoder's side of it: what the history is after reading v
            if v > 3:
                h = [off, h[0], h[1]]
            else:
                idx = v - 1 + (ll == 0)
                if idx == 1:
                    h = [h[1], h[0], h[2]]
                elif idx == 2:
                    h = [h[2], h[0], h[1]]
                elif idx == 3:
                    h = [h[0] - 1, h[0], h[1]]
            assert h[0] == off
        out.append(vals)
        if b in committed:
            rep = h
    return out


REP_CASES = {
    # name: ((ll, off) of each sequence (ml 5; the first one follows 600 literals that pay for the
    # block, whatever its ll says), the offset values expected)
    "rep1_ll": ([(0, 10), (2, 10)], [13, 1]),
    "rep2_ll": ([(0, 10), (2, 20), (2, 10)], [13, 23, 2]),
    "rep3_ll": ([(0, 10), (2, 20), (2, 30), (2, 10)], [13, 23, 33, 3]),
    "ll0_rep2": ([(0, 10), (2, 20), (0, 10)], [13, 23, 1]),
    "ll0_rep3": ([(0, 10), (2, 20), (2, 30), (0, 10)], [13, 23, 33, 2]),
    "ll0_rep1_minus1": ([(0, 10), (0, 9)], [13, 3]),
    "ll0_rep1_is_plain": ([(0, 10), (0, 10)], [13, 13]),
    "first_offset_1": ([(0, 1)], [1]),
    "first_offset_4": ([(0, 4)], [2]),
    "first_offset_8": ([(0, 8)], [3]),
}


@pytest.mark.parametrize("name", sorted(REP_CASES))
def test_repeat_offset_rules(enc, judge, name):
    ops, want = REP_CASES[name]
    zb = enc.zenc_zblock()
    c = Content(zb).lit(sym64(600))
    for ll, off in ops:
        c.lit(sym64(ll)).match(5, off)
    frame, content, per, ofv = full_frame(enc, c)
    assert parse(frame)[1][0][0] == 2
    assert ofv[0] == want, (ofv, want)
    assert ofv == rfc_offsets(per, {0})
    seq3 = np.ascontiguousarray(per[0], np.uint32)
    flat = np.zeros(len(per[0]), np.uint32)
    enc.zenc_full_offsets(seq3.ctypes.data, len(per[0]), flat.ctypes.data)
    assert flat.tolist() == want
    judge(frame, content)


def _noise(n: int) -> bytes:
    return RNG.integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("between", ["none", "raw", "rle", "encoded_then_raw"])
def test_repeat_offsets_across_blocks(enc, judge, between):
    zb = enc.zenc_zblock()
    c = Content(zb).lit(sym64(zb - 5)).match(5, 50).cut()                 # block 0 ends on offset 50
    types = [2]
    if between == "raw":
        c.lit(_noise(zb)).cut()
        types.append(0)
    elif between == "rle":
        c.lit(b"\x99" * zb).cut()
        types.append(1)
    elif between == "encoded_then_raw":                                    # a match that cannot pay for noise
        c.lit(_noise(zb - 3)).match(3, 77).cut()
        types.append(0)
    c.lit(sym64(700)).match(5, 77).lit(sym64(3)).match(5, 50).lit(sym64(3)).match(5, 4)
    types.append(2)
    frame, content, per, ofv = full_frame(enc, c)
    assert [b[0] for b in parse(frame)[1]] == types
    committed = {i for i, t in enumerate(types) if t == 2}
    assert ofv[0] == [53] and ofv[-1] == [80, 2, 7], "50 is still in the history, 77 never entered it"
    if between == "encoded_then_raw":
        assert ofv[1] == [80], "the discarded block had chosen its value"
    assert ofv == rfc_offsets(per, committed)
    judge(frame, content)


# -- the whole pipeline ---------------------------------------------------------------------
def _generated(i: int) -> bytes:
    r = np.random.default_rng(7000 + i)
    n = [0, 300 << 10, 1, (1 << 17) + 1][i] if i < 4 else int(2 ** r.uniform(0, np.log2(300 << 10)))
    alphabet = i % 5
    if alphabet == 0:
        base = r.integers(32, 96, n, dtype=np.uint8)              # low
    elif alphabet == 1:
        base = r.integers(160, 256, n, dtype=np.uint8)            # high
    elif alphabet == 2:
        base = np.minimum(r.geometric(0.03, n), 255).astype(np.uint8) ^ np.uint8(0x55 if i & 8 else 0)   # mixed
    elif alphabet == 3:
        base = np.full(n, 0xE7 if i & 8 else 0x20, np.uint8)      # one symbol
    else:
        base = (r.integers(0, 2, n, dtype=np.uint8) * 0x7F + 0x40).astype(np.uint8)   # two: 0x40, 0xBF
    structure = (i // 5) % 4
    if structure == 1 and n:                                      # short periods
        k = int(r.integers(1, 40))
        base = np.tile(base[:k], n // k + 1)[:n]
    elif structure == 2 and n:                                    # long periods
        k = int(r.integers(300, 5000))
        base = np.tile(base[:k], n // k + 1)[:n]
    elif structure == 3 and n > 64:                               # repeats from anywhere in the frame
        base = base.copy()
        for _ in range(int(r.integers(1, 40))):
            ln = int(r.integers(4, max(5, n // 8)))
            a, b = int(r.integers(0, n - ln + 1)), int(r.integers(0, n - ln + 1))
            base[b:b + ln] = base[a:a + ln].copy()
    return base.tobytes()


def test_generated_contents(enc, zstd, oracle):
    zb = enc.zenc_zblock()
    kinds = set()
    for i in range(300):
        content = _generated(i)
        frame = compress(enc, content, i & 1)
        assert len(frame) <= enc.zenc_frame_bound(len(content))
        got, err = zstd_util.decode(zstd, frame, len(content))
        assert err == 0 and got == content, ("libzstd", i, err)
        got, err = oracle.zstd_decode(frame, len(content))
        assert err == 0 and got == content, ("oracle", i, err)
        at = 0
        for typ, size, body in parse(frame)[1]:
            bn = min(zb, len(content) - at)
            assert typ != 2 or size < bn, (i, "Compressed at a size >= its input")
            at += bn
            kinds.add(typ)
    assert kinds == {0, 1, 2}
