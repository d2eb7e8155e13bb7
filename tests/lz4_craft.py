"""Hand-built LZ4 sequence streams at the edges of the block and frame format.

Every other LZ4 block the suite decodes came out of a compressor, which emits
a narrow dialect: blocks end in >= 5 literals after a match that ends >= 12
bytes from the end, offset 0 and zero-byte blocks never appear, extension
chains rarely end in a 0 byte.  This module writes the token / extension /
offset bytes itself, so a case can sit exactly on a rule of liblz4 1.9.3's
LZ4_decompress_safe (MFLIMIT = 12, LASTLITERALS = 5, the history floor, the
block capacity) and on the sizes where the GPU engines change path (the
two-item split at lit > 255 or ml > 258, the 128 / 256-byte literal rings, the
3072-byte execute stage, 16-item lines).

  seq / raw_seq      one sequence, canonical / with explicit malformed fields
  lz4f_frame, frame  an LZ4F frame around block payloads
  expand             the intended output, byte by byte (the plain reference)
  seekable           frames + a seek table
  CASES, PAIRS       the named table and its accepted / rejected boundary pairs
  random_valid       edge-biased generator of valid frames
  decode, check      a batch through zsk_lz4_decode_frames, held to the oracle

A case's verdict here is written down from the format rules; tests/golden/
lz4_craft.json records what liblz4 1.9.3 and the compiled reference reader
make of the same frames (make_lz4_craft.py), and test_lz4_craft.py holds the
table and the oracle to that record.
"""
from __future__ import annotations

import numpy as np
import xxhash

CAP = {4: 1 << 16, 5: 1 << 18, 6: 1 << 20, 7: 1 << 22}

# lengths and offsets at each encoding edge (token nibble 15, extension bytes
# 255 / 0) and each engine edge (items split at lit > 255 / ml > 258)
LIT_EDGES = [0, 1, 14, 15, 16, 254, 255, 256, 269, 270, 271, 524, 525]
ML_EDGES = [4, 5, 18, 19, 20, 258, 259, 273, 274, 275, 528, 529]
OFF_EDGES = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257]


# ---------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------
def _ext(n: int) -> bytes:
    """extension bytes of a length whose token nibble is 15 (n = length - 15)"""
    return b"\xff" * (n // 255) + bytes([n % 255])


def seq(lit: bytes, off=None, ml=None) -> bytes:
    """One sequence: token, literal extension, literals, offset, match
    extension.  `ml` is the real match length (>= 4); off=None: the
    literals-only last sequence of a block."""
    n = len(lit)
    if off is None:
        return bytes([min(n, 15) << 4]) + (_ext(n - 15) if n >= 15 else b"") + bytes(lit)
    assert ml >= 4 and 0 <= off <= 0xFFFF
    m = ml - 4
    return (bytes([min(n, 15) << 4 | min(m, 15)]) + (_ext(n - 15) if n >= 15 else b"") + bytes(lit)
            + int(off).to_bytes(2, "little") + (_ext(m - 15) if m >= 15 else b""))


def raw_seq(token: int, lit_ext: bytes = b"", lit: bytes = b"", off: bytes = b"", ml_ext: bytes = b"",
            cut: int | None = None) -> bytes:
    """A sequence from explicit fields (nothing is derived or checked), cut to
    its first `cut` bytes: the malformed cases."""
    s = bytes([token]) + lit_ext + lit + off + ml_ext
    return s if cut is None else s[:cut]


def expand(seqs, out: bytearray | None = None) -> bytes:
    """What (literals, offset, match length) sequences decode to, after the
    history `out`: byte-by-byte copies, zeros for offset 0 (liblz4 1.9.3)."""
    out = bytearray() if out is None else out
    for lit, off, ml in seqs:
        out += lit
        if off is not None:
            for _ in range(ml):
                out.append(out[-off] if off else 0)
    return bytes(out)


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------
def lz4f_frame(blocks, flg=0x60, bd=0x40, content_size=None, dict_id=None, tail=b"", content=None):
    """An LZ4F frame (magic, descriptor, header checksum) of the given blocks:
    bytes payloads are stored blocks, (h, payload) pairs are copied.  FLG's
    block-checksum bit adds each block's XXH32; its content-checksum bit adds
    XXH32(content) after the end mark."""
    if content_size is not None:
        flg |= 8
    if dict_id is not None:
        flg |= 1
    desc = bytes([flg, bd])
    if content_size is not None:
        desc += int(content_size).to_bytes(8, "little")
    if dict_id is not None:
        desc += int(dict_id).to_bytes(4, "little")
    out = bytearray(b"\x04\x22\x4d\x18" + desc + bytes([(xxhash.xxh32(desc).intdigest() >> 8) & 0xFF]))
    for b in blocks:
        if isinstance(b, (bytes, bytearray)):
            b = (len(b) | 0x80000000, bytes(b))
        out += b[0].to_bytes(4, "little") + b[1]
        if flg & 0x10:
            out += xxhash.xxh32(b[1]).intdigest().to_bytes(4, "little")
    out += b"\0\0\0\0"
    if flg & 4:
        out += xxhash.xxh32(content).intdigest().to_bytes(4, "little")
    return bytes(out + tail)


def frame(blocks, bsid=4, independent=True, stored=(), content_size=None, block_checksum=False,
          content_checksum=False, content=None) -> bytes:
    """An LZ4F frame of block payloads (bytes each); the blocks whose index is
    in `stored` are written as stored blocks.  `content`: the decoded bytes,
    needed for the content checksum."""
    flg = 0x40 | (0x20 if independent else 0) | (0x10 if block_checksum else 0) | (4 if content_checksum else 0)
    bl = [bytes(b) if i in stored else (len(b), bytes(b)) for i, b in enumerate(blocks)]
    return lz4f_frame(bl, flg=flg, bd=bsid << 4, content_size=content_size, content=content)


def seekable(frames, dsizes) -> bytes:
    """the frames + a seek table (zseek's skippable frame, no checksums)"""
    n = len(frames)
    table = bytearray((0x184D2A5E).to_bytes(4, "little") + (8 * n + 9).to_bytes(4, "little"))
    for f, s in zip(frames, dsizes):
        table += len(f).to_bytes(4, "little") + int(s).to_bytes(4, "little")
    table += n.to_bytes(4, "little") + bytes([0]) + (0x8F92EAB1).to_bytes(4, "little")
    return b"".join(frames) + bytes(table)


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
def lits(n: int, salt: int = 0) -> bytes:
    """n deterministic bytes without a short period"""
    return bytes(((i * 131 + salt * 29 + 7) ^ (i >> 6) ^ (i >> 11)) & 0xFF for i in range(n))


class S(bytes):
    """a stored block"""


class R(bytes):
    """a compressed block given as raw payload bytes"""


CASES: list = []      # (name, frame bytes, declared dsize, expected bytes | None)
PAIRS: list = []      # (accepted case, rejected case): the two sides of one boundary
NEIGHBOURS: list = []  # two intact (frame, dsize) for a case to sit between


def _build(blocks, **kw):
    """blocks: lists of (lit, off, ml) sequences, S(...) stored or R(...) raw
    payloads -> (frame bytes, the intended output)"""
    out = bytearray()
    payloads, stored = [], set()
    for i, b in enumerate(blocks):
        if isinstance(b, S):
            stored.add(i)
            payloads.append(bytes(b))
            out += b
        elif isinstance(b, R):
            payloads.append(bytes(b))
        else:
            payloads.append(b"".join(seq(*s) for s in b))
            end = len(out) + sum(len(lit) + (ml or 0) for lit, _, ml in b)
            try:
                expand(b, out)
            except IndexError:                  # a match from before the frame: only the size is meant
                out += bytes(end - len(out))
    if kw.get("content_checksum") and "content" not in kw:
        kw["content"] = bytes(out)
    if kw.get("content_size") is True:
        kw["content_size"] = len(out)
    return frame(payloads, stored=stored, **kw), bytes(out)


def _add(name, blocks, ok, dsize=None, want=None, **kw):
    """`want`: the intended output of a frame with raw blocks that is valid"""
    f, out = _build(blocks, **kw)
    want = out if want is None else want
    assert all(name != c[0] for c in CASES), name
    CASES.append((name, f, len(want) if dsize is None else dsize, want if ok else None))
    return name


def _pair(good, bad):
    PAIRS.append((good, bad))


def T(k, salt=9):
    """the literals-only last sequence"""
    return (lits(k, salt), None, None)


HEAD = (lits(8, 1), 8, None)   # 8 literals, then a match that copies them


def _head(ml):
    return (HEAD[0], 8, ml)


def _make_cases():
    c4, c5 = CAP[4], CAP[5]

    # --- a. end-of-block rules -------------------------------------------
    # input side: a match-bearing sequence needs 8 bytes after its literals,
    # and every match extension byte needs 5 bytes after it
    for ml, kmin in ((18, 5), (19, 4), (274, 4)):
        names = {k: _add(f"a_ml{ml}_tail{k}", [[_head(ml), T(k)]], k >= kmin) for k in (0, kmin - 1, kmin, kmin + 1)}
        _pair(names[kmin], names[kmin - 1])
        # ... and with a last sequence whose literal count takes an extension
        # byte (token 0xF0): always long enough; its rejected side declares
        # 15 literals and brings 14
        good = [_add(f"a_ml{ml}_tail{k}", [[_head(ml), T(k)]], True) for k in (15, 16, 270)]
        bad = _add(f"a_ml{ml}_tail15_short",
                   [R(seq(*_head(ml)) + raw_seq(0xF0, b"\x00", lits(14, 9)))], False, dsize=8 + ml + 15)
        _pair(good[0], bad)
    # output side: literals may end at cap - 12 before a match, no later
    for bsid, cap, run in ((4, c4, 60000), (5, c5, 100000)):
        for d, ok in ((13, True), (12, True), (11, False)):
            n = cap - d - (1 + run)
            nm = _add(f"a_bsid{bsid}_lit_end_cap-{d}", [[(b"s", 1, run), (lits(n, 2), 1, 4), T(5)]], ok, bsid=bsid)
            if d != 13:
                names[d] = nm
        _pair(names[12], names[11])
        # a match may end at cap - 5, no later
        for d, ok in ((6, True), (5, True), (4, False)):
            names[d] = _add(f"a_bsid{bsid}_match_end_cap-{d}", [[(b"m", 1, cap - d - 1), T(5)]], ok, bsid=bsid)
        _pair(names[5], names[4])
        # a block may decode to cap bytes, no more
        full = _add(f"a_bsid{bsid}_block_cap", [[(b"c", 1, cap - 8), T(7)]], True, bsid=bsid)
        over = _add(f"a_bsid{bsid}_block_cap+1", [[(b"c", 1, cap - 8), T(8)]], False, bsid=bsid)
        _pair(full, over)
        assert len(CASES[-2][3]) == cap

    # --- b. lengths around each encoding and item edge -------------------
    pre = (lits(5, 3), 3, 4)
    for n in LIT_EDGES:
        _add(f"b_lit{n}_ml4", [[pre, (lits(n, 4), 2, 4), T(5)]], True)
    for ml in ML_EDGES:
        for n in (0, 1):
            _add(f"b_ml{ml}_lit{n}", [[pre, (lits(n, 5), 7, ml), T(5)]], True)
    for n in (255, 256):
        for ml in (258, 259):
            _add(f"b_lit{n}_ml{ml}", [[pre, (lits(n, 6), 9, ml), T(5)]], True)

    # --- c. offsets and overlap ------------------------------------------
    for off in OFF_EDGES:
        for ml in (4, 7, 64, 65, 300, 3100):
            _add(f"c_off{off}_ml{ml}", [[(lits(off + 3, off), off, ml), T(5)]], True)
    # offset 0: liblz4 1.9.3 only checks that the match starts inside the
    # history, and its short-offset copy then writes zeros
    _add("c_off0_first_nolit", [[(b"", 0, 8), T(5)]], True)
    _add("c_off0_first", [[(lits(3, 7), 0, 8), T(5)]], True)
    _add("c_off0_second", [[_head(6), (lits(2, 7), 0, 21), T(5)]], True)
    _add("c_off0_last_match", [[_head(6), (lits(20, 7), 3, 9), (b"", 0, 4), T(5)]], True)
    _add("c_off0_linked_block2", [[_head(30), T(9)], [(lits(4, 8), 0, 300), (b"", 5, 5), T(6)]], True,
         independent=False)
    _add("c_off0_indep_block2", [[_head(30), T(9)], [(lits(4, 8), 0, 300), (b"", 5, 5), T(6)]], True)

    # --- d. history floor --------------------------------------------------
    _pair(_add("d_off_eq_op", [[(lits(7, 1), 7, 8), T(5)]], True),
          _add("d_off_eq_op+1", [[(lits(7, 1), 8, 8), T(5)]], False))
    b0 = [(lits(20, 2), None, None)]
    _pair(_add("d_indep_block_first_byte", [b0, [(lits(6, 3), 6, 5), T(5)]], True),
          _add("d_indep_before_block", [b0, [(lits(6, 3), 7, 5), T(5)]], False))
    _pair(_add("d_linked_before_block", [b0, [(lits(6, 3), 7, 5), T(5)]], True, independent=False),
          _add("d_linked_before_frame", [b0, [(lits(6, 3), 27, 5), T(5)]], False, independent=False))
    _add("d_linked_frame_first_byte", [b0, [(lits(6, 3), 26, 5), T(5)]], True, independent=False)
    big = S(lits(c4, 4))
    _pair(_add("d_linked_65535_block2", [big, [(b"", 65535, 8), T(5)]], True, independent=False),
          _add("d_linked_65535_block2_short", [S(big[:65534]), [(b"", 65535, 8), T(5)]], False, independent=False))
    _add("d_linked_65535_block2_lit1", [big, [(b"x", 65535, 8), T(5)]], True, independent=False)
    _pair(_add("d_linked_65535_block3", [S(big[:40000]), S(big[:20000]), [(lits(5535, 5), 65535, 70), T(5)]],
               True, independent=False),
          _add("d_linked_65535_block3_short", [S(big[:39999]), S(big[:20000]), [(lits(5535, 5), 65535, 70), T(5)]],
               False, independent=False))

    # --- e. runs longer than the rings -----------------------------------
    for n in (130, 260, 5000):
        for off in (1, 2, 3, 4, n):
            _add(f"e_run{n}_off{off}", [[(lits(n, off), off, 20), T(5)]], True)
    _add("e_dense_40x_ml4", [[(lits(4, 1), 4, 4)] + [(b"", 4, 4)] * 40 + [T(5)]], True)
    for items in (16, 17, 32, 33):
        body = [(lits(1 + i % 3, i), 1 + i % 4, 4 + i % 17) for i in range(items - 1)]
        _add(f"e_items{items}", [[(lits(4, 1), 2, 4)] + body[1:] + [T(5)]], True)
        # the same count with one sequence that splits into two items
        split = [(lits(4, 1), 2, 4), (lits(300, 2), 300, 300)] + body[3:] + [T(5)]
        _add(f"e_items{items}_split", [split], True)

    # --- f. block structure ------------------------------------------------
    z = [(b"", None, None)]                     # the single token 0x00
    blk = [_head(10), T(6)]
    _add("f_zero_block_only", [z], True)
    _add("f_zero_blocks_only", [z, z, z], True)
    _add("f_zero_block_first", [z, blk], True)
    _add("f_zero_block_middle", [blk, z, blk], True)
    _add("f_zero_block_last", [blk, z], True)
    _add("f_zero_block_middle_linked", [blk, z, [(lits(3, 2), 20, 12), T(5)]], True, independent=False)
    _add("f_stored_comp_stored", [S(lits(40, 1)), blk, S(lits(7, 2))], True)
    _add("f_comp_stored_comp_linked", [blk, S(lits(40, 1)), [(b"", 50, 30), T(5)]], True, independent=False)
    _add("f_stored_1byte_blocks", [S(b"a"), S(b"b"), blk, S(b"c")], True)
    _add("f_literals_only_block", [[T(100)]], True)
    _add("f_literals_only_block_1", [[T(1)]], True)
    _add("f_block_checksum", [blk, S(lits(9, 1)), blk], True, block_checksum=True)
    _add("f_content_checksum", [blk, S(lits(9, 1)), blk], True, content_checksum=True)
    _pair(_add("f_both_checksums", [blk, blk], True, block_checksum=True, content_checksum=True),
          _add("f_content_checksum_wrong", [blk, blk], False, content_checksum=True, content=b"other"))
    _pair(_add("f_content_size_right", [blk, blk], True, content_size=True),
          _add("f_content_size_plus1", [blk, blk], False, content_size=49))
    _add("f_content_size_minus1", [blk, blk], False, content_size=47)
    _pair(_add("f_dsize_right", [blk, S(lits(5, 1))], True),
          _add("f_dsize_plus1", [blk, S(lits(5, 1))], False, dsize=30))
    _add("f_dsize_minus1", [blk, S(lits(5, 1))], False, dsize=28)
    _add("f_dsize_minus1_literals", [[_head(10), T(11)]], False, dsize=28)

    # --- g. malformed streams ----------------------------------------------
    h = seq(*_head(10))
    # token 0xF0 needs 15 bytes after it besides its first extension byte
    _pair(_add("g_f0_16_before_end", [R(h + raw_seq(0xF0, b"\x00", lits(15, 9)))], True,
               want=expand([_head(10), T(15)])),
          _add("g_f0_15_before_end", [R(h + raw_seq(0xF0, b"\x00", lits(14, 9)))], False, dsize=33))
    _add("g_lit_ext_runs_off", [R(h + raw_seq(0xF0, b"\xff" * 20))], False, dsize=4000)
    _add("g_match_ext_runs_off", [R(raw_seq(0x8F, b"", HEAD[0], b"\x08\x00", b"\xff" * 12))], False, dsize=4000)
    _add("g_match_ext_then_tail_missing", [R(raw_seq(0x8F, b"", HEAD[0], b"\x08\x00", b"\xff\x03"))], False,
         dsize=4000)
    _add("g_offset_cut_in_half", [R(h + raw_seq(0x30, b"", b"abc", b"\x02"))], False, dsize=40)
    _add("g_offset_missing", [R(h + raw_seq(0x31, b"", b"abc"))], False, dsize=40)
    _pair(_add("g_lit_count_exact", [R(h + raw_seq(0x60, b"", lits(6, 9)))], True, want=expand([_head(10), T(6)])),
          _add("g_lit_count_one_more", [R(h + raw_seq(0x70, b"", lits(6, 9)))], False, dsize=25))
    _add("g_last_seq_one_byte_over", [R(h + raw_seq(0x60, b"", lits(6, 9)) + b"\x00")], False, dsize=24)
    _add("g_last_seq_one_lit_over", [R(h + raw_seq(0x50, b"", lits(6, 9)))], False, dsize=24)

    NEIGHBOURS.append(_build([[(lits(300, 11), 17, 40), (lits(3, 12), 300, 500), T(12)]]))
    NEIGHBOURS.append(_build([[_head(90), T(5)], S(lits(33, 13))], independent=False))


_make_cases()
CASE = {c[0]: c for c in CASES}


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
def random_valid(seed: int, n: int):
    """n valid frames of at most 4 KiB decoded, as (frame bytes, expected
    bytes): literal lengths, match lengths and offsets drawn from the edge
    lists mixed with uniform values, one to three blocks (linked or
    independent, some stored, some empty).  Valid by construction: an offset
    never reaches below the history floor, a block's last sequence has 5
    literals or more (4 after a match with extension bytes), and no block
    comes near its capacity -- so the oracle must accept every one of them."""
    rng = np.random.default_rng(seed)
    out = []

    def pick(edges, lo, hi):
        return int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(lo, hi))

    for i in range(n):
        independent = bool(rng.integers(0, 2))
        budget = int(rng.choice([40, 300, 1500, 4080]))
        blocks, total = [], 0
        for _ in range(int(rng.choice([1, 1, 2, 3]))):
            kind = rng.random()
            if kind < 0.1:
                blocks.append([(b"", None, None)])
                continue
            if kind < 0.2:
                m = min(pick([1, 15, 16], 1, 60), budget - total)
                if m > 0:
                    blocks.append(S(lits(m, i)))
                    total += m
                continue
            floor, op, seqs, ext = (total if independent else 0), total, [], False
            for _ in range(int(rng.choice([0, 1, 2, 5, 20, 40]))):
                lit = pick(LIT_EDGES, 0, 40)
                ml = pick(ML_EDGES, 4, 40)
                if op + lit + ml + 5 > budget:
                    lit, ml = min(lit, 3), 4 + min(ml, 15) % 8
                    if op + lit + ml + 5 > budget:
                        break
                room = op + lit - floor
                if room == 0:
                    lit = 1 + lit % 3
                    room = lit
                off = min(pick(OFF_EDGES, 1, room + 1), room)
                if rng.random() < 0.15:
                    off = room                         # the match starts at the floor
                if rng.random() < 0.03:
                    off = 0
                seqs.append((lits(lit, len(seqs) + i), off, ml))
                op += lit + ml
                ext = ml >= 19
            k = pick([5, 6, 15, 16, 270], 5, 30) if seqs else pick([0, 1, 15, 270], 0, 30)
            if seqs and ext and rng.random() < 0.3:
                k = 4
            k = max(min(k, budget - op), (4 if ext else 5) if seqs else 0)
            seqs.append((lits(k, 77 + i), None, None))
            blocks.append(seqs)
            total = op + k
        if not blocks:
            blocks.append([(b"", None, None)])
        out.append(_build(blocks, independent=independent))
    return out


# ---------------------------------------------------------------------------
# the device batch API (needs a GPU)
# ---------------------------------------------------------------------------
def decode(zs, gpu, frames, dsizes, engine):
    """frames back to back through zsk_lz4_decode_frames(_ex) -> (each frame's
    output slot, statuses)"""
    import torch
    n = len(frames)
    c = np.cumsum([0] + [len(f) for f in frames])
    d = np.cumsum([0] + list(dsizes))
    desc = np.zeros(n, dtype=[("c_off", "<u8"), ("d_off", "<u8"), ("c_size", "<u4"), ("d_size", "<u4")])
    desc["c_off"], desc["d_off"] = c[:-1], d[:-1]
    desc["c_size"], desc["d_size"] = np.diff(c), np.asarray(dsizes)
    td = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    comp = torch.zeros(int(c[-1]) + 256, dtype=torch.uint8, device=gpu)
    comp[: int(c[-1])].copy_(torch.from_numpy(np.frombuffer(b"".join(frames), np.uint8).copy()))
    out = torch.zeros(max(int(d[-1]), 1), dtype=torch.uint8, device=gpu)
    status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    zs.decode_frames(td, comp, out, status, engine=engine)
    torch.cuda.synchronize()
    o = out.cpu().numpy().tobytes()
    return [o[int(d[i]): int(d[i + 1])] for i in range(n)], status.cpu().tolist()


def check(zs, oracle, gpu, frames, dsizes, engine="block"):
    """engine == oracle (status, bytes of OK frames) and == wave statuses"""
    got, st = decode(zs, gpu, frames, dsizes, engine)
    _, st_w = decode(zs, gpu, frames, dsizes, "wave")
    assert st == st_w
    for i, (f, ds) in enumerate(zip(frames, dsizes)):
        ost, obytes, _, _ = oracle.decode_frame(f, ds)
        if ost == 0 and len(obytes) == ds:
            assert st[i] == 0, (i, zs.status_string(st[i]))
            assert got[i] == obytes, i
        else:
            assert st[i] != 0, i
    return st
