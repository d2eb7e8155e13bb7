"""Hand-built *linked* LZ4 frames of full 64 KiB blocks: the inputs of the
block plan (lz4_split.hip), the block lanes (lz4_lean.hip), the accept /
re-parse step (lz4_chunk.hip), the job segments (seq_exec.hip) and, above all,
of the block-parallel execute of the one-frame route (seq_exec_blocks_kernel).

That kernel runs every block of a frame at once.  A byte copied from before
its block, or from a byte so copied, is *tainted*: it holds its origin in the
previous block, not its value, and is resolved after the earlier blocks have
published by following origins back block by block.  lz4_craft.py's linked
cases have short first blocks, which the block plan declines, so none of them
reaches that code.  Here every block but the last decodes to exactly B = 65,536
bytes (unless the case is about that), block size id 4, no checksums, and the
matches sit on the taint code's edges:

  a  where taint enters: first sequences at block position 0, matches that
     straddle the block start at every clip phase, both sides of the
     lane-per-byte / 16-byte-piece switch (offset 15|16, length 256|257)
  b  taint bits against the 32-bit words they are kept in
  c  later generations inside a block (a tainted source, a half-tainted one)
  d  how many bytes of a block are tainted (the split over 1,024 threads)
  e  hop chains through up to 63 blocks
  f  the block plan's and the origin scratch's limits
  g  refused frames

Block 0 is a stored block (variant 0) or a compressed block with matches of
its own (variant 1); where a family is a cross product the variants alternate
over it, so every offset and every length meets both.

  CASES, BLOCKS      the table (as lz4_craft.CASES) and each case's sequences
  case               one row of it by name
  random_linked      edge-biased generator of valid linked frames
  taint_stats        the definition of taint, byte by byte: counts, hops,
                     generations, copy rules
  decode             a batch into a 0xA5-prefilled buffer
"""
from __future__ import annotations

import numpy as np

import lz4_craft
from lz4_craft import LIT_EDGES, ML_EDGES, R, S, _build, raw_seq, seq

B = 65536
SENT = 0xA5

_LITS: dict = {}


def lits(n: int, salt: int = 0) -> bytes:
    """lz4_craft.lits (the same bytes; test_lz4_linked_craft.py checks), by numpy"""
    key = (n, salt)
    if key not in _LITS:
        i = np.arange(n, dtype=np.int64)
        _LITS[key] = ((((i * 131 + salt * 29 + 7) ^ (i >> 6) ^ (i >> 11)) & 0xFF).astype(np.uint8)).tobytes()
    return _LITS[key]


def T(k, salt=9):
    """the literals-only last sequence"""
    return (lits(k, salt), None, None)


def size_of(seqs) -> int:
    return sum(len(lit) + (ml or 0) for lit, _, ml in seqs)


def fill(p: int, salt: int):
    """sequences that bring a block from position p to exactly B with bytes
    that are not tainted: literals, or 1,000 literals and a match over them"""
    room = B - p
    assert room == 0 or room >= 5, room
    if room == 0:
        return []
    if room < 1100:
        return [T(room, salt)]
    return [(lits(1000, salt), 1000, room - 1005), T(5, salt)]


def full(seqs, salt: int):
    return list(seqs) + fill(size_of(seqs), salt)


def b0(variant: int, salt: int = 1):
    """block 0: stored, or compressed with matches of its own (its last 12,005
    bytes literals, so the bytes short offsets reach have no period)"""
    if variant == 0:
        return S(lits(B, salt))
    blk = [(lits(3000, salt), 1000, 9000), (lits(2500, salt + 1), 17, 600), (lits(1500, salt + 2), 12345, 30000),
           (b"", 40000, 6931), T(12005, salt + 3)]
    assert size_of(blk) == B
    return blk


def CH(off: int, salt: int):
    """a chain block: one match over all but the last 5 bytes"""
    return [(b"", off, B - 5), T(5, salt)]


RECIPES: dict = {}    # name -> (blocks, accepted, declared dsize | None, frame options), in table order
BLOCKS: dict = {}     # name -> the blocks the frame is built from
_BUILT: dict = {}

A_OFFS = [1, 2, 15, 16, 17, 255, 256, 4096, 65535]
A_MLS = [4, 15, 16, 17, 64, 65, 256, 257, 300, B - 5]
A_K = list(range(1, 18)) + [31, 32, 33]
A_E = [1, 3, 15, 16, 17]
B_PHASES = [0, 1, 15, 16, 30, 31]
B_LENS = [33, 64, 65, 96, 97]
D_COUNTS = [0, 1, 4, 1023, 1024, 1025, 4097, B - 5]
E_BLOCKS = [2, 3, 5, 33, 64]
E_OFFS = [65535, 65531, 32768]


def _add(name, blocks, ok=True, dsize=None, **kw):
    assert name not in RECIPES, name
    RECIPES[name] = (blocks, ok, dsize, kw)
    BLOCKS[name] = blocks
    return name


def case(name):
    """(name, frame bytes, declared dsize, expected bytes | None), as a row of
    lz4_craft.CASES; built when first asked for (expand is byte by byte)"""
    if name not in _BUILT:
        blocks, ok, dsize, kw = RECIPES[name]
        f, out = _build(blocks, independent=False, **kw)
        _BUILT[name] = (name, f, len(out) if dsize is None else dsize, out if ok else None)
    return _BUILT[name]


class _Table:
    """CASES: the whole table in order, each row built on first use (a tool
    that wants five frames does not pay for five hundred)"""

    def __iter__(self):
        return (case(n) for n in RECIPES)

    def __len__(self):
        return len(RECIPES)

    def __getitem__(self, i):
        return [case(n) for n in RECIPES][i]


CASES = _Table()


def tainted_block(n: int, salt: int):
    """a full block with exactly n tainted bytes"""
    if n == 0:
        return full([(lits(300, salt), 100, 500), (lits(20, salt + 1), 1, 100)], salt + 2)
    if n == 1:      # 5 literals, then 1 byte from before the block and 3 of the literals
        return full([(lits(5, salt), 6, 4)], salt + 1)
    if n == 4:
        return full([(b"", 100, 4)], salt)
    if n == B - 5:  # matches of every kind back to back, each from 65,535 back
        mls, left, i = [], B - 5, 0
        cyc = [4, 15, 16, 17, 64, 65, 256, 257, 300, 1031]
        while left:
            m = cyc[i % len(cyc)]
            i += 1
            if left - m < 4:
                m = left
            mls.append(m)
            left -= m
        return [(b"", 65535, m) for m in mls] + [T(5, salt)]
    chunks = [61] * (n // 61) + ([n % 61] if n % 61 else [])
    if chunks[-1] < 4:
        chunks[-2] -= 4 - chunks[-1]
        chunks[-1] = 4
    assert sum(chunks) == n and min(chunks) >= 4
    seqs, p = [], 0
    for i, c in enumerate(chunks):   # 13 literals, then c bytes from before the block
        seqs.append((lits(13, salt + i), p + 13 + 777, c))
        p += 13 + c
    return full(seqs, salt + 1)


def _make_cases():
    salt = [100]

    def s():
        salt[0] += 1
        return salt[0]

    # --- a. where taint enters ---------------------------------------------
    for i, off in enumerate(A_OFFS):
        for j, ml in enumerate(A_MLS):
            _add(f"a_first_off{off}_ml{ml}", [b0((i + j) & 1, s()), full([(b"", off, ml)], s())])
    # k literals, then a match whose source's first e bytes lie before the
    # block: as long as its offset (the longest without overlap), and longer
    n = 0
    for k in A_K:
        for e in A_E:
            off = k + e
            for tag, ml in (("le", off), ("gt", off + 37)):
                if ml >= 4:
                    n += 1
                    _add(f"a_straddle_k{k}_e{e}_{tag}", [b0(n & 1, s()), full([(lits(k, s()), off, ml)], s())])
    # every clip length 1..16 (and 17: a whole piece, then 1) of the piece rule
    # (offset >= 16, length <= 256) and of the lane-per-byte rule (length > 256)
    for e in range(1, 18):
        for ml in (40, 300):
            _add(f"a_clip_e{e}_ml{ml}", [b0(e & 1, s()), full([(lits(20, s()), 20 + e, ml)], s())])
    # both sides of the rule switches, the source before the block and the
    # source tainted bytes of the block
    for off, ml in ((15, 20), (16, 20), (40, 256), (40, 257)):
        _add(f"a_switch_off{off}_ml{ml}_first", [b0(ml & 1, s()), full([(b"", off, ml)], s())])
        _add(f"a_switch_off{off}_ml{ml}_gen2",
             [b0(off & 1, s()), full([(b"", 300, 64), (lits(3, s()), off, ml)], s())])

    # --- b. taint bits against 32-bit words ----------------------------------
    # a tainted match of length L starting at block position x: by pieces (from
    # before the block) and by lanes (offset 7 over 8 tainted bytes)
    def b_blocks(x, L, wide, top):
        at = x - 8 if wide else x       # where the match from before the block starts
        off = 65535 if top else at + 1000
        if top:     # untainted bytes, the last 16 of them literals
            lead = [(lits(1000, s()), 1000, at - 16 - 1000), (lits(16, s()), off, 8 if wide else L)]
        else:
            lead = [(lits(at, s()), off, 8 if wide else L)]
        return lead + ([(b"", 7, L)] if wide else [])

    n = 0
    for r in B_PHASES:
        for L in B_LENS:
            for wide in (False, True):
                n += 1
                _add(f"b_x{r}_len{L}_{'lanes' if wide else 'pieces'}",
                     [b0(n & 1, s()), full(b_blocks(64 + r, L, wide, False), s())])
        # at the top of the block the match ends at B - 5, so the start's
        # phase fixes the length modulo 32: the two lengths in [33, 97]
        for L in [L for L in range(33, 98) if (B - 5 - L) % 32 == r]:
            for wide in (False, True):
                n += 1
                blk = b_blocks(B - 5 - L, L, wide, True) + [T(5, s())]
                assert size_of(blk) == B
                _add(f"b_top_x{r}_len{L}_{'lanes' if wide else 'pieces'}", [b0(n & 1, s()), blk])

    # --- c. later generations inside a block ---------------------------------
    _add("c_full_pieces", [b0(0, s()), full([(b"", 5000, 200), (lits(50, s()), 150, 80)], s())])
    _add("c_full_lanes", [b0(1, s()), full([(b"", 5000, 400), (lits(50, s()), 350, 300)], s())])
    for ph in range(17):
        # bytes [0, 64) tainted, then literals; the source's second 16-byte
        # piece has its first ph bytes tainted
        _add(f"c_t2u_ph{ph}", [b0(ph & 1, s()), full([(b"", 5000, 64), (lits(100, s()), 116 + ph, 48)], s())])
        # literals, then [100, 164) tainted; the source's first piece is
        # untainted, its second has its last 16 - ph bytes tainted
        _add(f"c_u2t_ph{ph}",
             [b0(~ph & 1, s()), full([(lits(100, s()), 5100, 64), (lits(36, s()), 116 + ph, 48)], s())])
        if ph in (0, 1, 8, 15, 16):
            _add(f"c_t2u_lanes_ph{ph}",
                 [b0(ph & 1, s()), full([(b"", 5000, 64), (lits(100, s()), 116 + ph, 300)], s())])
            _add(f"c_u2t_lanes_ph{ph}",
                 [b0(~ph & 1, s()), full([(lits(100, s()), 5100, 64), (lits(36, s()), 116 + ph, 300)], s())])
    # an untainted source next to tainted bytes: the 36 literals after them,
    # the 16 literals before them
    _add("c_abut_after", [b0(0, s()), full([(lits(100, s()), 5100, 64), (lits(36, s()), 36, 36)], s())])
    _add("c_abut_before", [b0(1, s()), full([(lits(100, s()), 5100, 64), (lits(36, s()), 116, 16)], s())])
    for depth in (3, 10):
        _add(f"c_chain_depth{depth}_pieces",
             [b0(0, s()), full([(b"", 5000, 40)] + [(lits(3, s()), 43, 40) for _ in range(depth - 1)], s())])
        _add(f"c_chain_depth{depth}_lanes",
             [b0(1, s()), full([(b"", 5000, 300)] + [(lits(3, s()), 303, 300) for _ in range(depth - 1)], s())])
    _add("c_off3_run_prev", [b0(0, s()), full([(b"", 3, 500)], s())])
    _add("c_off3_run_block", [b0(1, s()), full([(lits(9, s()), 5009, 4), (b"", 3, 500)], s())])

    # --- d. how many bytes are tainted -----------------------------------------
    for v in (0, 1):
        for n in D_COUNTS:
            # (a chain block after it: its bytes hop through this block's
            # origins; after the block with no tainted byte it is the tainted one)
            _add(f"d_tainted{n}_v{v}", [b0(v, s()), tainted_block(n, s()), CH(65535, s())])

    # --- e. hops ------------------------------------------------------------------
    for off in E_OFFS:
        for nb in E_BLOCKS:
            _add(f"e_chain{nb}_off{off}", [S(lits(B, 1))] + [CH(off, k) for k in range(1, nb)])
    for nb in (3, 33):
        _add(f"e_chain{nb}_off65535_v1", [b0(1, s())] + [CH(65535, k) for k in range(1, nb)])
    _add("e_chain_into_stored", [b0(1, s()), CH(65535, 1), CH(65531, 2), S(lits(B, s())), CH(65535, 4),
                                 CH(32768, 5)])
    _add("e_chain_from_gen2", [b0(0, s()), full([(b"", 5000, 40), (lits(3, s()), 43, 40), (lits(3, s()), 43, 40)],
                                                 s()), CH(65535, 2), CH(65535, 3)])
    # 4-byte tainted matches that start at every phase of a 16-byte piece, 60
    # literals apart (a piece with one tainted byte, its first or its last,
    # among them), and two chain blocks whose bytes hop through them
    sparse, p = [], 0
    for i in range(256):
        at = 64 * i + 13 + i % 16
        sparse.append((lits(at - p, s()), at + 4 + i * 37 % 5000, 4))
        p = at + 4
    _add("e_chain_through_sparse", [b0(1, s()), full(sparse, s()), CH(65535, 2), CH(65531, 3)])
    z5 = (bytes(5), None, None)
    _add("e_zeros64", [S(bytes(B))] + [[(b"", 1, B - 5), z5] for _ in range(63)])
    _add("e_zeros5_v1", [[(b"\0", 1, B - 6), z5]] + [[(b"", 1, B - 5), z5] for _ in range(4)])

    # --- f. plan and scratch limits -----------------------------------------------
    # (64 blocks, the most the plan takes: e_chain64_*)
    _add("f_blocks65", [S(lits(B, 1))] + [CH(65535, k) for k in range(1, 64)] + [[(lits(1, 3), 65535, 7), T(5)]])
    last = {1: [T(1)], 4: [T(4)], 5: [T(5)], 12: [(b"", 65535, 7), T(5)], 13: [(lits(1, 3), 65535, 7), T(5)],
            B: CH(65535, 2)}
    for i, (n, blk) in enumerate(last.items()):
        assert size_of(blk) == n
        _add(f"f_last{n}", [b0(i & 1, s()), CH(65535, 1), blk])
    _add("f_last_stored", [b0(0, s()), CH(65535, 1), S(lits(1000, s()))])
    _add("f_last_stored_full", [b0(1, s()), CH(65535, 1), S(lits(B, s()))])
    # 16,380 sequences of 3 bytes: more items than the job's slots hold
    _add("f_dense_before", [b0(0, s()), [(b"", 65535, 4)] * 16380 + [T(16)], CH(65535, 2)])
    _add("f_dense_chain", [b0(1, s()), [(b"", 65535, 4)] + [(b"", 4, 4)] * 16379 + [T(16)], CH(65535, 2)])
    # a middle block one byte short: the blocks after it do not start where
    # the plan put them; one byte over: above the block's capacity
    _add("f_mid_B-1", [b0(0, s()), [(b"", 65535, B - 6), T(5)], CH(65535, 2)])
    _add("f_mid_B+1", [b0(0, s()), [(b"", 65535, B - 5), T(6)], CH(65535, 2)], ok=False)
    _add("f_content_size", [b0(1, s()), CH(65535, 1), CH(65531, 2)], content_size=True)
    _add("f_off0_block2", [b0(0, s()), CH(65535, 1), full([(lits(10, s()), 0, 50), (lits(5, s()), 65535, 100)], s())])

    # --- g. refused frames ----------------------------------------------------------
    head = seq(lits(100, 5), 65535, 1000)
    _add("g_truncated_seq", [b0(0, s()), CH(65535, 1), R(head + raw_seq(0x30, b"", b"abc", b"\x02")), CH(65535, 3)],
         ok=False, dsize=4 * B)
    _add("g_match_ext_cut", [b0(1, s()), CH(65535, 1), R(head + raw_seq(0x0F, b"", b"", b"\x10\x00", b"\xff\xff")),
                             CH(65535, 3)], ok=False, dsize=4 * B)
    _add("g_block_size_over", [b0(0, s()), CH(65535, 1), CH(65535, 2), R(lits(B + 1, s()))], ok=False, dsize=4 * B)


_make_cases()


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
def random_linked(seed: int, n: int):
    """n valid linked frames of 2 to 6 blocks as (frame bytes, expected bytes,
    blocks).  Offsets: half from {1, 2, 15, 16, 17, 65535} and the distance to
    the block start +- {0, 1, 15, 16}, half uniform over the history; lengths
    from lz4_craft's edge lists and uniform up to 3,000.  Valid by
    construction, by random_valid's rules (no offset below the history floor,
    a block ends in 5 literals after a match that ends 5 bytes before its end),
    and every block but the last is filled to exactly B; the last ends
    anywhere.  A tenth of the blocks after the first are stored."""
    rng = np.random.default_rng(seed)
    out = []

    def pick(edges, lo, hi):
        return int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(lo, hi))

    for i in range(n):
        nb = int(rng.choice([2, 2, 3, 3, 4, 6]))
        blocks, total = [], 0
        for b in range(nb):
            end = B if b + 1 < nb else int(rng.choice([40, 4096, B - 1, B])) if rng.random() < 0.5 else \
                int(rng.integers(40, B + 1))
            if b and rng.random() < 0.1:
                blocks.append(S(lits(end, 1000 * i + b)))
                total += end
                continue
            seqs, p, csize = [], 0, 0
            while True:
                lit = pick(LIT_EDGES, 0, 3000)
                ml = pick(ML_EDGES, 4, 3000)
                if csize + lit > 50000:
                    lit = 0
                if total + p + lit == 0:
                    lit = 1 + lit % 3
                hist = min(total + p + lit, 65535)
                d = p + lit                       # distance to the block start
                if rng.random() < 0.5:
                    off = int(rng.choice([1, 2, 15, 16, 17, 65535, d, d + 1, d + 15, d + 16, d + 1, d + 16,
                                          max(d - 1, 1), max(d - 15, 1), max(d - 16, 1)]))
                else:
                    off = int(rng.integers(1, hist + 1))
                off = max(1, min(off, hist))
                if p + lit + ml > end - 30:
                    # the block's last match (it ends 5 bytes before the end)
                    lit = min(lit, 16, end - p - 30)
                    if total + p + lit == 0:
                        lit = 1
                    off = max(1, min(off, total + p + lit, 65535))
                    seqs += [(lits(lit, 7 * i + len(seqs)), off, end - p - lit - 5), T(5, i + b)]
                    break
                seqs.append((lits(lit, 7 * i + len(seqs)), off, ml))
                p += lit + ml
                csize += lit + 6
            assert size_of(seqs) == end
            blocks.append(seqs)
            total += end
        f, want = _build(blocks, independent=False)
        out.append((f, want, blocks))
    return out


# ---------------------------------------------------------------------------
# taint, by its definition
# ---------------------------------------------------------------------------
def taint_stats(blocks):
    """Per block of a linked frame, from the definition alone (seq_exec.hip's
    header comment on seq_exec_blocks_kernel): a byte copied from before its
    block, or from a tainted byte, is tainted, and its origin is the previous
    block's byte it is a copy of.  Byte k of a match at block position mb with
    offset off is a copy of the byte at mb - off + k mod off (an overlapping
    match repeats the off bytes before it).  Literals, stored bytes and the
    zeros of offset 0 are not tainted.

    -> a list, per block a dict:
      tainted   how many of its bytes are tainted
      hops      the longest chain of origins from one of its bytes back to an
                untainted byte (0: no tainted byte)
      gen       the deepest generation: 1 for a byte copied from before the
                block, 1 more for each copy of a tainted byte inside the block
      matches   per tainted match (mb, off, ml, rule, clip): rule "wide"
                (off < 16 or ml > 256: a lane a byte) or "pieces" (16-byte
                pieces); clip: for a match whose source starts e bytes before
                the block and ends inside it, the length 1..16 of the last
                piece before the block start, (e - 1) % 16 + 1, else 0
      origin    per byte its origin position in the previous block (-1:
                untainted)
    """
    res = []
    prev_hops = None
    for blk in blocks:
        if isinstance(blk, (bytes, bytearray)) and not isinstance(blk, R):
            n = len(blk)
            res.append({"tainted": 0, "hops": 0, "gen": 0, "matches": [], "origin": np.full(n, -1, np.int32)})
            prev_hops = np.zeros(n, np.int32)
            continue
        assert not isinstance(blk, R), "raw blocks have no sequences"
        n = size_of(blk)
        origin = np.full(n, -1, np.int32)
        hops = np.zeros(n, np.int32)
        gen = np.zeros(n, np.int32)
        matches = []
        p = 0
        for lit, off, ml in blk:
            p += len(lit)
            if off is None:
                continue
            if off == 0:
                p += ml
                continue
            src = p - off + np.arange(ml) % off
            before = src < 0
            inside = ~before
            dst = np.arange(p, p + ml)
            if before.any():
                o = src[before] + len(prev_hops)
                assert o.min() >= 0, "the history is the previous block"
                origin[dst[before]] = o
                hops[dst[before]] = prev_hops[o] + 1
                gen[dst[before]] = 1
            si = src[inside]
            t = origin[si] >= 0
            origin[dst[inside]] = origin[si]
            hops[dst[inside]] = hops[si]
            gen[dst[inside]] = np.where(t, gen[si] + 1, 0)
            if before.any() or t.any():
                e = off - p
                clip = (e - 1) % 16 + 1 if 0 < e < min(off, ml) else 0
                matches.append((p, off, ml, "wide" if off < 16 or ml > 256 else "pieces", clip))
            p += ml
        res.append({"tainted": int((origin >= 0).sum()), "hops": int(hops.max(initial=0)),
                    "gen": int(gen.max(initial=0)), "matches": matches, "origin": origin})
        prev_hops = hops
    return res


# ---------------------------------------------------------------------------
# the device batch API (needs a GPU)
# ---------------------------------------------------------------------------
def decode(zs, gpu, frames, dsizes, engine):
    """lz4_craft.decode into a buffer prefilled with 0xA5 (a tainted byte that
    is never resolved or never stored cannot pass as a zero) -> (each frame's
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
    out = torch.full((max(int(d[-1]), 1),), SENT, dtype=torch.uint8, device=gpu)
    status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    zs.decode_frames(td, comp, out, status, engine=engine)
    torch.cuda.synchronize()
    o = out.cpu().numpy().tobytes()
    return [o[int(d[i]): int(d[i + 1])] for i in range(n)], status.cpu().tolist()


def first_diff(got: bytes, want: bytes):
    """(how many bytes differ, the first one's block and position in it)"""
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if len(a) != len(b):
        return ("length", len(a), len(b))
    bad = np.nonzero(a != b)[0]
    return (int(bad.size), int(bad[0]) // B, int(bad[0]) % B) if bad.size else None
