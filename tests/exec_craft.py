"""Hand-built frames on the edges of the *execute* kernels' own comparisons.

lz4_craft.py and zstd_craft.py sit on format edges and lz4_linked_craft.py on
seq_exec_blocks_kernel's taint code; the parity suites decode compressor
output (1.7 dependency rounds, ~10 pending matches per batch).  Here the
sequence lists are placed on what the other executes decide:

  seq_exec_kernel<OUTB, SEG>   the wave execute (seq_exec_dev.h): the cut of a
      batch (64 item lanes, OUTB staged bytes, extended pairs kept whole), the
      nb == 0 step of a sequence too long to stage, round 0's pieces and their
      stage-or-HBM choice against `flushed`, the readiness search of the
      dependency rounds, copy_ready's entries, copy_overlap_wave's phases, the
      flush;
  seq_exec_frame_kernel        2,048-item windows, done bits, copy_match's
      branches, literal runs around kFLong, an unstaged literal source;
  seq_exec_big_kernel          the cut at H + kBWin, the 3/4 slide, sources
      around H, the stuck path.

  CONST                 the kernels' constants, read out of the sources
  lanes_of / lanes      item lanes of a sequence list (LZ4 or zstd slot rules)
  wave, frame_model, big_model, stats
                        a plain restatement of what the kernels *decide* (not
                        of how they copy): batches, flushed, early / pending /
                        overlapping matches, rounds, pieces, windows, cuts,
                        slides, depth
  RECIPES, case, zcase  the table: name -> blocks of (literals, offset, match
                        length) sequences; the LZ4 frame, the zstd frame
  random_exec           valid frames with dense in-batch dependencies

The cut and the readiness rule are scripts/exec_model.py's (`batches`,
`exact_rounds`): one definition, used here and by that script.  The table is
built for W = kExecStage (3072: the lean, scan and chunk engines) and W = 4096
(the block route's SEG instantiation and zstd's), from the constants as the
sources have them: a changed constant moves the cases with it.
"""
from __future__ import annotations

import importlib.util
import os
import re
import zlib

import numpy as np

import lz4_craft
import zstd_craft
from lz4_craft import S, _build, seekable  # noqa: F401  (seekable: for the tests)
from lz4_linked_craft import lits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libzseek_amd", "csrc")

_spec = importlib.util.spec_from_file_location("exec_model", os.path.join(ROOT, "scripts", "exec_model.py"))
exec_model = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(exec_model)
batches, exact_rounds = exec_model.batches, exec_model.exact_rounds


# ---------------------------------------------------------------------------
# the kernels' constants
# ---------------------------------------------------------------------------
def _read_const(fname: str, pattern: str) -> int:
    with open(os.path.join(CSRC, fname)) as f:
        m = re.search(pattern, f.read())
    assert m, (fname, pattern)
    return sum(int(x) for x in m.group(1).split("+"))


_EXPR = r"([0-9][0-9 +]*);"
CONST = {
    "kExecStage": _read_const("seq_exec_dev.h", r"constexpr uint32_t kExecStage = " + _EXPR),
    "seg_stage": _read_const("seq_exec_seg.hip", r"seq_exec_kernel<(\d+), true>"),
    "zstd_stage": _read_const("seq_exec.hip", r"seq_exec_kernel<(\d+), false>"),
    "kFT": _read_const("seq_exec.hip", r"constexpr uint32_t kFT = " + _EXPR),
    "kFMax": _read_const("seq_exec.hip", r"constexpr uint32_t kFMax = " + _EXPR),
    "kFCStage": _read_const("seq_exec.hip", r"constexpr uint32_t kFCStage = " + _EXPR),
    "kFLong": _read_const("seq_exec.hip", r"constexpr uint32_t kFLong = " + _EXPR),
    "kBWin": _read_const("seq_exec.hip", r"constexpr uint32_t kBWin = " + _EXPR),
}
W_LZ4, W_SEG, W_ZSTD = CONST["kExecStage"], CONST["seg_stage"], CONST["zstd_stage"]
WS = sorted({W_LZ4, W_SEG, W_ZSTD})
KFT, KFMAX, KFCSTAGE, KFLONG, KBWIN = (CONST[k] for k in ("kFT", "kFMax", "kFCStage", "kFLong", "kBWin"))
WIN_ITEMS = 2 * KFT


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def seqs_of(blocks):
    """blocks (lists of (literals, offset, match length), S stored) -> the
    frame's (literal length, match length, offset) list; a stored block is a
    literal run"""
    out = []
    for b in blocks:
        if isinstance(b, (bytes, bytearray)):
            if len(b):
                out.append((len(b), 0, 0))
        else:
            out += [(len(lit), ml or 0, off or 0) for lit, off, ml in b]
    return out


def lanes(seqs, fmt: str = "lz4", pad: bool | None = None):
    """Item lanes (literal length, match length, offset, first half) of a
    sequence list.  A short item holds lit <= 255, ml <= 258 (zstd: and
    ml == 0 or ml >= 4), off <= 65535; anything else is an extended pair: the
    first half carries the lengths, the second is an empty lane.  pad: a pair
    never starts in slot 63 of a 64-slot group, an empty item goes before it
    (zstd's replay and the LZ4 scan engine; default: zstd only)."""
    pad = fmt == "zstd" if pad is None else pad
    out = []
    for lit, ml, off in seqs:
        ext = lit > 255 or ml > 258 or off > 0xFFFF or (fmt == "zstd" and 0 < ml < 4)
        if ext:
            if pad and len(out) & 63 == 63:
                out.append((0, 0, 0, False))
            out += [(lit, ml, off, True), (0, 0, 0, False)]
        else:
            out.append((lit, ml, off, False))
    return out


def npieces(n: int) -> int:
    return (n + 15) >> 4


def wave(ln, W: int, a0: int = 0):
    """seq_exec_kernel<W> on item lanes, for an output address with
    address & 15 == a0: per batch
      i, j, nb      lanes [i, j); nb = j - i, 0 for the step of a lone lane
                    too long to stage (`long`)
      bstart, end   output range
      flushed       frame bytes below this are in HBM when the batch starts
      matches       per match: lane, mb, me, msrc, need, overlap, early and
                    the round it is copied in (0: round 0)
      pending, rounds, pieces (round 0's whole 16-byte pieces), shorts"""
    out, fc = [], 0
    for i, j, bstart in batches(ln, W, 64):
        tot = sum(x[0] + x[1] for x in ln[i:j])
        flushed = max(16 * fc - a0, 0)
        if tot > W:
            out.append({"i": i, "j": j, "nb": 0, "long": True, "bstart": bstart, "end": bstart + tot,
                        "flushed": flushed, "matches": [], "pending": 0, "rounds": 0, "pieces": 0, "shorts": 0,
                        "lit": ln[i][0], "ml": ln[i][1], "off": ln[i][2]})
            fc = (bstart + tot + a0) >> 4
            continue
        p, ms, pieces, shorts = bstart, [], 0, 0
        for k, (L, M, O, _) in enumerate(ln[i:j]):
            mb = p + L
            if L:
                pieces, shorts = pieces + (npieces(L) if L >= 16 else 0), shorts + (L < 16)
            if M:
                overlap = O < M
                need = mb if overlap else mb - O + M
                early = not overlap and need <= bstart
                if early:
                    pieces, shorts = pieces + (npieces(M) if M >= 16 else 0), shorts + (M < 16)
                ms.append({"lane": k, "mb": mb, "me": mb + M, "msrc": mb - O, "need": need, "overlap": overlap,
                           "early": early, "round": 0})
            p = mb + M
        pend = [m for m in ms if not m["early"]]
        for m, r in zip(pend, exact_rounds([(m["mb"], m["me"], m["msrc"], m["need"]) for m in pend])):
            m["round"] = r
        out.append({"i": i, "j": j, "nb": j - i, "long": False, "bstart": bstart, "end": p, "flushed": flushed,
                    "matches": ms, "pending": len(pend), "rounds": max((m["round"] for m in pend), default=0),
                    "pieces": pieces, "shorts": shorts})
        last = j >= len(ln)
        fc = (p + a0 + 15) >> 4 if last else (p + a0) >> 4
    return out


def depths(ln):
    """match dependency depth per output byte: literals 0, a match one more
    than the deepest of the min(off, ml) bytes it reads from others"""
    total = sum(x[0] + x[1] for x in ln)
    d = np.zeros(total, np.int32)
    p = 0
    for L, M, O, _ in ln:
        p += L
        if M:
            d[p: p + M] = 1 + int(d[p - O: p - O + min(O, M)].max())
            p += M
    return d


def frame_model(ln):
    """seq_exec_frame_kernel: the 2,048-item windows (first item, output
    start) and the frame's match dependency depth"""
    wins, p = [], 0
    for w0 in range(0, len(ln), WIN_ITEMS):
        wins.append((w0, p))
        p += sum(x[0] + x[1] for x in ln[w0: w0 + WIN_ITEMS])
    d = depths(ln)
    return {"windows": wins, "depth": int(d.max(initial=0))}


def big_model(ln):
    """seq_exec_big_kernel: per batch of 2,048 items the window start H, the
    first item w0, the cut item (None: no cut), the decoded end P after it and
    whether the window slid; `stuck`: an item longer than the window"""
    nit, H, P, w0, out = len(ln), 0, 0, 0, []
    while w0 < nit:
        first, op, ci = w0, P, None
        for k in range(w0, min(w0 + WIN_ITEMS, nit)):
            n = ln[k][0] + ln[k][1]
            if n and op + n > H + KBWIN:
                ci, cut_op = k, op
                break
            op += n
        P1 = cut_op if ci is not None else op
        if ci is not None and P1 == H:
            out.append({"H": H, "w0": first, "cut": ci, "P": P1, "slide": False, "stuck": True})
            return {"batches": out, "stuck": True, "slides": sum(b["slide"] for b in out)}
        P = P1
        w0 = ci if ci is not None else w0 + WIN_ITEMS
        slide = (ci is not None or P - H >= KBWIN - KBWIN // 4) and w0 < nit
        out.append({"H": H, "w0": first, "cut": ci, "P": P, "slide": slide, "stuck": False})
        if slide:
            H = P
    return {"batches": out, "stuck": False, "slides": sum(b["slide"] for b in out)}


def lanes_of(name: str, fmt: str = "lz4", pad: bool | None = None):
    return lanes(seqs_of(RECIPES[name][0]), fmt, pad)


def stats(name, W: int | None = None, fmt: str = "lz4", a0: int = 0, pad: bool | None = None):
    """what the model saw of a case (a name of the table, or blocks): the
    wave execute's batches for stage size W (nb, pending, rounds and pieces per
    batch, the nb == 0 steps), the frame kernel's windows and depth (frames up
    to kFMax), the window kernel's batches, cuts and slides (bigger ones)"""
    if isinstance(name, str):
        ln = zlanes_of(name) if name in ZRECIPES else lanes_of(name, fmt, pad)
    else:
        ln = lanes(seqs_of(name), fmt, pad)
    total = sum(x[0] + x[1] for x in ln)
    out = {"lanes": len(ln), "total": total}
    if W is not None:
        b = wave(ln, W, a0)
        out.update(batches=b, nb=[x["nb"] for x in b], pending=[x["pending"] for x in b],
                   rounds=[x["rounds"] for x in b], pieces=[x["pieces"] for x in b],
                   long=sum(x["long"] for x in b))
    if total <= KFMAX:
        out["frame"] = frame_model(ln)
    else:
        out["big"] = big_model(ln)
    return out


def batch_at(st, pos: int):
    """the wave batch that produces output byte pos"""
    return next(b for b in st["batches"] if b["bstart"] <= pos < b["end"])


# ---------------------------------------------------------------------------
# building sequence lists
# ---------------------------------------------------------------------------
_salt = [0]


def _case_salt(name: str):
    _salt[0] = zlib.crc32(name.encode()) % 251


def L(n: int) -> bytes:
    """n literal bytes under the next salt: no two runs of a case alike"""
    _salt[0] = _salt[0] % 255 + 1
    return lits(n, _salt[0])


def T(k: int = 5):
    """the literals-only last sequence"""
    return (L(k), None, None)


class Q:
    """a sequence list under construction, with its output position"""

    def __init__(self, pos: int = 0):
        self.s, self.pos = [], pos

    def add(self, lit, off, ml):
        lit = L(lit) if isinstance(lit, int) else lit
        assert 1 <= off <= self.pos + len(lit), (off, self.pos, len(lit))
        self.s.append((lit, off, ml))
        self.pos += len(lit) + ml
        return self

    def at(self, lit, src: int, ml: int) -> int:
        """literals, then a match that reads from output position src; -> its
        destination"""
        lit = L(lit) if isinstance(lit, int) else lit
        mb = self.pos + len(lit)
        self.add(lit, mb - src, ml)
        return mb

    def shorts(self, lens):
        """short sequences of the given total lengths (8..513), offsets over
        the last 60 bytes and the own literals in turn"""
        for k, n in enumerate(lens):
            lit = min(n - 4, 255, 3 + (k * 5) % 13)
            ml = n - lit
            assert lit >= 1 and 4 <= ml <= 258, n
            mb = self.pos + lit
            self.add(lit, 1 + (k * 7) % min(mb, 60), ml)
        return self

    def hist(self, n: int):
        """n bytes (>= 12) of plain history: literal runs of up to 996 bytes,
        each closed by a 4-byte match"""
        while n:
            k = n - 12 if 1000 < n < 1012 else min(n, 1000)
            self.add(k - 4, 8, 4)
            n -= k
        return self

    def tiny(self, count: int):
        """`count` items of 8 bytes"""
        return self.shorts([8] * count)

    def done(self, k: int = 5):
        return self.s + [T(k)]


def split(n: int, total: int):
    """n lengths that sum to total, alike"""
    return [total // n + (1 if k < total % n else 0) for k in range(n)]


def pre(W: int, short: int = 0) -> Q:
    """a first batch of W - short bytes in one extended item: the next lane
    (more than `short` bytes) starts the batch under test at bstart = W - short"""
    return Q().add(W - short - 4, 8, 4)


RECIPES: dict = {}   # name -> (blocks, aimed stage size | None, frame options)
_BUILT: dict = {}
_ZBUILT: dict = {}


def _add(name, blocks, W=None, **kw):
    assert name not in RECIPES, name
    if blocks and isinstance(blocks[0], tuple):
        blocks = [blocks]
    RECIPES[name] = (blocks, W, kw)
    return name


def case(name):
    """(name, LZ4 frame, decoded size, expected bytes), as a row of
    lz4_craft.CASES; built on first use"""
    if name not in _BUILT:
        blocks, _, kw = RECIPES[name]
        f, out = _build(blocks, **kw)
        _BUILT[name] = (name, f, len(out), out)
    return _BUILT[name]


def zblocks(blocks):
    """the same sequences as zstd blocks: the literals in a raw literal
    section, explicit offsets, a stored block as a raw block"""
    out = []
    for b in blocks:
        if isinstance(b, (bytes, bytearray)):
            out.append(zstd_craft.Raw(bytes(b)))
        else:
            out.append(zstd_craft.Cb(b"".join(s[0] for s in b),
                                     [(len(lit), zstd_craft.O(off), ml) for lit, off, ml in b if off is not None]))
    return out


def zcase(name):
    """(name, zstd frame, decoded size, expected bytes): the case's sequences
    as compressed zstd blocks"""
    if name not in _ZBUILT:
        zb = zblocks(RECIPES[name][0])
        want = zstd_craft.expand([zstd_craft.model(zb)])
        _ZBUILT[name] = (name, zstd_craft.frame(zb), len(want), want)
    return _ZBUILT[name]


class _Table:
    def __init__(self, names, get):
        self.names, self.get = names, get

    def __iter__(self):
        return (self.get(n) for n in self.names())

    def __len__(self):
        return len(self.names())


FOLLOW = (1, 15, 16, 17, 31, 32, 33)
B_OFFS = (1, 2, 3, 7, 15, 16, 17, 31, 1023, 1024, 1025)
CHAIN_DEPTHS = (1, 2, 3, 31, 63)
CHAIN_MLS = (4, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129)
OVL_PEND_OFFS = tuple(range(1, 18)) + (31, 32)
OVL_EDGE_OFFS = (4, 15, 16, 17, 31, 32, 63, 64, 65)
F_ITEMS = (WIN_ITEMS - 1, WIN_ITEMS, WIN_ITEMS + 1, 2 * WIN_ITEMS, 2 * WIN_ITEMS + 1)
F_LITS = (64, 65, KFLONG, KFLONG + 1, 1024, 1025)


def _followers(q: Q, end: int):
    """short matches right after a too-long sequence ending at `end`, their
    sources ending FOLLOW bytes before it: the two chunks the nb == 0 step
    reloads from HBM, and the first byte it does not"""
    for d in FOLLOW:
        q.at(b"", end - d - 8, 8)


def _family_a(W):
    w = f"_w{W}"
    for d in (-1, 0, 1):
        _case_salt(n := f"a_sum{d:+d}{w}")
        _add(n, Q().shorts(split(64, W + d)).done(), W)
    for k in (1, 2, 31, 32, 33, 62, 63):
        _case_salt(n := f"a_over_lane{k}{w}")
        q = Q()
        if k * 513 < W:      # short lanes cannot fill the stage: the lane that does not fit is a pair
            q.tiny(k).add(W - 4, 9, 4)
        else:
            q.shorts(split(k, W - 3)).add(3, 2, 4)
        _add(n, q.tiny(3).done(), W)
    for k in (63, 64, 65, 127, 128, 129):
        _case_salt(n := f"a_items{k}{w}")
        _add(n, Q().tiny(k - 1).done(), W)
    for k in (0, 62, 63):
        _case_salt(n := f"a_pair_lane{k}{w}")
        _add(n, Q().tiny(k).add(300, 7, 4).tiny(3).done(), W)
    _case_salt(n := f"a_pair_unfit{w}")
    _add(n, Q().shorts(split(40, W - 100)).add(300, 7, 4).tiny(3).done(), W)
    _case_salt(n := f"a_pair_unfit_twice{w}")
    _add(n, Q().shorts(split(40, W - 100)).add(300, 7, 4).shorts(split(40, W - 404)).add(300, 7, 300).tiny(3).done(), W)


def _family_b():
    def forms(base, W, first_lit, off, ml, need, again=b""):
        # as the frame's first sequence, followed at once by the short matches
        _case_salt(n := base + "_first")
        q = Q().add(first_lit, off, ml)
        _followers(q, q.pos)
        _add(n, q.tiny(3).done(), W)
        # after history and two batches of 64 tiny items: two of them back to
        # back, then the short matches
        _case_salt(n := base + "_after")
        q = Q().hist(max(need, 12)).tiny(128).add(again, off, ml).add(again, off, ml)
        _followers(q, q.pos)
        _add(n, q.tiny(3).done(), W)

    for W in WS:
        n = W + 1
        forms(f"b_lit{n}", W, n, 9, 4, 12, again=n)
        forms(f"b_apart0_ml{n}", W, n, n, n, n)           # the source ends at the destination
        forms(f"b_apart1_ml{n}", W, n + 1, n + 1, n, n + 1)   # ... one byte before it
    # (5,000 bytes: too long for every stage size)
    for W, ml in [(W, W + 1) for W in WS] + [(None, max(5000, max(WS) + 2))]:
        for off in B_OFFS + (ml - 1,):
            forms(f"b_ovl_ml{ml}_off{off}", W, off, off, ml, off)


def _family_c(W):
    w = f"_w{W}"
    _case_salt(n := f"c_grid{w}")
    q, k = pre(W), 0
    for lit in range(34):
        for ml in range(4, 21):
            q.at(lit, (k * 7) % (W - 64), ml)
            k += 1
    _add(n, q.done(), W)
    _case_salt(n := f"c_pieces256{w}")
    q = pre(W)
    for k in range(64):
        q.at(17, 40 * k, 17)
    _add(n, q.done(), W)
    _case_salt(n := f"c_pieces304{w}")
    q = pre(W)
    for k in range(64):
        q.at(33 if k % 8 < 3 else 17, 40 * k, 33 if k % 8 < 3 else 17)
    _add(n, q.done(), W)
    _case_salt(n := f"c_src_end_bstart{w}")
    q = pre(W)
    for k in range(20):
        ml = 4 + 3 * k
        q.at(5, W - ml, ml)
    _add(n, q.done(), W)
    # ... and ending one byte into the batch: no longer early
    _case_salt(n := f"c_src_end_bstart+1{w}")
    q = pre(W)
    for k in range(20):
        ml = 4 + 3 * k
        q.at(5, W + 1 - ml, ml)
    _add(n, q.done(), W)
    for ml in (4, 15, 16, 17, 40):
        # bstart = W - 9: flushed is W - 16 for a 16-byte-aligned output and
        # within 15 bytes below bstart for any other
        _case_salt(n := f"c_flushed_ml{ml}{w}")
        q = pre(W, 9)
        fl = (W - 9) & ~15
        for k in range(49):
            q.at(6, fl - 32 + k, ml)
        _add(n, q.done(), W)


def _family_d(W):
    w = f"_w{W}"
    for depth in CHAIN_DEPTHS:
        for ml in CHAIN_MLS:
            if ml + 7 + depth * (ml + 1) > W:
                continue
            _case_salt(n := f"d_chain{depth}_ml{ml}{w}")
            q = pre(W)
            src = q.pos                      # lane 0's literals
            q.at(ml + 3, 100, 4)             # (its own match is early)
            for i in range(depth):
                src = q.at(i % 2, src, ml)   # reads the lane before: lane 0's literals, then a destination
            _add(n, q.done(), W)
    for shift, tag in ((0, ""), (-1, "_lo"), (1, "_hi")):
        _case_salt(n := f"d_adj{tag}{w}")
        q = pre(W)
        a = q.at(20, q.pos, 10)              # pending: its own literals
        gap = q.pos                          # = a's end
        b = q.at(12, q.pos, 10)              # 12 literals, then the next pending match
        assert gap == a + 10 and b == gap + 12
        q.at(5, gap + shift, 12)             # [a's end, b's start): ready at once; shifted: waits one round
        _add(n, q.done(), W)
    for k in (2, 3, 10):
        _case_salt(n := f"d_span{k}{w}")
        q = pre(W)
        dst = [q.at(6, q.pos, 6) for _ in range(k)]
        q.at(3, dst[0], dst[-1] + 6 - dst[0])
        _add(n, q.done(), W)
    _case_salt(n := f"d_lowest_only{w}")
    q = pre(W)
    a = q.at(6, q.pos, 6)
    for k in range(5):
        q.at(3, 50 * k, 8)
    q.at(2, a, 6)
    _add(n, q.done(), W)
    _case_salt(n := f"d_fanout{w}")
    q = pre(W)
    src = q.pos
    q.at(200, 10, 4)
    for k in range(63):
        q.at(b"", src + 3 * k, 8)
    _add(n, q.done(), W)
    for off in OVL_PEND_OFFS:
        _case_salt(n := f"d_ovl_pend_off{off}{w}")
        q = pre(W)
        q.at(40, q.pos, 33)
        q.add(b"", off, 100)
        _add(n, q.done(), W)
    _case_salt(n := f"d_same_round{w}")
    q = pre(W)
    q.at(64, 10, 4)
    q.add(b"", 3, 50).add(30, 20, 60)
    for _ in range(3):
        q.at(10, q.pos, 10)
    _add(n, q.done(), W)
    # both sides of `overlap`: a match one byte longer than its offset, and
    # one as long, each over its own literals
    _case_salt(n := f"d_ovl_edge{w}")
    q = pre(W)
    for off in OVL_EDGE_OFFS:
        q.add(off, off, off + 1).add(off, off, off)
    _add(n, q.done(), W)
    for off in range(16, 49):
        _case_salt(n := f"d_ovl_first_off{off}{w}")
        _add(n, pre(W, 5).add(b"", off, 200).tiny(3).done(), W)


def _family_e():
    for k in range(1, 18):
        _case_salt(n := f"e_len{k}")
        _add(n, [T(k)])
    _case_salt(n := "e_mod16")
    q = Q()
    for _ in range(16):
        q.shorts([6] * 63 + [7])
    _add(n, q.done())


def _family_f():
    for k in F_ITEMS:
        _case_salt(n := f"f_items{k}")
        _add(n, Q().tiny(k - 1).done())
    for k in (KFT - 1, WIN_ITEMS - 1):
        _case_salt(n := f"f_pair_at{k}")
        _add(n, Q().tiny(k).add(300, 250, 300).tiny(100).done())
    for k in F_LITS:
        _case_salt(n := f"f_lit{k}")
        _add(n, Q().add(8, 8, 8).add(k, 5, 6).add(k, k, 20).done())
    # many one-byte stored blocks: more compressed bytes than the literal
    # stage holds, for a frame that decodes small
    _case_salt(n := "f_unstaged")
    nb = KFCSTAGE // 5 + 100
    blk = Q().add(300, 100, 40).add(KFLONG + 1, 20, 30).add(70, 9, 9).done()
    _add(n, [S(L(1)) for _ in range(nb)] + [blk, S(L(3))])
    _case_salt(n := "f_apart")
    q = Q().add(16, 8, 4)
    for m in (64, 65, 128, 129):
        q.add(m, m, m).add(2 * m, 2 * m, m)
    _add(n, q.done())
    for ov in (16, 17, 31, 32, 33, 63, 64, 65):
        _case_salt(n := f"f_trail_ov{ov}")
        q = Q()
        for m in (ov + 1, ov + 37, 300):
            q.add(ov, ov, m)
        _add(n, q.done())
    for ov in range(1, 16):
        _case_salt(n := f"f_ovl_ov{ov}")
        e = ov * -(-16 // ov)
        q = Q()
        for m in sorted({4, e - 1, e, e + 1, e + 15, e + 16, e + 17, 300}):
            q.add(ov, ov, m)
        _add(n, q.done())
    _case_salt(n := "f_done_words")
    q = Q().add(512, 8, 4)
    for s in (95, 96, 97):
        for e in (191, 192, 193):
            q.at(3, s, e - s)
    _add(n, q.done())
    _case_salt(n := "f_chain64k")
    k = (KFMAX - 9) // 4 - 1
    _add(n, [(L(4), 4, 4)] + [(b"", 4, 4)] * k + [T(5)])


G_B0 = 1000   # the stored first block


def _g_to(q: Q, target: int):
    """items up to exactly `target`: 500-byte short ones, the last two sized
    to land on it"""
    while target - q.pos > 1012:
        q.add(250, 300, 250)
    r = target - q.pos
    assert r == 0 or r >= 16, r
    if r > 506:
        q.add(250, 300, r - 258 - 250)
        r = target - q.pos
    if r:
        q.add(min(r - 4, 250), 300, r - min(r - 4, 250))
    assert q.pos == target
    return q


def _family_g():
    """the window kernel: ~200 KiB linked frames.  Every block's closing
    5-literal sequence shifts what follows, so positions are found by a trial
    layout: sequences are laid out block by block as they are added."""
    total = 3 * KBWIN + 4000

    class GQ(Q):
        """Q whose positions count the blocks' closing literals: a block is
        closed (5 literals) before the sequence that would not fit"""

        def __init__(self):
            super().__init__(G_B0)
            self.blocks, self.cur, self.room = [S(lits(G_B0, 77))], [], 65536

        def add(self, lit, off, ml):
            lit = L(lit) if isinstance(lit, int) else lit
            n = len(lit) + ml
            if n + 5 > self.room:
                self.close()
            assert 1 <= off <= self.pos + len(lit) and off <= 65535
            self.cur.append((lit, off, ml))
            self.s.append((lit, off, ml))
            self.pos += n
            self.room -= n
            return self

        def close(self, k=5):
            self.cur.append(T(k))
            self.blocks.append(self.cur)
            self.pos += k
            self.cur, self.room = [], 65536

        def finish(self):
            _g_to(self, max(total, self.pos + 600))
            self.close()
            return self.blocks

    def g(name):
        _case_salt(name)
        return GQ()

    # an item ends exactly at H + kBWin (H = 0), and one byte past it
    for d in (0, 1):
        q = g(n := f"g_end_at_win{d:+d}")
        _g_to(q, KBWIN + d - 40).add(20, 300, 20)
        _add(n, q.finish(), independent=False)
    # P - H against 3/4 of the window when the first 2,048 items end (the
    # stored block is a pair: slots 0 and 1)
    for d in (-1, 0, 1):
        q = g(n := f"g_three_quarters{d:+d}")
        q.shorts(split(WIN_ITEMS - 2, KBWIN - KBWIN // 4 + d - G_B0))
        _add(n, q.finish(), independent=False)
    # sources around H after the first slide (H = kBWin: the cut item starts
    # there), and an offset of 65,535 from the window's first byte
    q = g(n := "g_sources_at_h")
    _g_to(q, KBWIN)
    H = q.pos
    q.add(b"", 65535, 40)                 # the cut item: at H, from H - 65,535
    q.at(9, H - 20, 40)                   # straddles H
    q.at(9, H - 40, 40)                   # ends at H
    q.at(9, H, 40)                        # starts at H
    q.at(9, H - 1, 2 * 40)
    _add(n, q.finish(), independent=False)
    # an extended pair across the 2,048-item boundary
    q = g(n := "g_pair_across_items")
    q.tiny(WIN_ITEMS - 3).add(300, 250, 300)
    _add(n, q.finish(), independent=False)
    # an extended pair is the cut item
    q = g(n := "g_pair_is_cut")
    _g_to(q, KBWIN - 100).add(300, 250, 300)
    _add(n, q.finish(), independent=False)


H_SLOTS = (0, 61, 62, 63)


def _family_h():
    """zstd only: matches of 3 and offsets over 65,535 are extended pairs"""
    W = W_ZSTD
    Z = zstd_craft
    for k in H_SLOTS:
        # a pair made by off > 65535 behind a raw block of 65,540 bytes, as
        # s_item_off*; k one-item sequences before it (the raw block is a pair)
        lit = bytearray()
        seqs = []
        for i in range(k):
            lit += lits(3, i)
            seqs.append((3, Z.O(2), 5))
        lit += lits(9, 200)
        seqs += [(1, Z.O(65536 + 8 * k), 9), (1, Z.O(65539), 300), (1, 1, 4)]
        ZRECIPES[f"h_off_pair_after{k}"] = [Z.Raw(Z.lits(65540, 23)), Z.Cb(bytes(lit), seqs)]
    # matches of 3 bytes: a chain of 63 pairs read each other, two batches
    lit = lits(40, 5)
    seqs = [(40, Z.O(40), 3)] + [(0, Z.O(3), 3)] * 62 + [(0, Z.O(1), 3)]
    ZRECIPES["h_ml3_chain"] = [Z.Cb(lit, seqs)]
    # ... and ml 3 as the lane that does not fit
    ZRECIPES["h_ml3_unfit"] = [Z.Cb(lits(W - 4, 6), [(W - 6, Z.O(7), 4), (2, Z.O(5), 3)])]


ZRECIPES: dict = {}   # zstd-only cases: name -> zstd_craft blocks


def _make():
    for W in (W_LZ4, W_SEG):
        _family_a(W)
    _family_b()
    for W in (W_LZ4, W_SEG):
        _family_c(W)
        _family_d(W)
    _family_e()
    _family_f()
    _family_g()
    _family_h()


_make()

NAMES = list(RECIPES)
CASES = _Table(lambda: NAMES, case)
# family h: a, c, d at zstd's stage size and the frame kernel's part of f as
# zstd compressed blocks, and the zstd-only cases
Z_NAMES = [n for n in NAMES if (n[0] in "acd" and RECIPES[n][1] == W_ZSTD) or (n[0] == "f" and n != "f_unstaged")]


def zonly(name):
    if name not in _ZBUILT:
        zb = ZRECIPES[name]
        want = zstd_craft.expand([zstd_craft.model(zb)])
        _ZBUILT[name] = (name, zstd_craft.frame(zb), len(want), want)
    return _ZBUILT[name]


def zget(name):
    return zonly(name) if name in ZRECIPES else zcase(name)


ZALL = Z_NAMES + list(ZRECIPES)
ZCASES = _Table(lambda: ZALL, zget)


def zlanes_of(name):
    """the item lanes of a zstd case, by zstd's slot rules"""
    if name not in ZRECIPES:
        return lanes_of(name, "zstd")
    seqs = []
    for b in zstd_craft.model(ZRECIPES[name]):
        if isinstance(b, bytes):
            seqs.append((len(b), 0, 0))
            continue
        used = 0
        for ll, ofv, ml in b[1]:
            assert ofv > 3 or (ofv == 1 and ll), "explicit offsets (or the last offset again)"
            seqs.append((ll, ml, ofv - 3 if ofv > 3 else seqs[-1][2]))
            used += ll
        if len(b[0]) > used:
            seqs.append((len(b[0]) - used, 0, 0))
    return lanes(seqs, "zstd")


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
def random_seqs(rng, zstd: bool):
    """one frame's sequences: full batches of 64 short items whose offsets
    mostly reach into the last 64 bytes produced, so most matches read bytes
    of their own batch and chains of them form"""
    q = Q()
    n = 64 * int(rng.integers(2, 5)) - 1
    q.add(int(rng.integers(8, 40)), int(rng.integers(1, 8)), int(rng.integers(4, 24)))
    for _ in range(n - 1):
        lit = int(rng.choice([0, 0, 0, 1, 2, 3, 8]))
        ml = int(rng.integers(3 if zstd else 4, 28))
        room = q.pos + lit
        off = int(rng.integers(1, min(room, 64) + 1)) if rng.random() < 0.85 else int(rng.integers(1, room + 1))
        q.add(lit, off, ml)
    return q.done(int(rng.integers(5, 20)))


def random_exec(seed: int, n: int, fmt: str = "lz4"):
    """n valid frames as (frame bytes, expected bytes, sequences); fmt "lz4"
    or "zstd".  At least half of all their batches have >= 20 pending matches
    and >= 4 rounds (test_exec_craft.py holds the seeds in use to that)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        _case_salt(f"random{seed}_{i}")
        seqs = random_seqs(rng, fmt == "zstd")
        if fmt == "zstd":
            zb = zblocks([seqs])
            want = zstd_craft.expand([zstd_craft.model(zb)])
            out.append((zstd_craft.frame(zb), want, seqs))
        else:
            f, want = _build([seqs])
            out.append((f, want, seqs))
    return out
