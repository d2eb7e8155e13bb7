"""Hand-built zstd frames at the edges of the frame, block, literals, Huffman,
FSE and sequence formats (RFC 8878).

Every other zstd frame the suite decodes was written by libzstd's compressor
(or is one of those with a byte flipped), which uses a small part of what the
format allows.  This module writes every field itself, so a case can sit on a
rule of libzstd 1.4.9's decoder: each literals size form, direct and FSE-coded
Huffman weights, the four sequence-table modes and repeat tables, the
repeat-offset rules, the sequence-count forms, the frame-header forms, several
frames in one seek-table entry.

  frame_header, block, skippable     the frame layer, field by field
  lit_raw, lit_rle, lit_huf          literals sections in every size form
  Huf                                weights -> codes, direct / FSE-coded description
  write_ncount, fse_table, fse_chain an FSE description writer and encoder
  seq_section                        sequence count, modes, tables, backward bit stream
  Frame                              a frame from block specs, tracking repeat tables
  expand                             the intended output, byte by byte (the plain model)
  seekable, NEIGHBOURS               frames + a seek table; two intact neighbours
  CASES, PAIRS                       the named table and its accepted / rejected pairs
  random_valid                       edge-biased generator of valid entries

A case's verdict here is written down from the format rules and libzstd
1.4.9's decoder; tests/golden/zstd_craft.json records what libzstd 1.4.9 and
the compiled reference reader make of the same entries (make_zstd_craft.py),
and test_zstd_craft.py holds the table and the oracle to that record.
"""
from __future__ import annotations

import numpy as np
import xxhash

MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 1 << 17

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192,
                             16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099,
                                8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1,
              -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEFAULT = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
MAX_SYM = (35, 31, 52)      # LL, OF, ML
MAX_LOG = (9, 8, 9)


class Invalid(Exception):
    """the model meets something libzstd refuses"""


# ---------------------------------------------------------------------------
# bit streams
# ---------------------------------------------------------------------------
def bits_backward(fields, mark: bool = True) -> bytes:
    """A backward bit stream from its fields in the order the decoder reads
    them, (value, bits) each: the first field sits right below the end mark
    in the last byte."""
    parts = [(1, 1) if mark else (0, 0)]        # (value, bits): small chunks, joined pairwise
    acc = n = 0
    for v, nb in fields:
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0, (v, nb)
        acc = (acc << nb) | v
        n += nb
        if n > 2048:
            parts.append((acc, n))
            acc = n = 0
    parts.append((acc, n))
    while len(parts) > 1:
        parts = [(parts[i][0] << parts[i + 1][1] | parts[i + 1][0], parts[i][1] + parts[i + 1][1])
                 if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0][0].to_bytes((parts[0][1] + 7) // 8, "little")


def bits_forward(fields) -> bytes:
    """a forward (LSB-first) bit stream: FSE descriptions"""
    acc = n = 0
    for v, nb in fields:
        acc |= v << n
        n += nb
    return acc.to_bytes((n + 7) // 8, "little")


# ---------------------------------------------------------------------------
# FSE
# ---------------------------------------------------------------------------
class Tab:
    """an FSE decoding table: per state its symbol, bit count and baseline"""

    def __init__(self, mode, desc, al, sym, nb, base):
        self.mode, self.desc, self.al, self.sym, self.nb, self.base = mode, desc, al, sym, nb, base
        self.states_of = {}
        for s, y in enumerate(sym):
            self.states_of.setdefault(y, []).append(s)


def fse_table(norm, al, mode=2, desc=b"") -> Tab:
    """the decoding table of a normalized distribution (RFC 8878 §4.1.1)"""
    size = 1 << al
    assert sum(abs(p) for p in norm) == size, (sum(abs(p) for p in norm), size)
    sym = [0] * size
    high = size - 1
    nxt = {}
    for s, p in enumerate(norm):
        if p == -1:
            sym[high] = s
            high -= 1
            nxt[s] = 1
        elif p:
            nxt[s] = p
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    nb, base = [0] * size, [0] * size
    for u in range(size):
        x = nxt[sym[u]]
        nxt[sym[u]] += 1
        nb[u] = al - (x.bit_length() - 1)
        base[u] = (x << nb[u]) - size
    return Tab(mode, desc, al, sym, nb, base)


def rle_table(symbol: int, write=None) -> Tab:
    """write: the symbol byte to put in the description instead"""
    return Tab(1, bytes([symbol if write is None else write]), 0, [symbol], [0], [0])


def ncount_fields(norm, al, al_field=None):
    """FSE_writeNCount's fields, (value, bits) each, for a forward stream: 4
    bits of accuracy log - 5, then each count + 1 in the shrinking width, a
    2-bit zero-run chain after every zero count (eight 3s in a row are the
    16-bit 0xFFFF form of 24 zeros)."""
    norm = list(norm)
    while norm and norm[-1] == 0:
        norm.pop()
    f = [((al if al_field is None else al_field) - 5, 4)]
    remaining, threshold, nb = (1 << al) + 1, 1 << al, al + 1
    i, prev0 = 0, False
    while remaining > 1:
        if prev0:
            start = i
            while norm[i] == 0:
                i += 1
            run = i - start
            while run >= 3:
                f.append((3, 2))
                run -= 3
            f.append((run, 2))
        c = norm[i]
        i += 1
        mx = 2 * threshold - 1 - remaining
        remaining -= abs(c)
        v = c + 1
        if v >= threshold:
            v += mx
        f.append((v, nb - (1 if v < mx else 0)))
        prev0 = c == 0
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    assert i == len(norm) and remaining == 1
    return f


def write_ncount(norm, al, al_field=None) -> bytes:
    return bits_forward(ncount_fields(norm, al, al_field))


def fse_chain(tab: Tab, syms, end_bits: bool = False):
    """The states that make `tab` emit `syms` -> (initial state, [(value,
    bits) read after each symbol but the last]).  Found backwards: the states
    of one symbol split [0, size) between their baselines, so the state before
    a given next state is unique.  end_bits: the last state must read bits
    (the Huffman weight walk ends on a read that runs off the stream)."""
    cand = [s for s in tab.states_of[syms[-1]] if tab.nb[s] > 0 or not end_bits]
    assert cand, "no end state that reads bits"
    st, trans = cand[0], []
    for y in reversed(syms[:-1]):
        for s in tab.states_of[y]:
            if tab.base[s] <= st < tab.base[s] + (1 << tab.nb[s]):
                trans.append((st - tab.base[s], tab.nb[s]))
                st = s
                break
        else:
            raise AssertionError("symbol without a state")
    trans.reverse()
    return st, trans


def normalize(counts, al):
    """counts -> a normalized distribution of 1 << al: every present symbol
    at least 1, the rounding remainder on the most frequent"""
    total, size = sum(counts), 1 << al
    norm = [max(1, c * size // total) if c else 0 for c in counts]
    i = max(range(len(norm)), key=lambda k: norm[k])
    norm[i] += size - sum(norm)
    assert norm[i] >= 1
    return norm


def spread_norm(used, al, alphabet, low=()):
    """a distribution over `used` symbols (those in `low` as "less than 1"):
    ones, the rest of the table on the first symbol that is not low"""
    norm = [0] * alphabet
    for s in used:
        norm[s] = -1 if s in low else 1
    rest = (1 << al) - len(set(used))
    first = next(s for s in used if s not in low)
    norm[first] += rest
    assert norm[first] >= 1
    return norm


# ---------------------------------------------------------------------------
# Huffman
# ---------------------------------------------------------------------------
class Huf:
    """Huffman weights (symbol -> 1..log) of a complete code: the codes
    HUF_readDTableX1 assigns, the description (direct nibbles or FSE-coded;
    the last symbol's weight is implied) and the backward streams."""

    def __init__(self, weights: dict):
        self.w = {s: w for s, w in weights.items() if w}
        total = sum(1 << (w - 1) for w in self.w.values())
        self.log = total.bit_length() - 1
        assert 1 << self.log == total, "incomplete code"
        start, rank = 0, {}
        for w in range(1, self.log + 1):
            rank[w] = start
            start += sum(1 for x in self.w.values() if x == w) << (w - 1)
        self.code = {}
        for s in sorted(self.w):
            w = self.w[s]
            self.code[s] = (rank[w] >> (w - 1), self.log + 1 - w)
            rank[w] += 1 << (w - 1)
        self.last = max(self.w)
        self.listed = [self.w.get(s, 0) for s in range(self.last)]

    def desc_direct(self) -> bytes:
        n = len(self.listed)
        assert 1 <= n <= 128
        w = self.listed + [0]
        return bytes([127 + n]) + bytes(w[i] << 4 | w[i + 1] for i in range(0, n, 2))

    def desc_fse(self, al=6, norm=None, one_state=False) -> bytes:
        """the listed weights FSE-coded: two states that take turns, the
        walk ending when a state's read runs off the stream"""
        body = fse_weights(self.listed, al, norm, one_state)
        assert len(body) < 128
        return bytes([len(body)]) + body

    def stream(self, data) -> bytes:
        return bits_backward([self.code[b] for b in data])


def fse_weights(listed, al=6, norm=None, one_state=False) -> bytes:
    n = len(listed)
    assert n >= 2
    if norm is None:
        norm = normalize([listed.count(w) for w in range(13)], al)
    tab = fse_table(norm, al)
    desc = write_ncount(norm, al)
    a, b = listed[0::2], listed[1::2]
    # the second-last weight's state ends on a read past the stream
    ia, ta = fse_chain(tab, a, end_bits=n % 2 == 0)
    ib, tb = fse_chain(tab, b, end_bits=n % 2 == 1)
    fields = [(ia, al), (ib, al)]
    if one_state:       # (the bite check's wrong walk: one state decodes all)
        ia, ta = fse_chain(tab, listed, end_bits=True)
        return desc + bits_backward([(ia, al)] + ta)
    for i in range(n - 2):
        fields.append((ta if i % 2 == 0 else tb)[i // 2])
    return desc + bits_backward(fields)


def flat_weights(symbols) -> dict:
    """a complete code over the symbols with lengths L - 1 and L"""
    s = sorted(set(symbols))
    n = len(s)
    assert n >= 2
    L = (n - 1).bit_length()
    k = (1 << L) - n
    return {y: (2 if i < k else 1) for i, y in enumerate(s)}


def ladder_weights(symbols) -> dict:
    """lengths 1, 2, ..., n - 1, n - 1: every code length present"""
    s = list(symbols)
    n = len(s)
    return {y: max(n - 1 - i, 1) for i, y in enumerate(s)}


# ---------------------------------------------------------------------------
# literals sections
# ---------------------------------------------------------------------------
def _lit_hdr_plain(typ: int, n: int, form=None) -> bytes:
    if form is None:
        form = 1 if n < 32 else 2 if n < 4096 else 3
    if form == 1:
        assert n < 32
        return bytes([typ | n << 3])
    if form == 2:
        assert n < 4096
        return (typ | 1 << 2 | n << 4).to_bytes(2, "little")
    return (typ | 3 << 2 | n << 4).to_bytes(3, "little")


def lit_raw(data: bytes, form=None, size=None) -> bytes:
    return _lit_hdr_plain(0, len(data) if size is None else size, form) + bytes(data)


def lit_rle(byte: int, n: int, form=None) -> bytes:
    return _lit_hdr_plain(1, n, form) + bytes([byte])


def lit_huf_header(typ, streams, regen, comp, form=None) -> bytes:
    if form is None:
        form = 3 if regen < 1024 and comp < 1024 else 4 if regen < 16384 and comp < 16384 else 5
    if form == 3:
        assert regen < 1024 and comp < 1024
        return (typ | (0 if streams == 1 else 1) << 2 | regen << 4 | comp << 14).to_bytes(3, "little")
    assert streams == 4
    if form == 4:
        assert regen < 16384 and comp < 16384
        return (typ | 2 << 2 | regen << 4 | comp << 18).to_bytes(4, "little")
    assert regen < (1 << 18) and comp < (1 << 18)
    return (typ | 3 << 2 | regen << 4 | comp << 22).to_bytes(5, "little")


def huf_streams(huf: Huf, data: bytes, streams: int, jump=None) -> bytes:
    if streams == 1:
        return huf.stream(data)
    seg = (len(data) + 3) // 4
    parts = [huf.stream(data[i * seg: (i + 1) * seg]) for i in range(3)] + [huf.stream(data[3 * seg:])]
    if jump is None:
        jump = [len(p) for p in parts[:3]]
    return b"".join(int(j).to_bytes(2, "little") for j in jump) + b"".join(parts)


def lit_huf(data: bytes, huf: Huf, streams=4, form=None, desc=None, treeless=False, regen=None, jump=None,
            body=None) -> bytes:
    """a Huffman literals section: `desc` the tree description (None: direct
    weights), treeless: none, the previous block's table"""
    if body is None:
        d = b"" if treeless else (huf.desc_direct() if desc is None else desc)
        body = d + huf_streams(huf, data, streams, jump)
    return lit_huf_header(3 if treeless else 2, streams, len(data) if regen is None else regen, len(body),
                          form) + body


# ---------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------
def _code(base, v):
    c = 0
    while c + 1 < len(base) and base[c + 1] <= v:
        c += 1
    return c


def seq_codes(seq):
    """(ll, offset value, ml) -> ((code, extra value, extra bits) x LL, OF, ML)"""
    ll, ofv, ml = seq
    lc, mc, oc = _code(LL_BASE, ll), _code(ML_BASE, ml), ofv.bit_length() - 1
    return ((lc, ll - LL_BASE[lc], LL_BITS[lc]), (oc, ofv - (1 << oc), oc), (mc, ml - ML_BASE[mc], ML_BITS[mc]))


def nseq_bytes(n: int, form=None) -> bytes:
    if form is None:
        form = 1 if n < 128 else 2 if n < 0x7F00 else 3
    if form == 1:
        assert n < 128
        return bytes([n])
    if form == 2:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    return b"\xff" + (n - 0x7F00).to_bytes(2, "little")


PREDEF = None


def predef():
    global PREDEF
    if PREDEF is None:
        PREDEF = [fse_table(LL_DEFAULT, 6, 0), fse_table(OF_DEFAULT, 5, 0), fse_table(ML_DEFAULT, 6, 0)]
    return PREDEF


def seq_stream(seqs, tabs, extra_fields=(), drop_bits=0) -> bytes:
    """the backward bit stream of the sequences under the three tables (LL,
    OF, ML): the initial states, then per sequence the OF, ML, LL extra bits
    and the LL, ML, OF state updates"""
    codes = [seq_codes(s) for s in seqs]
    ch = [fse_chain(tabs[t], [c[t][0] for c in codes]) for t in range(3)]
    fields = [(ch[t][0], tabs[t].al) for t in range(3)]
    for i, c in enumerate(codes):
        fields += [(c[1][1], c[1][2]), (c[2][1], c[2][2]), (c[0][1], c[0][2])]
        if i + 1 < len(codes):
            fields += [ch[0][1][i], ch[2][1][i], ch[1][1][i]]
    fields += list(extra_fields)
    if drop_bits:       # the stream one (or more) bits short: its lowest bits dropped
        total = sum(nb for _, nb in fields)
        acc = 1
        for v, nb in fields:
            acc = (acc << nb) | v
        acc >>= drop_bits
        return acc.to_bytes((total + 1 - drop_bits + 7) // 8, "little")
    return bits_backward(fields)


def seq_read_zero_fill(stream: bytes, tabs, nseq: int):
    """The sequences a decoder reads from `stream` when bits below the
    stream's start read as 0 (the GPU replay's rule; libzstd's is its
    container's): the states' initial values, then per sequence the OF, ML,
    LL extra bits and the LL, ML, OF updates, the last sequence's included."""
    val = int.from_bytes(stream, "little")
    pos = 8 * (len(stream) - 1) + stream[-1].bit_length() - 1

    def rd(nb):
        nonlocal pos
        pos -= nb
        mask = (1 << nb) - 1
        return (val >> pos) & mask if pos >= 0 else (val << -pos) & mask

    st = [rd(t.al) for t in tabs]
    out = []
    for _ in range(nseq):
        lc, oc, mc = (tabs[t].sym[st[t]] for t in range(3))
        ofv = (1 << oc) + rd(oc)
        ml = ML_BASE[mc] + rd(ML_BITS[mc])
        ll = LL_BASE[lc] + rd(LL_BITS[lc])
        out.append((ll, ofv, ml))
        for t in (0, 2, 1):
            st[t] = tabs[t].base[st[t]] + rd(tabs[t].nb[st[t]])
    return out


def seq_section(seqs, tabs, nform=None, nseq=None, reserved=0, stream=None) -> bytes:
    """count, mode byte, table descriptions, bit stream.  tabs: a Tab per LL,
    OF, ML whose mode and description are written as they are."""
    n = len(seqs) if nseq is None else nseq
    out = nseq_bytes(n, nform)
    if n == 0:
        return out
    out += bytes([tabs[0].mode << 6 | tabs[1].mode << 4 | tabs[2].mode << 2 | reserved])
    for t in tabs:
        out += t.desc
    return out + (seq_stream(seqs, tabs) if stream is None else stream)


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------
def frame_header(fcs=None, fcs_bytes=None, single=None, window=None, dict_id=None, dict_bytes=0, checksum=False,
                 reserved=0, unused=0) -> bytes:
    """magic + frame header.  fcs_bytes: 1 (single-segment only), 2 (value -
    256), 4 or 8; None with fcs=None: no content size.  window: the window
    descriptor byte (written when not single-segment)."""
    flag = {None: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    if single is None:
        single = fcs_bytes is not None
    did = {0: 0, 1: 1, 2: 2, 4: 3}[dict_bytes]
    fhd = flag << 6 | (1 if single else 0) << 5 | unused << 4 | reserved << 3 | (1 if checksum else 0) << 2 | did
    # (the table's checksummed frames all come from Frame.build, which records them)
    assert not (checksum and _recording and not _in_build)
    out = MAGIC + bytes([fhd])
    if not single:
        out += bytes([0x50 if window is None else window])
    out += int(dict_id or 0).to_bytes(dict_bytes, "little")
    if fcs_bytes == 1:
        assert single
        out += bytes([fcs])
    elif fcs_bytes == 2:
        out += (fcs - 256).to_bytes(2, "little")
    elif fcs_bytes in (4, 8):
        out += fcs.to_bytes(fcs_bytes, "little")
    return out


def block(typ: int, payload: bytes, last: bool, size=None) -> bytes:
    """a block header (last, type, 21-bit size) and its bytes"""
    size = len(payload) if size is None else size
    return ((1 if last else 0) | typ << 1 | size << 3).to_bytes(3, "little") + bytes(payload)


def skippable(data: bytes = b"", nibble=0, size=None) -> bytes:
    out = (0x184D2A50 | nibble).to_bytes(4, "little") + (len(data) if size is None else size).to_bytes(4, "little") + data
    if _recording and size is None:
        BUILT[out] = None
    return out


def checksum_of(content: bytes) -> bytes:
    return (xxhash.xxh64(content).intdigest() & 0xFFFFFFFF).to_bytes(4, "little")


class Raw(bytes):
    """a raw block"""


class Rle(tuple):
    """an RLE block: (byte, count)"""


class Cb:
    """A compressed block: literal bytes, (ll, offset value, ml) sequences
    and how to write them.
      lit    'raw' | 'rle' | 'huf1' | 'huf4' | 'treeless1' | 'treeless4'
      lform  the literals header's byte count (None: the smallest)
      huf    a Huf (None: flat weights over the literals); hdesc 'direct' | ('fse', al) |
             ('fse', al, 'or direct'): direct where the weights cannot be FSE-coded |
             ('fse', al, norm): under that distribution of the weights
      modes  per LL, OF, ML: 'pre' | ('rle',) | ('fse', al) | ('fse', al, norm) | 'rep'
      nform  the sequence count's byte count
    """

    def __init__(self, lits=b"", seqs=(), lit="raw", lform=None, huf=None, hdesc="direct", modes=("pre",) * 3,
                 nform=None, payload=None):
        self.lits, self.seqs, self.lit, self.lform, self.huf, self.hdesc = bytes(lits), list(seqs), lit, lform, huf, hdesc
        self.modes, self.nform, self.payload = modes, nform, payload


# The builder's record of what it wrote while the table below was made: every
# whole frame -> (its blocks as model() gives them, its checksum flag), every
# whole skippable frame -> None.  _add takes each accepted entry apart into
# these, so RECORDS has the frames, block by block, of all of them.
BUILT: dict = {}
_recording = _in_build = False
# accepted case -> (per frame its blocks, as expand() and items() take them;
# some frame carries the checksum flag)
RECORDS: dict = {}


def _record_of(name, entry):
    """the frames and skippable frames the entry was put together from"""
    frames, cks, p = [], False, 0
    while p < len(entry):
        hit = max((k for k in BUILT if entry.startswith(k, p)), key=len, default=None)
        if hit is None:
            return None
        if BUILT[hit] is not None:
            frames.append(BUILT[hit][0])
            cks = cks or BUILT[hit][1]
        p += len(hit)
    return frames, cks


class Frame:
    """a frame from block specs; keeps the tables a repeat mode or a treeless
    section refers to"""

    def __init__(self):
        self.tabs = [None, None, None]
        self.huf = None

    def literals(self, b: Cb) -> bytes:
        if b.lit == "raw":
            return lit_raw(b.lits, b.lform)
        if b.lit == "rle":
            assert len(set(b.lits)) <= 1
            return lit_rle(b.lits[0] if b.lits else 0x72, len(b.lits), b.lform)
        streams = int(b.lit[-1])
        if b.lit.startswith("treeless"):
            return lit_huf(b.lits, self.huf, streams, b.lform, treeless=True)
        huf = b.huf
        if huf is None:
            sy = set(b.lits)
            if len(sy) < 2:
                sy |= {(min(sy) + 1) & 255}
            n = len(sy)
            if b.hdesc != "direct" and n >= 4 and n & (n - 1) == 0:
                # (equal weights cannot be FSE-coded: three tiers instead)
                huf = Huf({y: 3 if i < n // 4 else 2 if i < n // 2 else 1 for i, y in enumerate(sorted(sy))})
            else:
                huf = Huf(flat_weights(sy))
        self.huf = huf
        desc = None
        if b.hdesc != "direct":
            try:
                given = len(b.hdesc) > 2 and not isinstance(b.hdesc[2], str)
                desc = huf.desc_fse(b.hdesc[1], norm=b.hdesc[2] if given else None)
            except AssertionError:      # weights that FSE cannot end on (all alike) or too few
                if len(b.hdesc) < 3 or given or huf.last > 128:
                    raise
        return lit_huf(b.lits, huf, streams, b.lform, desc)

    def tables(self, b: Cb):
        codes = [seq_codes(s) for s in b.seqs]
        tabs = []
        for t, m in enumerate(b.modes):
            used = sorted({c[t][0] for c in codes})
            if m == "pre":
                tab = predef()[t]
            elif m == "rep":
                p = self.tabs[t]
                tab = Tab(3, b"", p.al, p.sym, p.nb, p.base)
            elif m[0] == "rle":
                assert len(used) == 1
                tab = rle_table(used[0])
            else:
                al = m[1]
                norm = m[2] if len(m) > 2 else spread_norm(used, al, MAX_SYM[t] + 1)
                tab = fse_table(norm, al, 2, write_ncount(norm, al))
            tabs.append(tab)
        return tabs

    def cblock(self, b: Cb) -> bytes:
        if b.payload is not None:
            return b.payload
        lit = self.literals(b)
        if not b.seqs:
            return lit + nseq_bytes(0, b.nform)
        tabs = self.tables(b)
        self.tabs = tabs
        return lit + seq_section(b.seqs, tabs, b.nform)

    def build(self, blocks, last=True, **hdr) -> bytes:
        """blocks: Raw / Rle / Cb.  hdr: frame_header's arguments; fcs=True /
        checksum=True take the model's content."""
        content = None
        if hdr.get("fcs") is True or hdr.get("checksum") is True:
            content = expand([model(blocks)])
        if hdr.get("fcs") is True:
            hdr["fcs"] = len(content)
            if "fcs_bytes" not in hdr:
                n = len(content)
                hdr["fcs_bytes"] = 1 if n < 256 else 2 if n < 65792 else 4
                if hdr["fcs_bytes"] == 1 and hdr.get("single") is False:
                    hdr["fcs_bytes"] = 4        # (the 1-byte form is the single-segment one)
        global _in_build
        _in_build = True
        out = frame_header(**hdr)
        _in_build = False
        for i, b in enumerate(blocks):
            fin = last and i + 1 == len(blocks)
            if isinstance(b, Raw):
                out += block(0, b, fin)
            elif isinstance(b, Rle):
                out += block(1, bytes([b[0]]), fin, size=b[1])
            else:
                out += block(2, self.cblock(b), fin)
        if hdr.get("checksum"):
            out += checksum_of(content)
        if _recording and last:
            BUILT[bytes(out)] = (model(blocks), bool(hdr.get("checksum")))
        return out


def model(blocks):
    """block specs -> the model's view of a frame"""
    return [bytes(b) if isinstance(b, Raw) else bytes([b[0]]) * b[1] if isinstance(b, Rle) else (b.lits, b.seqs)
            for b in blocks]


def frame(blocks, **hdr) -> bytes:
    return Frame().build(blocks, **hdr)


def expand(frames, clamp: bool = True) -> bytes:
    """The model: what an entry decodes to.  frames: per frame a list of
    blocks, each the bytes of a raw / RLE block or (literal bytes, [(ll,
    offset value, ml)]).  Byte-by-byte copies; offset values 1..3 are the
    repeat codes (shifted by one when ll == 0; rep0 - 1 for the fourth,
    0 read as 1), the history is reset at every frame, and a match may not
    start before its own frame's first byte.  Raises Invalid where libzstd
    refuses.  clamp=False leaves rep0 - 1 = 0 as it is (the rule a decoder
    would have without "0 read as 1"): offset 0 is Invalid."""
    out = bytearray()
    for blocks in frames:
        rep = [1, 4, 8]
        start = len(out)
        for b in blocks:
            if isinstance(b, (bytes, bytearray)):
                out += b
                continue
            lits, seqs = b
            lp = 0
            for ll, ofv, ml in seqs:
                if lp + ll > len(lits):
                    raise Invalid("literals run out")
                out += lits[lp: lp + ll]
                lp += ll
                if ofv > 3:
                    off = ofv - 3
                    rep = [off, rep[0], rep[1]]
                else:
                    idx = ofv - 1 + (ll == 0)
                    if idx == 0:
                        off = rep[0]
                    elif idx == 1:
                        off = rep[1]
                        rep = [off, rep[0], rep[2]]
                    else:
                        off = rep[2] if idx == 2 else (rep[0] - 1 or 1) if clamp else rep[0] - 1
                        rep = [off, rep[0], rep[1]]
                if off > len(out) - start or off == 0:
                    raise Invalid("offset before the frame" if off else "offset 0")
                for _ in range(ml):
                    out.append(out[-off])
            out += lits[lp:]
    return bytes(out)


def items(frames, pad_slot: int = 63):
    """The item slots the replay gives an entry (lemit in zstd_seq_dev.h, and
    the wave form's scan): per emit (slot, extended, padded).  One item per
    sequence, per block's literal tail and per raw / RLE block that is not
    empty; two where it is extended (literals > 255, match > 258, a match of
    3, offset > 65535), with a zero item before them where the pair would
    start in slot `pad_slot` of a 64-slot group."""
    k, out = 0, []

    def emit(lit, off, ml):
        nonlocal k
        ext = lit > 255 or ml > 258 or (ml != 0 and ml < 4) or off > 0xFFFF
        pad = ext and (k & 63) == pad_slot
        out.append((k, ext, pad))
        k += (2 + pad) if ext else 1

    for blocks in frames:
        rep = [1, 4, 8]
        for b in blocks:
            if isinstance(b, (bytes, bytearray)):
                if b:
                    emit(len(b), 0, 0)
                continue
            lits_, seqs = b
            used = 0
            for ll, ofv, ml in seqs:
                if ofv > 3:
                    off = ofv - 3
                    rep = [off, rep[0], rep[1]]
                else:
                    idx = ofv - 1 + (ll == 0)
                    if idx == 0:
                        off = rep[0]
                    elif idx == 1:
                        off = rep[1]
                        rep = [off, rep[0], rep[2]]
                    else:
                        off = rep[2] if idx == 2 else (rep[0] - 1 or 1)
                        rep = [off, rep[0], rep[1]]
                emit(ll, off, ml)
                used += ll
            if len(lits_) > used:
                emit(len(lits_) - used, 0, 0)
    return out


def seekable(frames, dsizes) -> bytes:
    """the entries + a seek table (zseek's skippable frame, no checksums)"""
    n = len(frames)
    table = bytearray((0x184D2A5E).to_bytes(4, "little") + (8 * n + 9).to_bytes(4, "little"))
    for f, s in zip(frames, dsizes):
        table += len(f).to_bytes(4, "little") + int(s).to_bytes(4, "little")
    table += n.to_bytes(4, "little") + bytes([0]) + (0x8F92EAB1).to_bytes(4, "little")
    return b"".join(frames) + bytes(table)


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
def lits(n: int, salt: int = 0, alphabet: int = 256) -> bytes:
    """n deterministic bytes without a short period"""
    i = np.arange(n, dtype=np.int64)
    return ((((i * 131 + salt * 29 + 7) ^ (i >> 6) ^ (i >> 11)) & 0xFF) % alphabet).astype(np.uint8).tobytes()


def O(off: int) -> int:
    """an offset as an offset value"""
    return off + 3


CASES: list = []       # (name, entry bytes, d_size, expected bytes | None, libzstd error code)
PAIRS: list = []       # (accepted case, rejected case): the two sides of one boundary
NEIGHBOURS: list = []  # two intact (entry, content) for a case to sit between
ZSK_STATUS_ZSTD = 0x4000000
# Where the GPU decoder departs from libzstd 1.4.9 on purpose (INTEGRATION.md
# §1), under case names that say so: name -> the status it gives.  (Where that
# is 0 and libzstd refuses, the bytes it leaves are not looked at.)
DIVERGENT = {}
# ... and, where that status is 0 and libzstd refuses, the bytes its rule gives
DIVERGENT_BYTES = {}
# name -> the model's frames of the cases built from one (the rules a case sits on
# are looked up here by test_zstd_craft.py)
MODELS = {}
# Where the reader without a cache departs from the reference's, which decodes
# with libzstd's streaming calls up to the entry's d_size:
# name -> (the entry is delivered, the loop's last return value, the error text)
NO_CACHE_DIVERGENT = {
    "h_fcs8_high1": (False, -1, 'decompress user data: Corrupted block detected'),
    "h_window21": (True, 0, ''),
    "h_skippable_past_end": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_skippable_header_cut": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_trailing1": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_trailing2": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_trailing3": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_trailing4": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_trailing5": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_trailing6": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_trailing7": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_trailing8": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_trailing4_magic": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_bad_magic_second": (False, -1, 'decompress user data: Src size is incorrect'),
    "h_checksum_cut1": (False, -1, "decompress user data: Restored data doesn't match checksum"),
    "h_checksum_cut2": (False, -1, "decompress user data: Restored data doesn't match checksum"),
    "h_checksum_cut3": (False, -1, "decompress user data: Restored data doesn't match checksum"),
    "h_checksum_cut4": (False, -1, "decompress user data: Restored data doesn't match checksum"),
    "b_raw200000": (True, 0, ''),
    "b_rle200000": (True, 0, ''),
    "b_rle2097151": (True, 0, ''),
    "b_last_then_more": (False, -1, 'decompress user data: Src size is incorrect'),
    "b_no_last_block": (False, -1, 'decompress user data: Src size is incorrect'),
    "l_raw131072": (False, -1, 'decompress user data: Src size is incorrect'),
    "t_ll_code35_x65535": (True, 0, ''),
    "t_ml_code52_x65535": (True, 0, ''),
    "s_count32511": (True, 0, ''),
    "s_count32512": (True, 0, ''),
    "s_count32812": (True, 0, ''),
    "s_count_says_one_more": (False, -1, 'decompress user data: Destination buffer is too small'),
    "d_size_minus1": (False, -1, 'decompress user data: Destination buffer is too small'),
    "d_size_minus1_raw": (False, -1, 'decompress user data: Destination buffer is too small'),
    "d_size_minus1_match": (False, -1, 'decompress user data: Destination buffer is too small'),
}
# not a libzstd error: it decodes the entry, to fewer bytes than the seek table's d_size
SHORT = -1


def _add(name, entry, want=None, code=0, dsize=None):
    """want: the model's frames (a list per frame) or the expected bytes;
    code != 0: rejected with that libzstd error code"""
    assert all(name != c[0] for c in CASES), name
    if code == 0:
        exp = want if isinstance(want, (bytes, bytearray)) else expand(want)
        if not isinstance(want, (bytes, bytearray)):
            MODELS[name] = want
        CASES.append((name, bytes(entry), len(exp) if dsize is None else dsize, bytes(exp), 0))
        # (a frame put together by hand: the model given for it, block by block; no checksum flag)
        RECORDS[name] = _record_of(name, bytes(entry)) or (want, False)
        assert isinstance(RECORDS[name][0], list), name
    else:
        assert dsize is not None, name
        CASES.append((name, bytes(entry), dsize, None, code))
    return name


def _ok(name, blocks, **hdr):
    """one frame of block specs, accepted"""
    return _add(name, frame(blocks, **hdr), [model(blocks)])


def _bad(name, blocks, code, dsize=64, **hdr):
    return _add(name, frame(blocks, **hdr), None, code, dsize)


def _pair(good, bad):
    PAIRS.append((good, bad))


A = bytes.fromhex("28b52ffd20084100006162636465666768")
B4 = bytes.fromhex("28b52ffd20043d000008780100034e08")
B1 = bytes.fromhex("28b52ffd20043d000008780100004e08")

HEAD = (8, O(8), 5)     # 8 literals, then a match that copies the first 5


def _make_cases():
    L = lits
    # the seed frames below, written out by hand: a raw block; a compressed one with one sequence
    BUILT[A] = ([b"abcdefgh"], False)
    BUILT[B1] = ([(b"x", [(1, O(1), 3)])], False)
    # --- h. entry and frame header ----------------------------------------
    for n, fb in ((0, 1), (255, 1), (256, 2), (65791, 2), (65792, 4)):
        _add(f"h_fcs{n}_in{fb}", frame([Raw(L(n, 1))], fcs=n, fcs_bytes=fb), L(n, 1))
    for n, fb in ((0, 4), (255, 4), (300, 8), (256, 4)):
        _add(f"h_fcs{n}_wide{fb}", frame([Raw(L(n, 2))], fcs=n, fcs_bytes=fb), L(n, 2))
    _pair(_add("h_fcs8_high0", frame([Raw(L(40))], fcs=40, fcs_bytes=8), L(40)),
          _add("h_fcs8_high1", frame([Raw(L(40))], fcs=40 + (1 << 32), fcs_bytes=8), None, 20, 40))
    _pair(_add("h_fcs_right", frame([Raw(L(40))], fcs=40, fcs_bytes=1), L(40)),
          _add("h_fcs_plus1", frame([Raw(L(40))], fcs=41, fcs_bytes=1), None, 20, 40))
    _add("h_fcs_minus1", frame([Raw(L(40))], fcs=39, fcs_bytes=1), None, 20, 40)
    _pair(_add("h_window21", frame([Raw(L(40))], single=False, window=21 << 3), L(40)),
          _add("h_window22", frame([Raw(L(40))], single=False, window=22 << 3), None, 16, 40))
    _add("h_window_fcs", frame([Raw(L(40))], single=False, window=0x0F, fcs=40, fcs_bytes=4), L(40))
    _add("h_window_fcs2", frame([Raw(L(300))], single=False, window=0, fcs=300, fcs_bytes=2), L(300))
    _add("h_reserved_bit", frame([Raw(L(40))], fcs=40, fcs_bytes=1, reserved=1), None, 14, 40)
    _add("h_unused_bit", frame([Raw(L(40))], fcs=40, fcs_bytes=1, unused=1), L(40))
    for w in (1, 2, 4):
        _pair(_add(f"h_dict{w}_zero", frame([Raw(L(40))], fcs=40, fcs_bytes=1, dict_bytes=w), L(40)),
              _add(f"h_dict{w}_nonzero", frame([Raw(L(40))], fcs=40, fcs_bytes=1, dict_bytes=w, dict_id=1 << (8 * w - 1)),
                   None, 32, 40))
    _add("h_empty_frame", frame([Raw(b"")], fcs=0, fcs_bytes=1), b"")
    _add("h_empty_frame_window", frame([Raw(b"")], single=False), b"")
    fr = [frame([Raw(L(20 + i, i))], fcs=True) for i in range(40)]
    co = [L(20 + i, i) for i in range(40)]
    sk = skippable(b"skip me", 3)
    _add("h_2frames", fr[0] + fr[1], co[0] + co[1])
    _add("h_3frames_skips", sk + fr[0] + sk + fr[1] + skippable() + fr[2] + sk, b"".join(co[:3]))
    _add("h_40frames", b"".join(fr), b"".join(co))
    _add("h_40frames_skips", b"".join(f + skippable(bytes(i), i & 15) for i, f in enumerate(fr)), b"".join(co))
    _add("h_skippable_only", sk, b"")
    _add("h_skippable_past_end", fr[0] + skippable(b"abc", size=4), None, 72, 20)
    _add("h_skippable_header_cut", fr[0] + skippable(b"")[:7], None, 72, 20)
    for k in range(1, 9):
        _add(f"h_trailing{k}", fr[0] + bytes(k), None, 72, 20)
    _add("h_trailing4_magic", fr[0] + MAGIC, None, 72, 20)
    _add("h_bad_magic_first", b"\x29" + fr[0][1:], None, 10, 20)
    _add("h_bad_magic_second", fr[0] + b"\x29" + fr[1][1:], None, 72, 41)
    # the seed frames: a match may not reach into the entry's previous frame
    _add("h_seed_A", A, b"abcdefgh")
    _add("h_seed_B1", B1, b"xxxx")
    _pair(_add("h_seed_A+B1", A + B1, b"abcdefghxxxx"), _add("h_seed_A+B4", A + B4, None, 20, 12))
    _add("h_seed_B4", B4, None, 20, 4)
    for ofv in (1, 2, 3):
        for ll in (0, 1):
            blk = [Cb(b"x" * ll + b"yz", [(ll, ofv, 3)])]
            # rep0 = 1 is inside the frame once a literal precedes; 4 and 8 never are
            idx = ofv - 1 + (ll == 0)
            ok = ll == 1 and idx in (0, 3)
            f = frame(blk)
            n = ll + 3 + 2
            if ok:
                _add(f"h_rep_first_ofv{ofv}_ll{ll}", f, [model(blk)])
                _add(f"h_rep_first_ofv{ofv}_ll{ll}_after_A", A + f, b"abcdefgh" + expand([model(blk)]))
            else:
                _add(f"h_rep_first_ofv{ofv}_ll{ll}", f, None, 20, n)
                _add(f"h_rep_first_ofv{ofv}_ll{ll}_after_A", A + f, None, 20, 8 + n)
    # checksums
    body = [Cb(L(30, 3), [HEAD, (3, O(2), 40)])]
    good = frame(body, fcs=True, checksum=True)
    _pair(_add("h_checksum_right", good, [model(body)]),
          _add("h_checksum_wrong", good[:-1] + bytes([good[-1] ^ 1]), None, 22, 75))
    for k in range(1, 5):
        _add(f"h_checksum_cut{k}", good[:-k], None, 22, 75)
    plain = frame(body, fcs=True)
    c1 = expand([model(body)])
    # several checksummed frames in one entry: each is verified over its own bytes
    other = [Cb(L(40, 5), [HEAD, (1, O(9), 33)])]
    good2, c2 = frame(other, checksum=True), expand([model(other)])
    bad1 = good[:-1] + bytes([good[-1] ^ 1])
    _add("h_checksummed_x2", good + good2, c1 + c2)
    _add("h_checksummed_x3", good + sk + good2 + good, c1 + c2 + c1)
    _add("h_checksummed_then_plain", good + plain, c1 * 2)
    _pair("h_checksummed_x2", _add("h_checksummed_x2_first_wrong", bad1 + good2, None, 22, len(c1 + c2)))
    _add("h_checksummed_x2_second_wrong", good2 + bad1, None, 22, len(c1 + c2))
    _add("h_checksummed_x3_middle_wrong", good2 + bad1 + good2, None, 22, len(c2 + c1 + c2))
    _add("h_checksummed_x2_sums_swapped", good[:-4] + good2[-4:] + good2[:-4] + good[-4:], None, 22, len(c1 + c2))
    _add("h_plain_then_checksummed", plain + good, c1 * 2)
    _add("h_checksummed_then_skippables", sk + good + sk + skippable(), c1)
    _add("h_checksummed_then_skippable_wrong", good[:-1] + bytes([good[-1] ^ 4]) + sk, None, 22, 75)
    _add("h_plain_then_checksummed_wrong", plain + good[:-1] + bytes([good[-1] ^ 0x80]), None, 22, 150)

    # --- b. blocks ---------------------------------------------------------
    for n in (0, 1, 131071, 131072):
        _add(f"b_raw{n}", frame([Raw(L(n, 5))]), L(n, 5))
        _add(f"b_rle{n}", frame([Rle((0x41, n))]), b"A" * n)
    _add("b_raw200000", frame([Raw(L(200000, 6))]), L(200000, 6))
    _add("b_rle200000", frame([Rle((0x42, 200000))]), b"B" * 200000)
    _add("b_rle2097151", frame([Rle((0x43, 2097151))]), b"C" * 2097151)
    big = L(131067, 7)      # 3 header bytes + literals + the count byte = 131071
    _pair(_add("b_comp131071", frame([Cb(big)]), big),
          _add("b_comp131072", frame_header() + block(2, lit_raw(big + b"!") + b"\0", True), None, 72, 131068))
    _add("b_type3", frame_header() + block(3, b"abc", True), None, 20, 3)
    _add("b_1000_empty_raw", frame([Raw(b"")] * 1000 + [Raw(L(50, 8))]), L(50, 8))
    _add("b_1000_empty_then_seqs", frame([Raw(b"")] * 1000 + [Cb(L(9, 8), [HEAD])]),
         [[b""] * 1000 + [(L(9, 8), [HEAD])]])
    _add("b_last_then_more", frame([Raw(L(10))]) + block(0, L(5), True), None, 72, 15)
    _add("b_no_last_block", frame([Raw(L(10)), Raw(L(5))], last=False), None, 72, 15)
    _add("b_block_cut", frame([Raw(L(10))])[:-1], None, 72, 10)
    _add("b_raw_rle_comp_mix", *(lambda bl: (frame(bl, fcs=True), [model(bl)]))(
        [Raw(L(33, 1)), Rle((7, 70)), Cb(L(12, 2), [(4, O(100), 30), (0, O(1), 9)]), Rle((9, 1)), Raw(b"z")]))
    _add("b_comp_too_short", frame_header() + block(2, b"\0\0", True), None, 20, 0)

    # --- l. literals -------------------------------------------------------
    for n in (0, 31, 32, 4095, 4096, 131072):
        small = 1 if n < 32 else 2 if n < 4096 else 3
        for form in sorted({small, min(small + 1, 3), 3}):
            tag = "" if form == small else f"_wide{form}"
            if n == 0 and form == 1:
                # the block is 2 bytes, below libzstd's smallest compressed block
                _add("l_raw0", frame([Cb(b"", lform=1)]), None, 20, 0)
            elif n == 131072:
                # 131072 raw literals make a block past the size limit; the most that fit: 131067
                _add(f"l_raw131072{tag}", frame_header() + block(2, lit_raw(L(n, 9)) + b"\0", True), None, 72, n)
                _add(f"l_raw131067{tag}", frame([Cb(L(131067, 9), lform=form)]), L(131067, 9))
            else:
                _add(f"l_raw{n}{tag}", frame([Cb(L(n, 9), lform=form)]), L(n, 9))
            _add(f"l_rle{n}{tag}", frame([Cb(b"r" * n, lit="rle", lform=form)]), b"r" * n)
    _pair("l_rle131072",
          _add("l_rle131073", frame_header() + block(2, lit_rle(0x72, 131073) + b"\0", True), None, 20, 131073))
    _add("l_raw131073", frame_header() + block(2, lit_raw(b"", 3, size=131073) + bytes(100), True), None, 20, 131073)
    _add("l_raw_short", frame_header() + block(2, lit_raw(b"abc", size=9), True), None, 20, 9)
    text = lambda n, s=0: lits(n, s, 23)
    for n in (1, 2, 1023):
        _ok(f"l_huf1_{n}", [Cb(text(n), lit="huf1")])
    for n in (4, 6, 7, 8, 1023, 1024, 16383, 16384, 131072):
        _ok(f"l_huf4_{n}", [Cb(text(n, n), lit="huf4")])
    # 5 symbols: three streams of 2 leave the fourth -1
    _bad("l_huf4_5", [Cb(text(5, 5), lit="huf4")], 20, 5)
    _ok("l_huf4_1023_form4", [Cb(text(1023), lit="huf4", lform=4)])
    _ok("l_huf4_1023_form5", [Cb(text(1023), lit="huf4", lform=5)])
    _ok("l_huf4_16383_form5", [Cb(text(16383), lit="huf4", lform=5)])
    h23 = Huf(flat_weights(range(23)))
    for n in (1, 2, 3):
        d = text(n) + bytes(4 - n)
        sec = lit_huf(d, h23, 4, regen=n)
        _add(f"l_huf4_{n}", frame_header() + block(2, sec + b"\0", True), None, 20, n)
    d = text(40)
    parts = [h23.stream(d[i * 10:(i + 1) * 10]) for i in range(4)]
    sec = lit_huf(d, h23, 4, jump=[len(parts[0]), len(parts[1]), len(parts[2]) + len(parts[3])])
    _add("l_huf4_stream4_empty", frame_header() + block(2, sec + b"\0", True), None, 20, 40)
    sec = lit_huf(d, h23, 4, jump=[len(parts[0]), len(parts[1]), 0x7FFF])
    _add("l_huf4_jump_past_end", frame_header() + block(2, sec + b"\0", True), None, 20, 40)
    sec = lit_huf(d, h23, 1, body=h23.desc_direct() + h23.stream(d) + b"\0")
    _add("l_huf1_last_byte_0", frame_header() + block(2, sec + b"\0", True), None, 20, 40)
    sec = lit_huf(d, h23, 1, body=h23.desc_direct() + h23.stream(d + b"\x01"))
    _add("l_huf1_bits_left_over", frame_header() + block(2, sec + b"\0", True), None, 20, 40)
    sec = lit_huf(d, h23, 1, body=h23.desc_direct() + h23.stream(d[:-1]))
    _add("l_huf1_one_symbol_short", frame_header() + block(2, sec + b"\0", True), None, 20, 40)
    # treeless
    t1, t2, t3 = text(300, 1), text(200, 2), text(500, 3)
    fr_ = Frame()
    fr_.huf = h23
    _add("l_treeless_first_block", fr_.build([Cb(t1, lit="treeless1")]), None, 30, 300)
    _ok("l_treeless_after_huf", [Cb(t1, lit="huf4"), Cb(t2, lit="treeless1"), Cb(t3, lit="treeless4")])
    _ok("l_treeless_after_raw_between", [Cb(t1, lit="huf1"), Cb(L(50)), Raw(L(20)), Rle((1, 9)), Cb(b"q" * 40, lit="rle"),
                                         Cb(t2, lit="treeless4")])
    _ok("l_treeless_after_fse_desc", [Cb(t1, lit="huf4", hdesc=("fse", 6)), Cb(t2, lit="treeless1")])
    two = Frame()
    e = two.build([Cb(t1, lit="huf4")]) + two.build([Cb(t2, lit="treeless1")])
    _add("l_treeless_second_frame", e, None, 30, 500)
    _ok("l_huf_with_seqs", [Cb(text(600, 4), [(100, O(50), 300), (0, 1, 70), (400, O(770), 3)], lit="huf4")])

    # --- w. Huffman descriptions --------------------------------------------
    def hcase(name, weights, data=None, hdesc="direct", ok=True, n=200, code=20):
        h = Huf(weights)
        sy = sorted(h.w)
        data = bytes(sy[(i * 7 + (i >> 3)) % len(sy)] for i in range(n)) if data is None else data
        blk = [Cb(data, lit="huf1" if n < 300 else "huf4", huf=h, hdesc=hdesc)]
        return _ok(name, blk) if ok else _bad(name, blk, code, len(data))

    hcase("w_direct_2sym", {0: 1, 1: 1})
    hcase("w_direct_2sym_far", {0: 1, 128: 1})                       # 128 weights: header byte 255
    hcase("w_direct_odd_count", {i: 1 for i in range(4)})            # 3 listed
    hcase("w_direct_even_count", {0: 2, 1: 2, 2: 1, 3: 1, 4: 1, 5: 1})    # 5 listed... last implied 1
    hcase("w_last_weight_at_log", {0: 1, 1: 1, 2: 2, 3: 3})          # implied last weight = the table log
    hcase("w_log1", {5: 1, 9: 1})
    hcase("w_log6", flat_weights(range(64)))
    hcase("w_log11", ladder_weights(range(12)), n=4000)
    hcase("w_lengths_1_to_11", ladder_weights([3, 9, 1, 200 % 128, 7, 100, 50, 51, 52, 53, 54, 55]), n=3000)
    # table log 12: HUF_readStats allows it, the literals' DTable holds 12
    lad13 = ladder_weights(range(13))
    h12 = Huf(lad13)
    assert h12.log == 12
    hcase("w_log12", lad13, n=5000, ok=False)      # HUF_readStats takes 12, the literals' table 11
    # a weight of 12 (table log 12's 1-bit code) is in w_log12; a listed weight of 13:
    sec = lit_huf(b"ab", Huf({0: 1, 1: 1}), 1, body=bytes([128, 0xD0]) + b"\x05")
    _add("w_weight13", frame_header() + block(2, sec + b"\0", True), None, 20, 2)
    # weights whose total leaves a remainder that is no power of two: 2+2+1 = 5, left 3
    sec = lit_huf(b"ab", Huf({0: 1, 1: 1}), 1, body=bytes([130, 0x22, 0x10]) + b"\x05")
    _add("w_rest_not_pow2", frame_header() + block(2, sec + b"\0", True), None, 20, 2)
    # an odd number of weight-1 symbols: listed 2, 1 -> total 3, rest 1 -> last weight 1: two 1s...  listed 2,2,1: total 5
    sec = lit_huf(b"ab", Huf({0: 1, 1: 1}), 1, body=bytes([130, 0x21, 0x10]) + b"\x05")
    _add("w_odd_weight1_count", frame_header() + block(2, sec + b"\0", True), None, 20, 2)
    # a single listed weight 1: total 1, rest 1: two symbols of weight 1 (accepted: w_direct_2sym);
    # a single weight 2: total 2, rest 2 -> last weight 2, no weight-1 symbol
    sec = lit_huf(b"ab", Huf({0: 1, 1: 1}), 1, body=bytes([128, 0x20]) + b"\x05")
    _add("w_single_weight2", frame_header() + block(2, sec + b"\0", True), None, 20, 2)
    sec = lit_huf(b"ab", Huf({0: 1, 1: 1}), 1, body=bytes([128, 0x00]) + b"\x05")
    _add("w_all_zero_weights", frame_header() + block(2, sec + b"\0", True), None, 20, 2)
    # FSE-coded weights
    hcase("w_fse_al6", flat_weights(range(40)), hdesc=("fse", 6))
    hcase("w_fse_al5", flat_weights(range(40)), hdesc=("fse", 5))
    hcase("w_fse_mixed_weights", ladder_weights(range(0, 90, 9)), hdesc=("fse", 6), n=2000)
    hcase("w_fse_sparse_alphabet", flat_weights(range(0, 256, 5)), hdesc=("fse", 6))
    hcase("w_fse_255_weights", {s: 3 if s < 64 else 2 if s < 128 else 1 for s in range(256)}, hdesc=("fse", 6), n=700)       # every byte value
    hcase("w_fse_255_weights_al5", flat_weights([0, 3, 100, 255]), hdesc=("fse", 5), n=700)
    h40 = Huf(flat_weights(range(40)))
    norm7 = normalize([h40.listed.count(w) for w in range(13)], 7)
    body = bytes([0]) + fse_weights(h40.listed, 7, norm7)
    body = bytes([len(body) - 1]) + body[1:]
    d40 = bytes((i * 7) % 40 for i in range(100))
    sec = lit_huf(d40, h40, 1, body=body + h40.stream(d40))
    _add("w_fse_al7", frame_header() + block(2, sec + b"\0", True), None, 20, 100)
    # an FSE stream that yields 256 weights (255 is the most a table holds)
    sec = lit_huf(d40, h40, 1, body=(lambda b: bytes([len(b)]) + b)(fse_weights([2, 1, 1] * 85 + [2], 6)) + h40.stream(d40))
    _add("w_fse_256_weights", frame_header() + block(2, sec + b"\0", True), None, 20, 100)
    # a description of 127 bytes, the most the header byte can say (128 means one direct
    # weight): 255 weights under a distribution that spends 4 bits on each; the same
    # bytes behind a header byte of 128
    w256 = {s: 3 if s < 64 else 2 if s < 128 else 1 for s in range(256)}
    n127, n126 = [0, 4, 4, 8, 0, 0, 0, 48, 0, 0, 0, 0, 0], [0, 3, 6, 8, 0, 0, 0, 47, 0, 0, 0, 0, 0]
    h256 = Huf(w256)
    assert len(h256.desc_fse(6, norm=n127)) == 128 and len(h256.desc_fse(6, norm=n126)) == 127
    d256 = bytes((i * 7 + (i >> 3)) % 256 for i in range(700))
    for k, nrm in ((127, n127), (126, n126)):
        blk = [Raw(L(5, k)), Cb(d256, lit="huf4", huf=h256, hdesc=("fse", 6, nrm))]
        good = _ok(f"w_fse_desc_{k}_bytes", blk)
    sec = lit_huf(d256, h256, 4, body=b"\x80" + h256.desc_fse(6, norm=n127)[1:] + huf_streams(h256, d256, 4))
    _pair("w_fse_desc_127_bytes",
          _add("w_fse_desc_127_bytes_header_128", frame_header() + block(2, sec + b"\0", True), None, 20, 700))
    # a description written for a walk with one state: the two-state walk reads other weights
    sec = lit_huf(d40, h40, 1, body=h40.desc_fse(6, one_state=True) + h40.stream(d40))
    _add("w_fse_one_state_walk", frame_header() + block(2, sec + b"\0", True), None, 20, 100)
    # the same FSE-coded description at every byte alignment of the block
    for k in range(16):
        blk = [Raw(L(k, k)), Cb(text(300, k), lit="huf4", hdesc=("fse", 6))]
        _add(f"w_fse_align{k}", skippable(bytes(k)) + frame(blk), [model(blk)])

    # --- t. sequence tables --------------------------------------------------
    base = L(64, 11)
    s1 = [(5, O(3), 7), (0, O(10), 4), (2, 1, 9)]
    s2 = [(1, O(20), 5), (3, 2, 11), (0, O(7), 30)]
    mk = {"pre": lambda t: "pre", "rle": lambda t: ("rle",), "fse": lambda t: ("fse", (6, 5, 6)[t])}
    # RLE mode needs one code per table: sequences of one shape
    r1 = [(6, O(5), 6), (6, O(6), 6), (6, O(12), 6)]
    r2 = [(6, O(5), 6), (6, O(7), 6), (6, O(9), 6)]
    for a in ("pre", "rle", "fse", "rep"):
        for b in ("pre", "rle", "fse", "rep"):
            for c in ("pre", "rle", "fse", "rep"):
                first = tuple(mk["fse" if m == "rep" else m](t) for t, m in enumerate((a, b, c)))
                second = tuple("rep" if m == "rep" else mk[m](t) for t, m in enumerate((a, b, c)))
                _ok(f"t_modes_{a}_{b}_{c}", [Cb(base, r1, modes=first), Cb(base, r2, modes=second)])
    for other in ("pre", "rle", "fse"):
        m1 = tuple(mk[other](t) for t in range(3))
        _ok(f"t_rep_after_{other}", [Cb(base, r1, modes=m1), Cb(base, r2, modes=("rep",) * 3),
                                     Raw(b"between"), Cb(base, r1, modes=("rep",) * 3)])
    fz = Frame()        # (made to believe it has tables to repeat)
    fz.tabs = predef()
    for t, nm in enumerate(("ll", "of", "ml")):
        modes = tuple("rep" if i == t else "pre" for i in range(3))
        _add(f"t_rep_first_block_{nm}", fz.build([Cb(base, s1, modes=modes)]), None, 20, 200)
    two = Frame()
    e = two.build([Cb(base, r1, modes=(("fse", 6), ("fse", 5), ("fse", 6)))]) + two.build([Cb(base, r2, modes=("rep",) * 3)])
    _add("t_rep_second_frame", e, None, 20, 200)

    def with_tabs(name, seqs, tabs, ok=True, lit=None, dsize=None):
        lit = L(sum(s[0] for s in seqs) + 3, 12) if lit is None else lit
        if len(lit) > 100000:       # (as raw literals the block would pass its size limit)
            lit = b"\x55" * len(lit)
        payload = (lit_raw(lit) if len(lit) <= 100000 else lit_rle(0x55, len(lit))) + seq_section(seqs, tabs)
        f = frame_header() + block(2, payload, True)
        if ok:
            return _add(name, f, [[(lit, seqs)]])
        return _add(name, f, None, 20, dsize or 64)

    P = predef()
    # RLE mode: the largest legal symbol and one above
    bigll = [(65536 + 5, O(1), 3)]
    with_tabs("t_rle_ll35", bigll, [rle_table(35), P[1], P[2]], lit=L(65536 + 9, 1))
    with_tabs("t_rle_ll36", [(1, O(1), 3)], [rle_table(1, write=36), P[1], P[2]], ok=False)
    with_tabs("t_rle_ml52", [(1, O(1), 65539 + 100)], [P[0], P[1], rle_table(52)])
    with_tabs("t_rle_ml53", [(1, O(1), 3)], [P[0], P[1], rle_table(0, write=53)], ok=False)
    of31 = [(1, (1 << 31) + 5, 3)]
    with_tabs("t_rle_of31_offset_past_output", of31, [P[0], rle_table(31), P[2]], ok=False)
    with_tabs("t_rle_of32", [(1, O(1), 3)], [P[0], rle_table(2, write=32), P[2]], ok=False)
    for c in range(17, 31):
        with_tabs(f"t_rle_of{c}_offset_past_output", [(1, (1 << c) + c, 3)], [P[0], rle_table(c), P[2]], ok=False)

    def fse_tab(norm, al, al_field=None):
        return fse_table(norm, al, 2, write_ncount(norm, al, al_field))

    sq = [(3, O(2), 5), (0, O(3), 4), (3, O(2), 5)]
    for t, nm in enumerate(("ll", "of", "ml")):
        used = sorted({seq_codes(s)[t][0] for s in sq})
        for al in (5, MAX_LOG[t]):
            tabs = list(P)
            tabs[t] = fse_tab(spread_norm(used, al, MAX_SYM[t] + 1), al)
            good = with_tabs(f"t_fse_{nm}_al{al}", sq, tabs)
        al = MAX_LOG[t] + 1
        tabs = list(P)
        tabs[t] = fse_tab(spread_norm(used, al, MAX_SYM[t] + 1), al)
        _pair(good, with_tabs(f"t_fse_{nm}_al{al}", sq, tabs, ok=False))
        # one symbol holds the whole table
        one = [(3, O(2), 5)] * 3
        u = seq_codes(one[0])[t][0]
        tabs = list(P)
        norm = [0] * (u + 1)
        norm[u] = 32
        tabs[t] = fse_tab(norm, 5)
        with_tabs(f"t_fse_{nm}_one_symbol", one, tabs)
        # every symbol "less than 1": 32 symbols of -1
        tabs = list(P)
        tabs[t] = fse_tab([-1] * 32, 5)
        with_tabs(f"t_fse_{nm}_all_low", sq, tabs)
        # a maximum symbol above the alphabet
        tabs = list(P)
        norm = [0] * (MAX_SYM[t] + 2)
        norm[used[0]], norm[-1] = 31, 1
        for x in used[1:]:
            norm[x] = 1
            norm[used[0]] -= 1
        tabs[t] = fse_tab(norm, 5)
        with_tabs(f"t_fse_{nm}_symbol_above_alphabet", sq, tabs, ok=False)
    # zero-run chains: a run of 2 (one 2-bit flag), 3 (a repeat), 30 (the 16-bit form + more)
    for run, sym in ((2, 3), (3, 4), (7, 8), (27, 28), (30, 31), (50, 51)):
        norm = [0] * (sym + 1)
        norm[0], norm[sym] = 63, 1
        with_tabs(f"t_fse_ml_zero_run{run}", [(1, O(1), 3), (0, O(1), ML_BASE[sym]), (1, O(2), 3)], [P[0], P[1], fse_tab(norm, 6)])
    norm = [0] * 36
    norm[0], norm[35] = 31, 1
    with_tabs("t_fse_ll_zero_run34", [(65536, O(9), 3), (0, O(1), 4)], [fse_tab(norm, 5), P[1], P[2]],
              lit=L(65536 + 2, 3))
    # a description that ends one bit short, or lists one symbol too many
    f_ok = ncount_fields([16, 8, 8], 5)
    # a spare bit set after a description's last count, and a description that the block's
    # end cuts (an FSE description has no length of its own: one that is "short" reads on
    # into the bytes that follow)
    tab = fse_table([16, 8, 8], 5, 2, bits_forward(f_ok + [(1, 1)]))
    sq3 = [(1, O(1), 3), (0, O(1), 4), (2, O(2), 3)]
    with_tabs("t_fse_ll_desc_spare_bit_set", sq3, [tab, P[1], P[2]])
    _add("t_fse_ll_desc_cut_by_block_end", frame_header() + block(
        2, lit_raw(L(6)) + nseq_bytes(3) + bytes([2 << 6]) + write_ncount([16, 8, 8], 5)[:1], True), None, 20, 20)
    # every code as a decoded symbol
    lit_big = L(131072, 13)
    for c in range(36):
        for x in sorted({0, (1 << LL_BITS[c]) - 1}):
            ll = LL_BASE[c] + x
            with_tabs(f"t_ll_code{c}_x{x}", [(1, O(1), 3), (ll, O(2), 4)], P, lit=lit_big[: ll + 1])
    for c in range(53):
        for x in sorted({0, (1 << ML_BITS[c]) - 1}):
            with_tabs(f"t_ml_code{c}_x{x}", [(4, O(4), 3), (1, O(2), ML_BASE[c] + x)], P)
    hist = [Raw(L(131072, 14))] * 1
    for c in range(0, 17):
        for x in sorted({0, (1 << c) - 1}):
            ofv = (1 << c) + x
            if ofv < 4:
                continue
            blk = hist + [Cb(b"ab", [(1, ofv, 5)], modes=("pre", ("rle",), "pre"))]
            _add(f"t_of_code{c}_x{x}", frame(blk), [model(blk)])
    # one sequence of the full 89 bits: OF code 31 with LL 35 and ML 52 under 9-, 8-, 9-bit tables
    t89 = [fse_tab(spread_norm([35], 9, 36), 9), fse_tab(spread_norm([31], 8, 32), 8), fse_tab(spread_norm([52], 9, 53), 9)]
    with_tabs("t_89_bit_sequence", [(65536 + 65535, (1 << 31) + (1 << 31) - 1, 65539 + 65535)], t89, ok=False,
              lit=L(131072, 1)[:131071], dsize=131071 + 131074)

    # --- s. sequences ------------------------------------------------------
    def run_of(n, salt=0):
        """n small sequences over a few literals"""
        return [((i + salt) % 3, O(1 + (i * 5 + salt) % 6) if i % 4 else O(2), 3 + (i + salt) % 5) for i in range(n)]

    for n in (0, 1, 63, 64, 65, 127, 128, 129, 0x7EFF, 0x7F00, 0x7F00 + 300):
        sq_ = run_of(n)
        blk = [Cb(b"0123456789" + L(sum(s[0] for s in sq_), 15), [(10, O(10), 3)] + sq_[1:] if n else [])]
        _ok(f"s_count{n}", blk)
    five = run_of(5, 1)
    l5 = b"01234567" + L(20, 16)
    _ok("s_count5_in2", [Cb(l5, [(8, O(8), 3)] + five[1:], nform=2)])
    # (the 3-byte form starts at 0x7F00: 5 cannot be written in it)
    # count 0 in the 2-byte form: libzstd goes on to read a mode byte
    _add("s_count0_in2", frame_header() + block(2, lit_raw(l5) + nseq_bytes(0, 2), True), None, 72, 28)
    # ... and with one (and whatever follows it) takes the block as literals only
    _pair(_add("s_count0_in2_mode_byte", frame_header() + block(2, lit_raw(l5) + nseq_bytes(0, 2) + b"\0junk", True),
                   [[(l5, [])]]),
          "s_count0_in2")
    _add("s_count0_in2_rep_mode", frame_header() + block(2, lit_raw(l5) + nseq_bytes(0, 2) + b"\xfc", True), None, 20, 28)
    pay = lit_raw(l5) + nseq_bytes(0)
    _add("s_count0_then_byte", frame_header() + block(2, pay + b"\0", True), None, 72, 28)
    _add("s_count1_no_stream", frame_header() + block(2, lit_raw(l5) + b"\x01\x00", True), None, 20, 28)
    _add("s_count1_no_mode_byte", frame_header() + block(2, lit_raw(l5) + b"\x01", True), None, 72, 28)
    _add("s_mode_reserved_bits", frame_header() + block(2, lit_raw(l5) + seq_section(five, P, reserved=1), True),
         None, 20, 64)
    sfive = [(8, O(8), 3)] + five[1:]
    want5 = [[(l5, sfive)]]
    n5 = len(expand(want5))
    # libzstd 1.4.9 updates the three states after the last sequence too (a compressor
    # writes no bits for that: the reads run off the stream's start).  Spare bits that
    # this last update takes are not seen; more than it takes are "bits left over"
    _pair(_add("s_stream_spare_bit_in_last_update", frame_header() + block(2, lit_raw(l5) + seq_section(
        sfive, P, stream=seq_stream(sfive, P, extra_fields=[(0, 1)])), True), want5),
        _add("s_stream_4bytes_left_over", frame_header() + block(2, lit_raw(l5) + seq_section(
            sfive, P, stream=b"\x5a\x5a\x5a\x5a" + seq_stream(sfive, P)), True), None, 20, n5))
    # bits below the stream's start read as 0 in the last sequence: its LL extra bit
    # (17 = 16 + 1) is the stream's lowest and comes back 0
    s17 = sfive[:-1] + [(17, O(3), 4)]
    l17 = l5 + L(17, 4)
    _add("s_stream_1bit_short_reads_0", frame_header() + block(2, lit_raw(l17) + seq_section(
        s17, P, stream=seq_stream(s17, P, drop_bits=1)), True), [[(l17, sfive[:-1] + [(16, O(3), 4)])]])
    # (further below its start libzstd reads bits of its 64-bit container again, the GPU zeros)
    DIVERGENT["s_stream_24bits_short_libzstd_refuses_gpu_reads_zeros"] = 0
    DIVERGENT_BYTES["s_stream_24bits_short_libzstd_refuses_gpu_reads_zeros"] = expand(
        [[(l17, seq_read_zero_fill(seq_stream(s17, P, drop_bits=24), P, len(s17)))]])
    assert len(DIVERGENT_BYTES["s_stream_24bits_short_libzstd_refuses_gpu_reads_zeros"]) == n5 + 17
    _add("s_stream_24bits_short_libzstd_refuses_gpu_reads_zeros", frame_header() + block(2, lit_raw(l17) + seq_section(
        s17, P, stream=seq_stream(s17, P, drop_bits=24)), True), None, 20, n5 + 17)
    _add("s_stream_last_byte_0", frame_header() + block(2, lit_raw(l5) + seq_section(
        sfive, P, stream=seq_stream(sfive, P) + b"\0"), True), None, 20, n5)
    _add("s_count_says_one_more", frame_header() + block(2, lit_raw(l5) + seq_section(
        sfive, P, nseq=6), True), None, 70, n5)
    # repeat offsets: every index form, ll = 0 and ll > 0
    pre3 = [(6, O(5), 4), (1, O(3), 3), (1, O(6), 5)]      # history 6, 3, 5
    for ofv in (1, 2, 3):
        for ll in (0, 2):
            sq_ = pre3 + [(ll, ofv, 6), (1, 1, 4), (0, 1, 3), (0, 3, 5)]
            _ok(f"s_rep_ofv{ofv}_ll{ll}", [Cb(L(40, 17), sq_)])
    # rep0 - 1 reaching 0 (read as 1) in the sequences at + 1 and at + 2: a batch's first,
    # middle and last lane (at 62 and 126: lanes 63 and 0)
    for at in (0, 1, 31, 62, 63, 64, 65, 126, 127, 128):
        sq_ = [(2, O(1), 3)] + [(1, 1, 3)] * at
        sq_[-1] = (sq_[-1][0], O(1), 3)
        sq_ += [(0, 3, 7), (0, 3, 4), (1, 2, 3), (0, 1, 3)]
        _ok(f"s_rep0_minus1_is_0_at{at}", [Cb(L(len(sq_) + 4, 18), sq_)])
    # chains of consecutive repeat codes of mixed index across batch boundaries
    for n in (70, 130, 200):
        sq_ = [(9, O(7), 3), (1, O(2), 3), (1, O(4), 3)]
        sq_ += [((i * 7 + (i >> 2)) % 3 == 0 and 1 or 0, 1 + (i * 5 + (i >> 3)) % 3, 3 + i % 3) for i in range(n)]
        _ok(f"s_rep_chain{n}", [Cb(L(20 + n, 19), sq_)])
    # history across blocks, across a raw block, reset at a frame start
    b1 = Cb(L(12, 20), [(8, O(7), 4), (1, O(2), 3), (1, O(5), 3)])
    b2 = Cb(L(6, 21), [(1, 2, 4), (0, 2, 3), (1, 1, 5), (0, 3, 3)])
    _ok("s_rep_across_blocks", [b1, b2])
    _ok("s_rep_across_raw_block", [b1, Raw(L(9, 1)), Rle((3, 4)), b2])
    _ok("s_rep_across_literals_only_block", [b1, Cb(L(9, 1)), b2])
    f1, f2 = frame([b1]), frame([Cb(L(6, 21), [(4, 2, 4)])])      # rep1 = 4 after the reset, 7 if carried
    _add("s_rep_reset_at_frame", f1 + f2, [model([b1]), [(L(6, 21), [(4, 2, 4)])]])
    _add("s_rep_reset_at_frame_rep2", f1 + frame([Cb(L(9, 21), [(8, 3, 4)])]), [model([b1]), [(L(9, 21), [(8, 3, 4)])]])
    # items: short / extended boundaries
    for ll in (255, 256):
        for ml in (3, 258, 259):
            _ok(f"s_item_ll{ll}_ml{ml}", [Cb(L(ll + 300, 22), [(ll, O(200), ml), (0, O(1), 3)])])
    h64 = Raw(L(65540, 23))
    for off in (65535, 65536):
        _ok(f"s_item_off{off}", [h64, Cb(b"abc", [(1, O(off), 9), (1, 1, 4)])])
    # an extended pair on item slot 62, 63, 64 of a 64-slot group (and 126..128): the
    # fillers are one item each (a match of 3 would take two), see items()
    for slot in (61, 62, 63, 64, 65, 126, 127, 128):
        fill = [(1, O(1), 4)] * slot
        for kind, sq_, nl in (("pair", [(1, O(2), 300), (0, O(3), 5), (2, O(1), 259), (1, 1, 4)], 10),
                              ("ll", [(300, O(2), 4), (0, O(3), 5)], 310),
                              ("ml3", [(1, O(2), 3), (1, O(1), 5), (0, 2, 3)], 10)):
            name = _ok(f"s_ext_{kind}_at_slot{slot}", [Cb(L(slot + nl, 24), fill + sq_)])
            first = [i for i in items(MODELS[name]) if i[1]][0]
            assert first[0] == slot and first[2] == (slot & 63 == 63), name
    # errors
    lit10 = L(10, 26)
    e1 = [(4, O(4), 5), (7, O(2), 3)]
    _add("s_literals_run_out", frame_header() + block(2, lit_raw(lit10) + seq_section(e1, P), True), None, 20, 19)
    ok1 = [(4, O(4), 5), (6, O(2), 3)]
    good = _add("s_literals_exact", frame_header() + block(2, lit_raw(lit10) + seq_section(ok1, P), True), [[(lit10, ok1)]])
    _pair(good, "s_literals_run_out")
    _ok("s_literals_left_over", [Cb(lit10, [(4, O(4), 5), (1, O(2), 3)])])
    _pair(_ok("s_offset_eq_produced", [Cb(lit10, [(4, O(4), 5), (1, O(10), 3)])]),
          _add("s_offset_produced_plus1", frame([Cb(lit10, [(4, O(4), 5), (1, O(11), 3)])]), None, 20, 18))
    _pair(_ok("s_offset_eq_produced_block2", [Raw(b"0123"), Cb(lit10, [(4, O(8), 5)])]),
          _add("s_offset_produced_plus1_block2", frame([Raw(b"0123"), Cb(lit10, [(4, O(9), 5)])]), None, 20, 19))
    _pair(_add("s_offset_eq_produced_frame2", A + frame([Cb(lit10, [(4, O(4), 5)])]), b"abcdefgh" + expand([[(lit10, [(4, O(4), 5)])]])),
          _add("s_offset_produced_plus1_frame2", A + frame([Cb(lit10, [(4, O(5), 5)])]), None, 20, 23))
    _add("s_offset_whole_prev_frame", A + frame([Cb(lit10, [(4, O(12), 5)])]), None, 20, 23)

    # the entry's d_size against what it decodes to
    okf = frame([Cb(lit10, ok1)])
    _add("d_size_minus1", okf, None, 70, 17)
    _add("d_size_minus1_raw", frame([Raw(L(30))]), None, 70, 29)
    _add("d_size_minus1_match", frame([Cb(lit10, [(10, O(4), 5)])]), None, 70, 14)
    _add("d_size_plus1", okf, None, SHORT, 19)
    _add("d_size_plus1_raw", frame([Raw(L(30))]), None, SHORT, 31)
    _add("d_size_plus1_two_frames", A + okf, None, SHORT, 27)

    NEIGHBOURS.append((frame([Cb(lits(300, 11, 60), [(100, O(17), 40), (3, O(130), 500), (0, 1, 12)], lit="huf4")], fcs=True),
                       expand([[(lits(300, 11, 60), [(100, O(17), 40), (3, O(130), 500), (0, 1, 12)])]])))
    nb = [Cb(L(20, 12), [HEAD, (2, 1, 90)]), Raw(L(33, 13))]
    NEIGHBOURS.append((frame(nb, single=False, checksum=True), expand([model(nb)])))


_recording = True
_make_cases()
_recording = False
CASE = {c[0]: c for c in CASES}


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
LL_EDGES = [0, 1, 15, 16, 17, 63, 64, 255, 256]
ML_EDGES = [3, 4, 34, 35, 36, 130, 131, 258, 259]
OFF_EDGES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 255, 256, 257]


def random_valid(seed: int, n: int):
    """n valid entries of at most 4 KiB decoded, as (entry bytes, expected
    bytes): one to three frames (skippable frames among them), each of one to
    four blocks (raw, RLE, compressed) with a random choice in every field:
    header form, checksum, literals type and size form, direct or FSE-coded
    weights, table modes (repeat where a table exists), count form, repeat
    codes and edge-biased lengths and offsets.  Valid by construction: an
    offset never reaches before its frame."""
    rng = np.random.default_rng(seed)
    out = []

    def pick(edges, lo, hi):
        return int(rng.choice(edges)) if rng.random() < 0.4 else int(rng.integers(lo, hi))

    for i in range(n):
        entry, frames_model = b"", []
        budget = int(rng.choice([40, 300, 1500, 4000]))
        for _ in range(int(rng.choice([1, 1, 1, 2, 3]))):
            if rng.random() < 0.15:
                entry += skippable(bytes(int(rng.integers(0, 9))), int(rng.integers(0, 16)))
            F = Frame()
            blocks, produced, rep, have_tabs, have_huf = [], 0, [1, 4, 8], False, False
            for _ in range(int(rng.choice([1, 1, 2, 3, 4]))):
                room = budget - sum(len(x) for x in map(lambda m: expand([m]), frames_model)) - produced
                kind = rng.random()
                if kind < 0.15 or room < 12:
                    m = min(int(rng.integers(0, 40)), max(room, 0))
                    blocks.append(Raw(lits(m, i)))
                    produced += m
                    continue
                if kind < 0.25:
                    m = min(int(rng.integers(0, 60)), room)
                    blocks.append(Rle((int(rng.integers(0, 256)), m)))
                    produced += m
                    continue
                seqs, nlit, op = [], 0, produced
                for _ in range(int(rng.choice([0, 1, 2, 5, 20, 70, 130]))):
                    ll, ml = pick(LL_EDGES, 0, 20), pick(ML_EDGES, 3, 30)
                    if op + ll + ml - produced + 4 > room:
                        ll, ml = ll % 3, 3 + ml % 4
                        if op + ll + ml - produced + 4 > room:
                            break
                    if op + ll == 0:
                        ll = 1 + ll % 3
                    reach = op + ll
                    # a repeat code whose offset is inside the frame, or a new offset
                    ofv = None
                    if rng.random() < 0.4:
                        v = int(rng.integers(1, 4))
                        idx = v - 1 + (ll == 0)
                        o = [rep[0], rep[1], rep[2], rep[0] - 1 or 1][idx]
                        if o <= reach:
                            ofv = v
                    if ofv is None:
                        o = min(pick(OFF_EDGES, 1, reach + 1), reach)
                        if rng.random() < 0.1:
                            o = reach
                        ofv = o + 3
                        idx = -1
                    if idx == -1 or idx >= 2:
                        rep = [o, rep[0], rep[1]]
                    elif idx == 1:
                        rep = [o, rep[0], rep[2]]
                    seqs.append((ll, ofv, ml))
                    nlit += ll
                    op += ll + ml
                tail = min(int(rng.choice([0, 0, 1, 5, 40])), max(room - (op - produced), 0))
                nlit += tail
                alphabet = int(rng.choice([1, 2, 5, 23, 200, 256]))
                data = lits(nlit, i * 7 + len(blocks), alphabet)
                # literals
                lk = rng.random()
                if alphabet == 1 and nlit:
                    lit = "rle"
                elif nlit >= 8 and lk < 0.5:
                    lit = "huf4" if rng.random() < 0.6 or nlit >= 800 else "huf1"
                    if have_huf and set(data) <= set(F.huf.w) and rng.random() < 0.4:
                        lit = "treeless" + lit[-1]
                elif nlit >= 1 and nlit < 800 and lk < 0.6:
                    lit = "huf1"
                else:
                    lit = "raw"
                lform = None
                if lit in ("raw", "rle"):
                    lform = int(rng.choice([f for f in (1, 2, 3) if nlit < (32, 4096, 1 << 20)[f - 1]]))
                    if nlit == 0 and not seqs:
                        lform = int(rng.choice([2, 3]))     # (a 2-byte block is below libzstd's minimum)
                elif lit[-1] == "4":
                    lform = [None, 4, 5][int(rng.integers(0, 3))]
                hdesc = "direct"
                if lit.startswith("huf"):
                    have_huf = True
                    if max(set(data) | {(min(data) + 1) & 255} if len(set(data)) < 2 else set(data)) > 128 or rng.random() < 0.4:
                        hdesc = ("fse", int(rng.choice([5, 6])), "or direct")
                # table modes
                modes = []
                codes = [seq_codes(s) for s in seqs]
                for t in range(3):
                    used = {c[t][0] for c in codes}
                    opts = [("fse", int(rng.integers(5, MAX_LOG[t] + 1)))]
                    dflt = (LL_DEFAULT, OF_DEFAULT, ML_DEFAULT)[t]
                    if all(u < len(dflt) for u in used):
                        opts += ["pre", "pre"]
                    if len(used) == 1:
                        opts.append(("rle",))
                    if have_tabs and used <= set(F.tabs[t].sym):
                        opts.append("rep")
                    m = opts[int(rng.integers(0, len(opts)))]
                    if m != "pre" and m != "rep" and m[0] == "fse" and (1 << m[1]) < len(used):
                        m = ("fse", MAX_LOG[t])
                    modes.append(m)
                nform = int(rng.choice([1, 2] if len(seqs) < 128 else [2])) if seqs else None
                b = Cb(data, seqs, lit=lit, lform=lform, hdesc=hdesc, modes=tuple(modes), nform=nform)
                blocks.append(b)
                if seqs:
                    have_tabs = True
                produced = op + tail
                F.cblock(b)     # (leaves the tables the next block's choices look at)
            hdr = {}
            hk = rng.random()
            if hk < 0.5:
                hdr["fcs"] = True
                if rng.random() < 0.3:
                    hdr["fcs_bytes"] = int(rng.choice([4, 8]))
            if hk >= 0.4:
                hdr["single"] = False
                hdr["window"] = int(rng.integers(0, 22 * 8))
            if "fcs" not in hdr and hdr.get("single", True):
                hdr["fcs"] = True
            hdr["dict_bytes"] = int(rng.choice([0, 0, 0, 1, 2, 4]))
            if rng.random() < 0.3:
                hdr["checksum"] = True
            entry += Frame().build(blocks, **hdr)
            frames_model.append(model(blocks))
        if rng.random() < 0.1:
            entry += skippable(b"tail")
        out.append((entry, expand(frames_model)))
    return out


# ---------------------------------------------------------------------------
# the device batch API (needs a GPU)
# ---------------------------------------------------------------------------
def decode(zs, gpu, entries, dsizes, fill=0):
    """entries back to back through zsk_zstd_decode_frames -> (each entry's
    output slot, statuses)"""
    import torch
    n = len(entries)
    c = np.cumsum([0] + [len(f) for f in entries])
    d = np.cumsum([0] + list(dsizes))
    desc = np.zeros(n, zs.FRAME_DESC_DTYPE)
    desc["c_off"], desc["d_off"] = c[:-1], d[:-1]
    desc["c_size"], desc["d_size"] = np.diff(c), np.asarray(dsizes)
    td = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    comp = torch.zeros(int(c[-1]) + 256, dtype=torch.uint8, device=gpu)
    comp[: int(c[-1])].copy_(torch.from_numpy(np.frombuffer(b"".join(entries), np.uint8).copy()))
    out = torch.full((max(int(d[-1]), 1),), fill, dtype=torch.uint8, device=gpu)
    status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    zs.zstd_decode_frames(td, comp, out, status)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return [o[int(d[i]): int(d[i + 1])].tobytes() for i in range(n)], status.cpu().tolist()
