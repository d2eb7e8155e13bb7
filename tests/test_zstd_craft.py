"""tests/zstd_craft.py's hand-built zstd entries on the CPU: the table's own
verdicts and expected bytes (expand, a byte-by-byte model), the oracle
(oracle/zstd_oracle.c) and the record of libzstd 1.4.9 and the compiled
reference reader (tests/golden/zstd_craft.json, made by make_zstd_craft.py)
must all say the same about every entry.  The GPU decoder is held to the same
table in test_gpu_zstd_craft.py."""
from __future__ import annotations

import importlib.util
import json
import os

import numpy as np
import pytest

import zstd_craft
from conftest import GOLDEN, sha
from zstd_craft import SHORT

CASES = zstd_craft.CASES


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_zstd_craft", os.path.join(GOLDEN, "make_zstd_craft.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def record(maker):
    with open(os.path.join(GOLDEN, "zstd_craft.json")) as f:
        meta = json.load(f)
    rec = maker.unpack(meta)
    assert [c["name"] for c in rec] == [c[0] for c in CASES], "regenerate zstd_craft.json"
    assert [c["entry_sha"] for c in rec] == [sha(c[1]) for c in CASES], "regenerate zstd_craft.json"
    assert [c["dsize"] for c in rec] == [c[2] for c in CASES], "regenerate zstd_craft.json"
    assert meta["neighbour_entry_shas"] == [sha(e) for e, _ in zstd_craft.NEIGHBOURS]
    assert meta["libzstd"] == 10409
    return rec


def test_table_shape():
    """578 cases: 451 accepted, 124 rejected with a libzstd error code, 3
    that decode short of their declared size; every boundary pair has its
    accepted and its rejected member; entries are small but for the few that
    must reach the block limit, 65536 bytes back or 2 MiB."""
    ok = [c for c in CASES if c[3] is not None]
    assert (len(CASES), len(ok), sum(c[4] == SHORT for c in CASES)) == (578, 451, 3)
    assert len(zstd_craft.PAIRS) == 21
    for good, bad in zstd_craft.PAIRS:
        assert zstd_craft.CASE[good][3] is not None and zstd_craft.CASE[bad][3] is None, (good, bad)
    assert all(len(c[3]) == c[2] and c[4] == 0 for c in ok)
    assert all(c[4] != 0 for c in CASES if c[3] is None)
    assert sum(c[2] > 4096 for c in CASES) <= 110 and sum(c[2] > (1 << 17) + 16 for c in CASES) <= 16
    assert max(c[2] for c in CASES) == 2097151
    for fam in "hblwtsd":
        assert any(c[0].startswith(fam + "_") and c[3] is None for c in CASES), fam
    for fam in "hblwts":
        assert any(c[0].startswith(fam + "_") and c[3] is not None for c in CASES), fam
    names = {c[0] for c in CASES}
    assert set(zstd_craft.DIVERGENT) <= names and set(zstd_craft.NO_CACHE_DIVERGENT) <= names
    assert (len(zstd_craft.DIVERGENT), len(zstd_craft.NO_CACHE_DIVERGENT)) == (1, 33)


def test_field_encoding():
    """the writer itself on values worked out by hand from RFC 8878"""
    zc = zstd_craft
    assert zc.frame([zc.Raw(b"abcdefgh")], fcs=8, fcs_bytes=1) == zc.A
    assert zc.frame([zc.Cb(b"x", [(1, 7, 3)])], fcs=4, fcs_bytes=1) == zc.B4       # offset value 7 = offset 4
    assert zc.frame([zc.Cb(b"x", [(1, 4, 3)])], fcs=4, fcs_bytes=1) == zc.B1
    assert zc.frame_header(fcs=65791, fcs_bytes=2)[4:] == b"\x60\xff\xff"
    assert zc.frame_header(window=0x0B, dict_bytes=2, dict_id=0x1234, checksum=True) == zc.MAGIC + b"\x06\x0b\x34\x12"
    assert zc.block(1, b"z", True, size=5) == b"\x2b\x00\x00z" and zc.block(0, b"ab", False) == b"\x10\x00\x00ab"
    assert zc.lit_raw(b"abc") == b"\x18abc" and zc.lit_raw(b"abc", 2) == b"\x34\x00abc"
    assert zc.lit_rle(0x41, 4096) == bytes([1 | 3 << 2 | (4096 << 4) & 0xFF, (4096 >> 4) & 0xFF, 4096 >> 12, 0x41])
    assert zc.lit_huf_header(2, 4, 1023, 500, 4) == (2 | 2 << 2 | 1023 << 4 | 500 << 18).to_bytes(4, "little")
    assert zc.nseq_bytes(127) == b"\x7f" and zc.nseq_bytes(128) == b"\x80\x80" and zc.nseq_bytes(5, 2) == b"\x80\x05"
    assert zc.nseq_bytes(0x7EFF) == b"\xfe\xff" and zc.nseq_bytes(0x7F00) == b"\xff\x00\x00"
    assert zc.seq_codes((16, 4, 35)) == ((16, 0, 1), (2, 0, 2), (32, 0, 1))
    assert zc.seq_codes((65536 + 65535, (1 << 31) - 1, 65539 + 65535)) == ((35, 65535, 16), (30, (1 << 30) - 1, 30),
                                                                            (52, 65535, 16))
    assert zc.bits_backward([(1, 1), (0, 2), (5, 3)]) == bytes([0b1100101])
    assert zc.bits_backward([(0x1FF, 9)]) == b"\xff\x03"
    # RFC 8878 §4.1.1's layout: the predefined offset table's first cells
    t = zc.predef()[1]
    assert (t.sym[:8], t.nb[:8], t.base[:8]) == ([0, 6, 9, 15, 21, 3, 7, 12], [5, 4, 5, 5, 5, 5, 4, 5], [0] * 8)
    assert [(s, t.nb[s], t.base[s]) for s in t.states_of[6]] == [(1, 4, 0), (24, 4, 16)]
    # Huffman: weights 1, 1, 2 (+ implied 3): codes from the low end of the table
    h = zc.Huf({0: 1, 1: 1, 2: 2, 3: 3})
    assert h.log == 3 and h.code == {0: (0, 3), 1: (1, 3), 2: (1, 2), 3: (1, 1)}
    assert h.desc_direct() == bytes([130, 0x11, 0x20])
    # repeat offsets (§3.1.2.5), ll == 0 shifting the index
    # 8 back; then ll == 0: value 2 is the third (4), value 1 the second (now 8); 1 - 1 read as 1
    assert zc.expand([[(b"abcdefgh", [(8, 11, 3), (0, 2, 3), (0, 1, 3)])]]) == b"abcdefgh" + b"abc" + b"hab" + b"gha"
    assert zc.expand([[(b"abcdefgh", [(8, 4, 3), (0, 3, 3)])]]) == b"abcdefgh" + b"hhh" + b"hhh"
    with pytest.raises(zc.Invalid):
        zc.expand([[b"abcdefgh"], [(b"x", [(1, 7, 3)])]])


def test_libzstd_verdicts_match_table(record):
    """libzstd 1.4.9's recorded code is the table's on every case (0 and a
    decoded length below the declared size where the table says SHORT), its
    bytes are expand's on every accepted one"""
    for (name, _, dsize, want, code), rec in zip(CASES, record):
        if code == SHORT:
            assert rec["code"] == 0 and rec["len"] < dsize, name
        else:
            assert rec["code"] == code, (name, rec["code"])
        if want is not None:
            assert (rec["len"], rec["sha"]) == (dsize, sha(want)), name


def test_oracle_matches_libzstd(oracle, record):
    """every case: the oracle's code is libzstd's; where libzstd decodes, its
    bytes are the record's (and so expand's)"""
    for (name, entry, dsize, _, _), rec in zip(CASES, record):
        got, code = oracle.zstd_decode(entry, dsize)
        assert code == rec["code"], (name, code, rec["code"])
        if code == 0:
            assert (len(got), sha(got)) == (rec["len"], rec["sha"]), name


def test_libzstd_live(record, maker):
    """where libzstd 1.4.9 is installed: run live, it gives the recorded verdicts"""
    z = maker.load_zstd()
    if z is None:
        pytest.skip("libzstd 1.4.9 not installed")
    for (name, entry, dsize, _, _), rec in zip(CASES, record):
        assert maker.libzstd_answer(z, entry, dsize) == [rec["code"], rec["len"], rec["sha"]], name


def test_reference_reader_live(ref, record, maker):
    """where the reference is built: run live on every 8th case, it gives the
    recorded answers"""
    for (name, entry, dsize, _, _), rec in list(zip(CASES, record))[::8]:
        if rec["reference"] != "hang" and dsize < (1 << 17):
            img, sizes = maker.case_image(entry, dsize)
            got = maker.ref_answers(ref, img, sum(sizes))
            assert [dict(zip(("bytes", "sha", "last", "error"), g)) for g in got] == rec["reference"], name


def test_reference_reader_record(record):
    """the reference reader with a cache (one ZSTD_decompressDCtx per entry)
    delivers exactly what libzstd's verdict says: everything, or the first
    neighbour alone and libzstd's error text"""
    (_, a), (_, b) = zstd_craft.NEIGHBOURS
    hangs = []
    for (name, _, dsize, want, code), rec in zip(CASES, record):
        if rec["reference"] == "hang":
            hangs.append(name)
            continue
        c1 = rec["reference"][1]
        if want is not None:
            assert (c1["bytes"], c1["last"], c1["sha"]) == (len(a) + dsize + len(b), 0, sha(a + want + b)), name
        elif dsize == 0:        # (an entry of no bytes is never read)
            assert (c1["bytes"], c1["last"], c1["sha"]) == (len(a) + len(b), 0, sha(a + b)), name
        else:
            assert (c1["bytes"], c1["last"], c1["sha"]) == (len(a), -1, sha(a)), name
    assert hangs == [c[0] for c in CASES if c[4] == SHORT]


def test_oracle_reads_past_a_streams_start_as_libzstd(oracle, maker):
    """Sequence streams cut short by 1 to 60 bits, or with bytes and counted
    sequences added: libzstd 1.4.9 decodes every counted sequence whatever the
    stream holds, reading on past its start inside its 64-bit container.  The
    oracle restates those reads; live libzstd, where installed, agrees on code
    and bytes (the oracle alone must at least be deterministic and in
    bounds)."""
    zc = zstd_craft
    z = maker.load_zstd()
    rng = np.random.default_rng(3)
    P = zc.predef()
    runs = 0
    for trial in range(60):
        ns = int(rng.integers(1, 40))
        seqs = [(int(rng.integers(0, 40)) + (i == 0), int(rng.integers(4, 8)) if i == 0 else int(rng.integers(1, 12)),
                 int(rng.integers(3, 400))) for i in range(ns)]
        lit = zc.lits(sum(s[0] for s in seqs) + 5, trial)
        try:
            want = zc.expand([[(lit, seqs)]])
        except zc.Invalid:
            continue
        for drop in (0, 1, 2, 3, 5, 8, 13, 21, 34, 60):
            for extra in (0, 1):
                try:
                    st = zc.seq_stream(seqs, P, drop_bits=drop)
                except ValueError:      # (fewer bits than that in the stream)
                    continue
                if not st or st[-1] == 0:
                    continue
                st = b"\xa7" * 3 * extra + st
                sec = zc.seq_section(seqs, P, stream=st, nseq=len(seqs) + extra * int(rng.integers(0, 3)))
                e = zc.frame_header() + zc.block(2, zc.lit_raw(lit) + sec, True)
                for ds in (len(want), len(want) + 500):
                    got = oracle.zstd_decode(e, ds)
                    assert got == oracle.zstd_decode(e, ds)
                    if drop == 0 and extra == 0:      # (whatever room the output has)
                        assert got == (want, 0), trial
                    if z is not None:
                        assert got == zstd_util_decode(z, e, ds), (trial, drop, extra, ds)
                    runs += 1
    assert runs > 1000


def test_cases_sit_on_the_rules_they_name():
    """What each family of cases would catch, shown on the model (the rules
    themselves run only on the GPU).
    "0 read as 1": without it every s_rep0_minus1_is_0_at* case meets offset
    0 -- in both forms of the replay, max(rep0 - 1, 1u) in the lane loop and
    x > v ? x - v : 1u in the wave form's composed maps.
    The item pad: lemit's slots by zstd_craft.items (lemit's whole rule: a
    match of 3 is extended too; literal tails and runs are items):
    s_ext_*_at_slot63 and _slot127 start their pair on slot 63 (padded by the
    == 63 rule, left astride two groups by == 62), _slot62 and _slot126 on
    slot 62 (padded by == 62 alone, which moves every later item by one).
    The FSE weight walk's two states: w_fse_one_state_walk is written for a
    walk with one state, which alone reads a complete set of weights from it;
    libzstd, with two, refuses it (code 20 in the record)."""
    zc = zstd_craft
    reps = [n for n in zc.MODELS if n.startswith("s_rep0_minus1_is_0_at")]
    assert len(reps) == 10
    for n in reps:
        with pytest.raises(zc.Invalid, match="offset 0"):
            zc.expand(zc.MODELS[n], clamp=False)
        assert zc.expand(zc.MODELS[n]) == zc.CASE[n][3]

    # lemit's slots, by lemit's whole rule (zstd_craft.items)
    for kind in ("pair", "ll", "ml3"):
        for slot in (61, 62, 63, 64, 65, 126, 127, 128):
            m = zc.MODELS[f"s_ext_{kind}_at_slot{slot}"]
            first = [i for i in zc.items(m) if i[1]][0]
            assert first == (slot, True, slot & 63 == 63)
        for slot in (63, 127):      # a pad occurs, and the == 62 rule would leave the pair astride two groups
            m = zc.MODELS[f"s_ext_{kind}_at_slot{slot}"]
            assert sum(i[2] for i in zc.items(m)) >= 1
            assert not [i for i in zc.items(m, 62) if i[1]][0][2] and zc.items(m, 62) != zc.items(m)
        for slot in (62, 126):      # no pad here; == 62 would add one and move every later item
            m = zc.MODELS[f"s_ext_{kind}_at_slot{slot}"]
            assert not [i for i in zc.items(m) if i[1]][0][2] and [i for i in zc.items(m, 62) if i[1]][0][2]
    # every accepted case's item count stays inside the plan's bound (2 per sequence + pads + 4 per block)
    padded = [n for n, m in zc.MODELS.items() if any(i[2] for i in zc.items(m))]
    assert len(padded) >= 6, padded
    h40 = zc.Huf(zc.flat_weights(range(40)))
    one = h40.desc_fse(6, one_state=True)
    assert one != h40.desc_fse(6) and zc.CASE["w_fse_one_state_walk"][4] == 20
    assert one in zc.CASE["w_fse_one_state_walk"][1]


def zstd_util_decode(z, e, ds):
    import zstd_util
    return zstd_util.decode(z, e, ds)


def test_random_valid(oracle, maker):
    """the generator's contract: the oracle (and live libzstd where it is
    installed) accepts 2000 of 2000 entries, to expand's bytes; entries decode
    to at most 4 KiB; it is deterministic and reaches the fields it draws"""
    entries = zstd_craft.random_valid(1, 2000)
    assert len(entries) == 2000
    z = maker.load_zstd()
    accepted = lib_accepted = 0
    for e, want in entries:
        got, code = oracle.zstd_decode(e, len(want))
        accepted += code == 0 and got == want
        if z is not None:
            got, code = zstd_util_decode(z, e, len(want))
            lib_accepted += code == 0 and got == want
    assert accepted == 2000
    assert z is None or lib_accepted == 2000
    assert max(len(w) for _, w in entries) <= 4096
    assert entries[:50] == zstd_craft.random_valid(1, 50)
    assert len({e for e, _ in entries}) > 1500
    assert any(len(w) == 0 for _, w in entries) and sum(len(w) > 1024 for _, w in entries) > 100
    blob = b"".join(e for e, _ in entries)
    assert blob.count(zstd_craft.MAGIC) > 2400        # several frames in an entry
