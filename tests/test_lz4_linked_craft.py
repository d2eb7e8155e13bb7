"""tests/lz4_linked_craft.py's hand-built linked frames on the CPU: the table's
verdicts and expected bytes (lz4_craft.expand, byte by byte), the oracle and
the record of liblz4 1.9.3 and the compiled reference reader
(tests/golden/lz4_linked_craft.json, made by make_lz4_linked_craft.py) must say
the same about every frame; and the table must hold what it is there for,
proved from taint_stats (the definition of taint, not the kernel's code): the
tainted-byte counts, hop chains, generations and clip phases at which
seq_exec_blocks_kernel changes path.  The GPU engines are held to the same
table in test_gpu_lz4_linked_craft.py."""
from __future__ import annotations

import importlib.util
import json
import os

import numpy as np
import pytest

import lz4_craft
import lz4_linked_craft as lc
from conftest import GOLDEN, sha
from lz4_linked_craft import B, BLOCKS, CASES
from test_lz4_craft import _oracle_loop


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_lz4_linked_craft",
                                                  os.path.join(GOLDEN, "make_lz4_linked_craft.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def record(maker):
    with open(os.path.join(GOLDEN, "lz4_linked_craft.json")) as f:
        meta = json.load(f)
    assert meta["sha_digits"] == maker.H
    assert [c["name"] for c in meta["cases"]] == [c[0] for c in CASES], "regenerate lz4_linked_craft.json"
    assert [c["frame_sha"] for c in meta["cases"]] == [maker.sha(c[1]) for c in CASES], \
        "regenerate lz4_linked_craft.json"
    assert meta["neighbour_frame_shas"] == [maker.sha(f) for f, _ in lz4_craft.NEIGHBOURS]
    return meta


@pytest.fixture(scope="module")
def stats():
    """taint_stats of every accepted case"""
    return {c[0]: lc.taint_stats(BLOCKS[c[0]]) for c in CASES if c[3] is not None}


def test_table_shape():
    """524 cases, 520 accepted; per family a-g 330, 84, 54, 16, 22, 15, 3;
    every frame is linked, block size id 4, no checksums; every block but the
    last of an accepted frame decodes to 64 KiB (f_mid_B-1 apart); no frame is
    above 4 MiB decoded but the 65-block one (by 13 bytes)"""
    ok = [c for c in CASES if c[3] is not None]
    assert (len(CASES), len(ok)) == (524, 520)
    fam = {k: sum(c[0].startswith(k + "_") for c in CASES) for k in "abcdefg"}
    assert fam == {"a": 330, "b": 84, "c": 54, "d": 16, "e": 22, "f": 15, "g": 3}
    assert [c[0] for c in CASES if c[3] is None] == ["f_mid_B+1", "g_truncated_seq", "g_match_ext_cut",
                                                     "g_block_size_over"]
    for name, f, ds, want in CASES:
        assert f[4] & 0xF4 == 0x40 and f[5] == 0x40, name     # version 1, linked, no checksums; 64 KiB blocks
        assert want is None or len(want) == ds
        assert ds <= 4 << 20 or name == "f_blocks65" and ds == (4 << 20) + 13
        if want is not None and name != "f_mid_B-1":
            sizes = [len(b) if isinstance(b, bytes) else lc.size_of(b) for b in BLOCKS[name]]
            assert all(s == B for s in sizes[:-1]) and len(sizes) >= 2, name
    # block 0 in both variants in every family that decodes
    for k in "abcdef":
        kinds = {isinstance(BLOCKS[c[0]][0], bytes) for c in CASES if c[0].startswith(k + "_")}
        assert kinds == {True, False}, k
    # lz4_craft's own table is not this module's to change
    assert len(lz4_craft.CASES) == 270


def test_lits_is_lz4_crafts():
    for n, salt in ((0, 0), (1, 3), (300, 7), (70000, 1), (B, 123)):
        assert lc.lits(n, salt) == lz4_craft.lits(n, salt)


def test_liblz4_verdicts_match_table(record):
    """liblz4 1.9.3 accepts exactly the cases the table calls accepted (the
    frame decodes and to the declared size), to expand's bytes"""
    for (name, _, dsize, want), rec in zip(CASES, record["cases"]):
        lz = rec["lz4f"]
        assert (lz["ok"] and lz["len"] == dsize) == (want is not None), name
        if want is not None:
            assert lz["sha"] == sha(want)[:16], name


def test_oracle_matches_liblz4(oracle, record):
    """Every case: the oracle's status and error name on the frame alone are
    liblz4's; every accepted case: its bytes are expand's and the record's."""
    for (name, frame, dsize, want), rec in zip(CASES, record["cases"]):
        lz = rec["lz4f"]
        st, got, _, _ = oracle.decode_frame(frame, dsize + record["lz4f_slack"])
        assert (st == 0) == lz["ok"], name
        assert oracle.error_name(st) == (lz["error"] or "OK_NoError"), name
        if st == 0:
            assert len(got) == lz["len"] and sha(got)[:16] == lz["sha"], name
        st, got, _, _ = oracle.decode_frame(frame, dsize)
        assert (st == 0 and len(got) == dsize) == (want is not None), name
        if want is not None:
            assert got == want, name


def test_oracle_matches_reference_reader(oracle, record, maker):
    """Every case between lz4_craft's two neighbours in a seekable file: the
    oracle's decode and test_cpu.py's error rule give the recorded answers of
    the reference reader's pread loop, cache 0 and 1 -- for accepted cases the
    neighbours' and expand's bytes.  No case hangs the reference."""
    (_, a), (_, b) = lz4_craft.NEIGHBOURS
    for (name, frame, dsize, want), rec in zip(CASES, record["cases"]):
        assert rec["reference"] != "hang", name
        img, total = maker.case_image(frame, dsize)
        for cache in (0, 1):
            ans = rec["reference"][f"cache{cache}"]
            mine = _oracle_loop(oracle, img, total, cache, [len(a), dsize, len(b)])
            mine["sha"] = mine["sha"][:16]
            assert mine == ans, (name, cache)
            if want is not None:
                assert (ans["bytes"], ans["last"], ans["sha"]) == (total, 0, sha(a + want + b)[:16]), (name, cache)
            else:
                assert (ans["bytes"], ans["last"]) == (len(a), -1), (name, cache)


def test_reference_reader_live(ref, record, maker):
    """where the reference is built: run live, it gives the recorded answers"""
    for (name, frame, dsize, _), rec in zip(CASES, record["cases"]):
        img, total = maker.case_image(frame, dsize)
        assert maker.ref_answers(ref, img, total) == rec["reference"], name


def test_liblz4_live(record, maker):
    """where liblz4 1.9.3 is installed: run live, it gives the recorded verdicts"""
    lz = maker.load_lz4()
    if lz is None or lz.LZ4_versionNumber() != 10903:
        pytest.skip("liblz4 1.9.3 not installed")
    for (name, frame, dsize, _), rec in zip(CASES, record["cases"]):
        assert maker.lz4f_verdict(lz, frame, dsize) == rec["lz4f"], name


def test_taint_stats_on_known_blocks():
    """taint_stats on blocks small enough to work out by hand"""
    prev = lc.b0(0)
    # 3 literals, then 6 bytes from 5 back: 2 from before the block (origins
    # B - 2, B - 1), the 3 literals, and the first of the 2 again
    st = lc.taint_stats([prev, [(b"abc", 5, 6), lc.T(5)]])[1]
    assert st["origin"].tolist() == [-1, -1, -1, B - 2, B - 1, -1, -1, -1, B - 2] + [-1] * 5
    assert (st["tainted"], st["hops"], st["gen"]) == (3, 1, 1)
    assert st["matches"] == [(3, 5, 6, "wide", 2)]
    # the next block copies that block's bytes 3.. (off = 14 - 3): 2 hops where
    # the source is tainted; then a copy of its own tainted bytes: generation 2
    st = lc.taint_stats([prev, [(b"abc", 5, 6), lc.T(5)], [(b"", 11, 4), (b"xy", 6, 4), lc.T(5)]])[2]
    assert st["origin"].tolist() == [3, 4, 5, 6, -1, -1, 3, 4, 5, 6] + [-1] * 5
    assert (st["tainted"], st["hops"], st["gen"]) == (8, 2, 2)
    assert st["matches"] == [(0, 11, 4, "wide", 0), (6, 6, 4, "wide", 0)]
    st = lc.taint_stats([prev, [(lc.lits(20, 1), 36, 40), lc.T(5)]])[1]
    assert st["matches"] == [(20, 36, 40, "pieces", 16)] and st["tainted"] == 16 + 4     # 16, then 36 + k of 40 again
    # offset 0 writes zeros, a stored block has no tainted byte
    st = lc.taint_stats([prev, [(b"q", 0, 9), lc.T(5)], lc.S(b"stored")])
    assert [s["tainted"] for s in st] == [0, 0, 0]


def test_taint_stats_origins_hold_the_bytes(stats):
    """every tainted byte of every accepted case equals, in expand's output,
    the previous block's byte taint_stats names as its origin: the restated
    definition agrees with the byte model"""
    for name, _, _, want in CASES:
        if want is None:
            continue
        out = np.frombuffer(want, np.uint8)
        pos = prev = 0
        for k, st in enumerate(stats[name]):
            o = st["origin"]
            t = np.nonzero(o >= 0)[0]
            assert st["tainted"] == t.size
            if t.size:
                assert (out[pos + t] == out[prev + o[t]]).all(), (name, k)
            prev, pos = pos, pos + len(o)
        assert pos == len(want), name


def test_table_covers_the_taint_paths(stats):
    """What the table is for, from taint_stats: a block at each tainted-byte
    count of family d (the split over 1,024 threads and its binary search),
    hop chains of 1, 2, 4, 32 and 63 blocks, generations of 3 and more inside
    a block, and both copy rules -- a lane a byte, 16-byte pieces -- at every
    clip length 1..16 of a match that straddles the block start."""
    counts, hops, gens, clips, rules = set(), set(), set(), set(), set()
    for name, per_block in stats.items():
        for k, st in enumerate(per_block):
            if k:
                counts.add(st["tainted"])
            hops.add(st["hops"])
            gens.add(st["gen"])
            for _, _, _, rule, clip in st["matches"]:
                rules.add(rule)
                if clip:
                    clips.add((rule, clip))
    assert counts >= set(lc.D_COUNTS) == {0, 1, 4, 1023, 1024, 1025, 4097, B - 5}
    assert hops >= {1, 2, 4, 32, 63}
    assert {3, 10} <= gens and max(gens) >= 16380
    assert clips == {(r, c) for r in ("wide", "pieces") for c in range(1, 17)}
    # the block with no tainted byte is followed by one with
    for v in (0, 1):
        assert [s["tainted"] for s in stats[f"d_tainted0_v{v}"]] == [0, 0, B - 5]
    # every family d block has a chain block hopping through its origins
    for n in lc.D_COUNTS:
        st = stats[f"d_tainted{n}_v1"]
        assert st[1]["tainted"] == n and st[2]["hops"] == (2 if n else 1), n
    # tainted matches start at every phase of a 16-byte piece, pieces with
    # only their first / only their last byte tainted among them, and the next
    # blocks' chains run through them
    st = stats["e_chain_through_sparse"]
    t = (st[1]["origin"] >= 0).reshape(-1, 16)
    assert {m[0] % 16 for m in st[1]["matches"]} == set(range(16)) and st[1]["tainted"] == 1024
    masks = {int(sum(int(b) << i for i, b in enumerate(row))) for row in t}
    assert {0x0001, 0x8000, 0x000F, 0xF000} <= masks
    assert [x["hops"] for x in st] == [0, 1, 2, 3]
    # both sides of the two rule switches, each on a tainted source
    for off, ml, rule in ((15, 20, "wide"), (16, 20, "pieces"), (40, 256, "pieces"), (40, 257, "wide")):
        for kind in ("first", "gen2"):
            m = stats[f"a_switch_off{off}_ml{ml}_{kind}"][1]["matches"][-1]
            assert m[1:4] == (off, ml, rule), (off, ml, kind)
    # family b: tainted matches start at each phase of a 32-bit word, low in
    # the block and ending on its last coverable byte, by both rules
    for tag, rule in (("pieces", "pieces"), ("lanes", "wide")):
        low = {(m[0] % 32, m[2]) for n, s in stats.items() if n.startswith("b_x") and n.endswith(tag)
               for m in s[1]["matches"][-1:] if m[3] == rule}
        assert low == {(r, L) for r in lc.B_PHASES for L in lc.B_LENS}, tag
        top = {m[0] % 32 for n, s in stats.items() if n.startswith("b_top") and n.endswith(tag)
               for m in s[1]["matches"][-1:] if m[3] == rule and m[0] + m[2] == B - 5}
        assert top == set(lc.B_PHASES), tag
    # family c: a source piece whose first ph / last 16 - ph bytes are tainted
    for ph in range(17):
        o = stats[f"c_t2u_ph{ph}"][1]["origin"]
        assert (o[164:180] >= 0).all() and (o[180:180 + ph] >= 0).all() and (o[180 + ph:212] < 0).all(), ph
        o = stats[f"c_u2t_ph{ph}"][1]["origin"]
        assert (o[200:216 + ph] < 0).all() and (o[216 + ph:248] >= 0).all(), ph
    # the chain frames: block k's chain is k hops long
    for nb in lc.E_BLOCKS:
        assert [s["hops"] for s in stats[f"e_chain{nb}_off65535"]] == list(range(nb))
    assert [s["hops"] for s in stats["e_chain_into_stored"]] == [0, 1, 2, 0, 1, 2]
    assert [s["hops"] for s in stats["e_zeros64"]] == [0] + [1] * 63
    assert stats["e_chain_from_gen2"][1]["gen"] == 3 and stats["e_chain_from_gen2"][3]["hops"] == 3


def test_random_linked(oracle):
    """the generator's contract: the oracle accepts 200 of 200 frames, to
    expand's bytes; 2 to 6 blocks, every block but the last full; it is
    deterministic; at least a fifth of all match bytes are tainted and at
    least 20 frames have a chain of 2 hops or more"""
    frames = lc.random_linked(5, 200)
    assert len(frames) == 200
    match_bytes = tainted = chains = 0
    for f, want, blocks in frames:
        st, got, _, _ = oracle.decode_frame(f, len(want))
        assert st == 0 and got == want
        sizes = [len(b) if isinstance(b, bytes) else lc.size_of(b) for b in blocks]
        assert 2 <= len(sizes) <= 6 and all(s == B for s in sizes[:-1]) and sum(sizes) == len(want)
        ts = lc.taint_stats(blocks)
        chains += max(s["hops"] for s in ts) >= 2
        tainted += sum(s["tainted"] for s in ts)
        match_bytes += sum(ml for b in blocks if not isinstance(b, bytes) for _, off, ml in b if off is not None)
    assert tainted * 5 >= match_bytes, (tainted, match_bytes)
    assert chains >= 20, chains
    assert [f for f, _, _ in frames[:20]] == [f for f, _, _ in lc.random_linked(5, 20)]
    assert len({f for f, _, _ in frames}) == 200
