"""tests/exec_craft.py's hand-built frames on the CPU: the oracle (and, for the
zstd forms, libzstd 1.4.9) accept every case to expand's bytes; the record of
the compiled reference reader (tests/golden/exec_craft.json, made by
make_exec_craft.py) says the same; and the table holds what it is there for --
proved from exec_craft's model of what the execute kernels decide (the cut, the
readiness rule, `flushed`, the windows), not from the kernels' code: every
family's named structure is asserted to be really there.  The GPU engines are
held to the same table in test_gpu_exec_craft.py."""
from __future__ import annotations

import importlib.util
import json
import os

import numpy as np
import pytest

import exec_craft as ec
import lz4_craft
import zstd_craft
import zstd_util
from conftest import GOLDEN, sha
from exec_craft import CASES, FOLLOW, KBWIN, KFCSTAGE, KFMAX, NAMES, RECIPES, W_LZ4, W_SEG, W_ZSTD, WIN_ITEMS, WS, stats

WW = (W_LZ4, W_SEG)


def w(W):
    return f"_w{W}"


def under(b):
    """the batch under test: the one after the preamble's"""
    return b["batches"][1]


def test_constants_and_shape():
    """the stage sizes and the workgroup kernels' constants are read from the
    sources; the table has every family, its frames are small but for the ones
    that have to be big (the grid, the too-long sequences, the frame kernel's
    item counts and chain, family g)"""
    assert 1024 <= W_LZ4 <= W_SEG == W_ZSTD and W_LZ4 % 16 == 0 and W_SEG % 16 == 0
    assert KFCSTAGE > KFMAX == KBWIN and ec.KFLONG >= 64 and ec.CONST["kFT"] == 1024
    fam = {k: sum(n[0] == k for n in NAMES) for k in "abcdefg"}
    assert fam == {"a": 42, "b": 84, "c": 20, "d": 230, "e": 18, "f": 40, "g": 8}
    assert len(ec.ZALL) == len(ec.Z_NAMES) + 6 and len(ec.Z_NAMES) == 185
    for name, f, ds, want in CASES:
        assert len(want) == ds
        if name[0] in "ade" or name.startswith("c_") and "grid" not in name:
            assert ds <= 8192 or "unfit_twice" in name and ds <= 2 * W_SEG + 600, name   # (two full batches)
        assert (ds > KFMAX) == (name[0] == "g"), name
    # no two literal runs of a case alike: a stale stage byte is not the right one
    for name in ("d_fanout_w3072", "c_pieces256_w4096", "a_sum+0_w3072"):
        runs = [s[0] for b in RECIPES[name][0] for s in b if len(s[0]) >= 4]
        assert len(set(runs)) == len(runs)


def test_oracle_accepts_lz4(oracle):
    """every LZ4 case: status 0 and expand's bytes"""
    for name, f, ds, want in CASES:
        st, got, _, _ = oracle.decode_frame(f, ds)
        assert st == 0 and got == want, name


def test_oracle_accepts_zstd(oracle):
    """every zstd case: the oracle decodes it to zstd_craft.expand's bytes,
    which are lz4_craft.expand's for the cases the two formats share"""
    for name, f, ds, want in ec.ZCASES:
        got, code = oracle.zstd_decode(f, ds)
        assert code == 0 and got == want, name
        if name in RECIPES:
            assert want == ec.case(name)[3], name


def test_libzstd_accepts_zstd():
    """... and so does libzstd 1.4.9, where it is installed"""
    z = zstd_util.load()
    if z is None:
        pytest.skip("libzstd 1.4.9 not installed")
    for name, f, ds, want in ec.ZCASES:
        assert zstd_util.decode(z, f, ds) == (want, 0), name


def test_zstd_slots_are_zstd_crafts():
    """the zstd lanes are zstd_craft.items' slots (lemit's rule: a pair never
    starts in slot 63 of a group)"""
    for name in ec.ZALL:
        zb = ec.ZRECIPES[name] if name in ec.ZRECIPES else ec.zblocks(RECIPES[name][0])
        ln = ec.zlanes_of(name)
        slots = [(k, x[3]) for k, x in enumerate(ln) if x[0] + x[1]]
        assert slots == [(k + pad, e) for k, e, pad in zstd_craft.items([zstd_craft.model(zb)])], name
        assert not any(x[3] and k & 63 == 63 for k, x in enumerate(ln)), name


# ---------------------------------------------------------------------------
# reach: the structure each family is named for is there, by the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("W", WW)
def test_reach_cut(W):
    assert [stats(f"a_sum{d:+d}{w(W)}", W)["nb"][0] for d in (-1, 0, 1)] == [64, 64, 63]
    for d, tot in ((-1, W - 1), (0, W)):
        assert stats(f"a_sum{d:+d}{w(W)}", W)["batches"][0]["end"] == tot
    for k in (1, 2, 31, 32, 33, 62, 63):
        st = stats(f"a_over_lane{k}{w(W)}", W)
        b = st["batches"][0]
        assert b["nb"] == k and not b["long"], k
        nxt = ec.lanes_of(f"a_over_lane{k}{w(W)}")[k]
        assert b["end"] <= W < b["end"] + nxt[0] + nxt[1]
    assert [stats(f"a_items{k}{w(W)}", W)["nb"] for k in (63, 64, 65, 127, 128, 129)] == \
        [[63], [64], [64, 1], [64, 63], [64, 64], [64, 64, 1]]
    for k, nb in ((0, 6), (62, 64), (63, 63)):
        ln = ec.lanes_of(f"a_pair_lane{k}{w(W)}")
        assert ln[k][3] and stats(f"a_pair_lane{k}{w(W)}", W)["nb"][0] == nb
    # the scan engine's and zstd's padding item moves the pair off slot 63
    assert stats(f"a_pair_lane63{w(W)}", W, pad=True)["nb"][0] == 64
    st = stats(f"a_pair_unfit{w(W)}", W)
    assert st["nb"][0] == 40 and ec.lanes_of(f"a_pair_unfit{w(W)}")[40][3]
    st = stats(f"a_pair_unfit_twice{w(W)}", W)
    ln = ec.lanes_of(f"a_pair_unfit_twice{w(W)}")
    assert st["nb"][:2] == [40, 42] and ln[40][3] and ln[82][3] and st["long"] == 0


def test_reach_too_long():
    """every b case under the stage size it is aimed at (5,000 bytes: both):
    the long sequence is an nb == 0 step -- the frame's first step, or two
    steps back to back after at least two ordinary batches -- and the batch
    right after holds the short matches whose sources end 1..33 bytes before
    its end, all of them early"""
    for name in (n for n in NAMES if n[0] == "b"):
        aim = RECIPES[name][1]
        for W in WS if aim is None else (aim,):
            st = stats(name, W)
            longs = [k for k, b in enumerate(st["batches"]) if b["long"]]
            if name.endswith("_first"):
                assert longs == [0], name
            else:
                assert len(longs) == 2 and longs[1] == longs[0] + 1 and longs[0] >= 2, name
                assert all(st["batches"][k]["nb"] > 0 for k in range(longs[0])), name
            end = st["batches"][longs[-1]]["end"]
            nxt = st["batches"][longs[-1] + 1]
            assert nxt["bstart"] == end
            assert [end - m["need"] for m in nxt["matches"][:7]] == list(FOLLOW), name
            assert all(m["early"] and m["me"] - m["mb"] == 8 for m in nxt["matches"][:7]), name
            # aimed: a sequence shorter by one byte would have been staged
            b = st["batches"][longs[0]]
            if aim is not None:
                assert max(b["lit"], b["ml"]) == W + 1 + ("apart1" in name and name.endswith("_first")), name
    offs = {int(n.split("_off")[1].split("_")[0]) for n in NAMES if n.startswith("b_ovl_ml5000")}
    assert offs == {1, 2, 3, 7, 15, 16, 17, 31, 1023, 1024, 1025, 4999}
    for W in WS:
        b = stats(f"b_apart0_ml{W + 1}_after", W)["batches"]
        k = next(k for k, x in enumerate(b) if x["long"])
        assert (b[k]["lit"], b[k]["off"], b[k]["ml"]) == (0, W + 1, W + 1)
        b = stats(f"b_apart1_ml{W + 1}_after", W)["batches"]
        assert (b[k]["lit"], b[k]["off"], b[k]["ml"]) == (0, W + 2, W + 1)
        assert stats(f"b_lit{W + 1}_first", W)["batches"][0]["lit"] == W + 1


@pytest.mark.parametrize("W", WW)
def test_reach_round0(W):
    st = stats(f"c_grid{w(W)}", W)
    ms = [m for b in st["batches"][1:] for m in b["matches"]]
    seqs = ec.seqs_of(RECIPES[f"c_grid{w(W)}"][0])[1:-1]
    assert {(s[0], s[1]) for s in seqs} == {(a, b) for a in range(34) for b in range(4, 21)}
    assert len(ms) == 34 * 17 and all(m["early"] for m in ms) and st["rounds"][1:] == [0] * (len(st["nb"]) - 1)
    assert under(stats(f"c_pieces256{w(W)}", W))["pieces"] == 256
    p = under(stats(f"c_pieces304{w(W)}", W))
    assert 300 <= p["pieces"] <= W // 16 + 128 and p["nb"] == 64 and p["end"] - p["bstart"] <= W
    b = under(stats(f"c_src_end_bstart{w(W)}", W))
    assert len(b["matches"]) == 20 and all(m["need"] == b["bstart"] and m["early"] for m in b["matches"])
    b = under(stats(f"c_src_end_bstart+1{w(W)}", W))
    assert len(b["matches"]) == 20 and all(m["need"] == b["bstart"] + 1 and m["round"] == 1 for m in b["matches"])
    for ml in (4, 15, 16, 17, 40):
        for a0 in range(16):
            b = under(stats(f"c_flushed_ml{ml}{w(W)}", W, a0=a0))
            assert b["bstart"] == W - 9 and b["bstart"] - 15 <= b["flushed"] <= b["bstart"]
            rel = [m["msrc"] - b["flushed"] for m in b["matches"]]
            assert rel == list(range(rel[0], rel[0] + 49))
            if a0 == 0:
                assert (rel[0], rel[-1]) == (-32, 16)
            # both sides of the stage-or-HBM choice, at the piece's 16th byte
            assert {-17, -16, -15} <= set(rel)
        assert any(m["early"] for m in b["matches"]) or ml == 40


@pytest.mark.parametrize("W", WW)
def test_reach_rounds(W):
    seen = set()
    for depth in ec.CHAIN_DEPTHS:
        for ml in ec.CHAIN_MLS:
            name = f"d_chain{depth}_ml{ml}{w(W)}"
            if name not in RECIPES:
                assert ml + 7 + depth * (ml + 1) > W
                continue
            b = under(stats(name, W))
            assert (b["rounds"], b["pending"], b["nb"]) == (depth, depth, min(depth + 2, 64)), name
            assert not any(m["overlap"] for m in b["matches"])
            seen.add((depth, ml))
    assert {d for d, _ in seen} == set(ec.CHAIN_DEPTHS) and {m for _, m in seen} == set(ec.CHAIN_MLS)
    assert (63, 4) in seen and (63, 16) in seen and all((3, m) in seen for m in ec.CHAIN_MLS)
    # adjacency: ready in round 1 when the source touches both neighbours,
    # blocked for a round when it is shifted by a byte either way
    for tag, rnd, blocker in (("", 1, None), ("_lo", 2, 0), ("_hi", 2, 1)):
        b = under(stats(f"d_adj{tag}{w(W)}", W))
        a, c, m = b["matches"]
        assert [a["round"], c["round"], m["round"]] == [1, 1, rnd]
        if tag == "":
            assert m["msrc"] == a["me"] and m["need"] == c["mb"]
        else:
            x = (a, c)[blocker]
            assert x["me"] > m["msrc"] and x["mb"] < m["need"]
            assert (m["msrc"] == a["me"] - 1) if blocker == 0 else (m["need"] == c["mb"] + 1)
    for k in (2, 3, 10):
        b = under(stats(f"d_span{k}{w(W)}", W))
        m = b["matches"][-1]
        hit = [x for x in b["matches"][:-1] if x["me"] > m["msrc"] and x["mb"] < m["need"]]
        assert len(hit) == k and m["round"] == 2 and all(x["round"] == 1 for x in hit)
    b = under(stats(f"d_lowest_only{w(W)}", W))
    m = b["matches"][-1]
    assert [x["early"] for x in b["matches"]] == [False] + [True] * 5 + [False] and m["round"] == 2
    assert b["matches"][0]["mb"] == m["msrc"] and b["matches"][0]["me"] == m["need"]
    b = under(stats(f"d_fanout{w(W)}", W))
    assert b["nb"] == 64 and b["pending"] == 63 and b["rounds"] == 1
    lit0 = (b["bstart"], b["bstart"] + 200)
    assert all(lit0[0] <= m["msrc"] and m["need"] <= lit0[1] for m in b["matches"][1:])
    for off in ec.OVL_PEND_OFFS:
        a, m = under(stats(f"d_ovl_pend_off{off}{w(W)}", W))["matches"]
        assert m["overlap"] and m["mb"] - m["msrc"] == off and (a["round"], m["round"]) == (1, 2)
        assert a["mb"] <= m["msrc"] and m["mb"] == a["me"]       # its pattern: bytes of the pending match
    ms = under(stats(f"d_same_round{w(W)}", W))["matches"]
    assert sorted((m["round"], m["overlap"]) for m in ms) == [(0, False)] + [(1, False)] * 3 + [(1, True)] * 2
    ms = under(stats(f"d_ovl_edge{w(W)}", W))["matches"]
    assert [(m["mb"] - m["msrc"], m["me"] - m["mb"], m["overlap"]) for m in ms] == \
        [x for off in ec.OVL_EDGE_OFFS for x in ((off, off + 1, True), (off, off, False))]
    assert all(m["round"] == 1 for m in ms)
    for off in range(16, 49):
        for a0 in (0, 7, 15):
            b = under(stats(f"d_ovl_first_off{off}{w(W)}", W, a0=a0))
            m = b["matches"][0]
            assert m["lane"] == 0 and m["overlap"] and m["mb"] == b["bstart"] and m["mb"] - m["msrc"] == off
            assert m["msrc"] < b["flushed"] <= b["bstart"]


def test_reach_flush():
    for k in range(1, 18):
        assert ec.case(f"e_len{k}")[2] == k
    for W in WS:
        st = stats("e_mod16", W)
        assert sorted(b["end"] % 16 for b in st["batches"][:16]) == list(range(16)) and st["nb"][:16] == [64] * 16


def test_reach_frame_kernel():
    assert [len(stats(f"f_items{k}")["frame"]["windows"]) for k in ec.F_ITEMS] == [1, 1, 2, 2, 3]
    assert [stats(f"f_items{k}")["lanes"] for k in ec.F_ITEMS] == list(ec.F_ITEMS)
    for k in (ec.KFT - 1, WIN_ITEMS - 1):
        ln = ec.lanes_of(f"f_pair_at{k}")
        assert ln[k][3] and ln[k + 1] == (0, 0, 0, False)
    for k in ec.F_LITS:
        assert [s[0] for s in ec.seqs_of(RECIPES[f"f_lit{k}"][0])][1:3] == [k, k]
    assert ec.F_LITS[2:4] == (ec.KFLONG, ec.KFLONG + 1)
    name, f, ds, _ = ec.case("f_unstaged")
    assert len(f) > KFCSTAGE and ds <= KFMAX and stats(name)["lanes"] > KFCSTAGE // 5
    seqs = ec.seqs_of(RECIPES["f_apart"][0])
    assert {(s[1], s[2]) for s in seqs[1:-1]} == {(m, k * m) for m in (64, 65, 128, 129) for k in (1, 2)}
    for ov in (16, 17, 31, 32, 33, 63, 64, 65):
        seqs = ec.seqs_of(RECIPES[f"f_trail_ov{ov}"][0])[:-1]
        assert all(s[2] == ov and s[1] > ov for s in seqs) and len(seqs) == 3
    for ov in range(1, 16):
        e = ov * ((16 + ov - 1) // ov)
        seqs = ec.seqs_of(RECIPES[f"f_ovl_ov{ov}"][0])[:-1]
        assert {s[1] for s in seqs} == {4, e - 1, e, e + 1, e + 15, e + 16, e + 17, 300} and all(s[2] == ov for s in seqs)
    ln = ec.lanes_of("f_done_words")
    p, rng = 0, set()
    for L, M, O, _ in ln:
        p += L
        if M > 64:
            rng.add((p - O, p - O + M))
        p += M
    assert rng == {(s, e) for s in (95, 96, 97) for e in (191, 192, 193)}
    st = stats("f_chain64k")
    assert st["total"] > KFMAX - 8 and st["total"] <= KFMAX and st["frame"]["depth"] > 16000
    assert len(st["frame"]["windows"]) == 8


def test_reach_window_kernel():
    def big(name):
        st = stats(name)
        assert st["total"] > 3 * KBWIN and not st["big"]["stuck"]
        return st["big"]["batches"], ec.lanes_of(name)

    def ends(ln, k):
        return sum(x[0] + x[1] for x in ln[: k + 1])

    b, ln = big("g_end_at_win+0")
    assert ends(ln, b[0]["cut"] - 1) == KBWIN and b[0]["P"] == KBWIN           # ends exactly at H + kBWin: kept
    b, ln = big("g_end_at_win+1")
    assert ends(ln, b[0]["cut"]) == KBWIN + 1 and b[0]["P"] < KBWIN            # one byte past: the cut item
    for d, slid in ((-1, False), (0, True), (1, True)):
        b, ln = big(f"g_three_quarters{d:+d}")
        assert (b[0]["cut"], b[0]["P"], b[0]["slide"]) == (None, KBWIN - KBWIN // 4 + d, slid)
        assert b[1]["w0"] == WIN_ITEMS and b[1]["H"] == (b[0]["P"] if slid else 0)
    b, ln = big("g_sources_at_h")
    H = b[1]["H"]
    assert H == KBWIN and b[0]["slide"] and b[0]["cut"] == b[1]["w0"]
    first = ln[b[1]["w0"]]
    assert (first[0], first[2]) == (0, 65535)                                   # at H, from H - 65,535
    p, src = H, []
    for L, M, O, _ in ln[b[1]["w0"]: b[1]["w0"] + 5]:
        p += L
        src.append((p - O - H, p - O + min(O, M) - H))
        p += M
    assert src[1:] == [(-20, 20), (-40, 0), (0, 40), (-1, 79)]
    b, ln = big("g_pair_across_items")
    assert ln[WIN_ITEMS - 1][3] and b[0]["cut"] is None and b[1]["w0"] == WIN_ITEMS
    b, ln = big("g_pair_is_cut")
    assert ln[b[0]["cut"]][3] and b[0]["slide"]
    assert [sum(x["slide"] for x in big(n)[0]) for n in NAMES if n[0] == "g"] == [3, 3, 3, 3, 3, 3, 3, 3]
    # the stuck path: lz4_craft's block over 64 KiB with one item longer than the window
    name, f, ds, want = lz4_craft.CASE["a_bsid5_match_end_cap-6"]
    out = ec.big_model(ec.lanes([(1, ds - 6, 1), (5, 0, 0)]))
    assert ds > KBWIN and out["stuck"]


def test_reach_zstd():
    """family h: the shared cases keep their structure under zstd's slot
    rules at W = 4096 (a pair moved off slot 63 apart); matches of 3 and
    offsets over 65,535 are pairs"""
    W = W_ZSTD
    for name in ec.Z_NAMES:
        if name[0] == "f":
            continue
        a, b = stats(name, W, "zstd"), stats(name, W)
        if name == f"a_pair_lane63{w(W)}":
            assert a["nb"][0] == 64 and b["nb"][0] == 63
        else:
            assert a["nb"] == b["nb"] and a["rounds"] == b["rounds"] and a["pieces"] == b["pieces"], name
    for k in ec.H_SLOTS:
        ln = ec.zlanes_of(f"h_off_pair_after{k}")
        far = [i for i, x in enumerate(ln) if x[2] > 0xFFFF]
        assert ln[0][3] and len(far) == 3 and all(ln[i][3] for i in far)   # (the last repeats the offset)
        assert far[0] == k + 2 + (k == 61)      # (slot 63 is padded)
    st = stats("h_ml3_chain", W)
    assert sum(st["rounds"]) >= 62 and all(x[3] for x in ec.zlanes_of("h_ml3_chain") if x[1] == 3)
    st = stats("h_ml3_unfit", W)
    ln = ec.zlanes_of("h_ml3_unfit")
    assert st["nb"][0] == 2 and ln[2][3] and ln[2][1] == 3 and st["batches"][0]["end"] == W - 2


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
SEEDS = {"lz4": (3, 300), "zstd": (5, 100)}


@pytest.mark.parametrize("fmt", ["lz4", "zstd"])
def test_random_exec(oracle, fmt):
    """valid by the oracle, deterministic, and dense: at least half of all
    batches have >= 20 pending matches and >= 4 rounds, at both stage sizes"""
    seed, n = SEEDS[fmt]
    frames = ec.random_exec(seed, n, fmt)
    assert [(f, x) for f, x, _ in frames[:20]] == [(f, x) for f, x, _ in ec.random_exec(seed, 20, fmt)]
    for f, want, _ in frames:
        if fmt == "lz4":
            st, got, _, _ = oracle.decode_frame(f, len(want))
            assert st == 0 and got == want
        else:
            assert oracle.zstd_decode(f, len(want)) == (want, 0)
        assert len(want) <= 8192
    for W in WS:
        bs = [b for _, _, seqs in frames for b in stats([seqs], W, fmt)["batches"]]
        dense = sum(b["pending"] >= 20 and b["rounds"] >= 4 for b in bs)
        assert len(bs) >= 2 * n and 2 * dense >= len(bs), (dense, len(bs))


# ---------------------------------------------------------------------------
# the model against scripts/exec_model.py on compressor output
# ---------------------------------------------------------------------------
def kernel_cut(ln, b, W):
    """seq_exec_kernel's own lines for one batch at lane b, restated one by
    one (the ballot, the two pair rules, the list's end): -> lanes taken"""
    nit, inc, over = len(ln), 0, None
    for lane in range(64):
        if b + lane < nit:
            inc += ln[b + lane][0] + ln[b + lane][1]
            if inc > W and over is None:
                over = lane
    nb = 64 if over is None else over
    if nb == 64 and b + 63 < nit and ln[b + 63][3]:
        nb = 63
    elif 0 < nb < 64 and ln[b + nb - 1][3]:
        nb += 1
    nb = min(nb, nit - b)
    return nb if nb else (2 if ln[b][3] else 1)


def test_model_cuts_match_exec_model():
    """On liblz4's output for the synthetic (the tools library) and on the
    table: the model's batches are the kernel's lines restated lane by lane
    (kernel_cut), pairs included; and with the extended sequences taken out
    they are scripts/exec_model.py's batches over plain sequences -- the same
    function, given lanes or sequences."""
    import libzseek_amd as z
    em = ec.exec_model
    nfr = 6
    img = z.lz4_seekable(z.synth_buffer(nfr * em.N), em.N)
    c_off, _ = z.seek_table_of(img)
    lists = [[(a, b, o) for a, b, o in em.sequences(img, c_off, f)] for f in range(nfr)]
    assert sum(len(fr) for fr in lists) > 5000
    npairs = 0
    for fr in lists + [ec.seqs_of(RECIPES[n][0]) for n in NAMES if n[0] in "abg"]:
        ln = ec.lanes(fr)
        npairs += sum(x[3] for x in ln)
        plain = [s for s in fr if not ec.lanes([s])[0][3]]
        for W in WS:
            mine = list(ec.batches(ln, W, 64))
            b = 0
            for i, j, _ in mine:
                assert i == b and j - i == kernel_cut(ln, b, W)
                b = j
            assert b == len(ln)
            assert list(ec.batches(ec.lanes(plain), W, 64)) == list(em.batches(plain, W, 64))
    assert npairs > 100


# ---------------------------------------------------------------------------
# the record of the compiled reference reader
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_exec_craft", os.path.join(GOLDEN, "make_exec_craft.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def record(maker):
    with open(os.path.join(GOLDEN, "exec_craft.json")) as f:
        meta = json.load(f)
    assert meta["sha_digits"] == maker.H
    assert [c["name"] for c in meta["cases"]] == [c[0] for c in maker.all_cases()], "regenerate exec_craft.json"
    assert [c["frame_sha"] for c in meta["cases"]] == [maker.sha(c[1]) for c in maker.all_cases()], \
        "regenerate exec_craft.json"
    assert meta["neighbour_frame_shas"] == [maker.sha(f) for f, _ in lz4_craft.NEIGHBOURS]
    assert meta["zstd_neighbour_shas"] == [maker.sha(f) for f, _ in zstd_craft.NEIGHBOURS]
    return meta


def test_reference_reader_record(record, maker):
    """every case between two intact neighbours in a seekable file: the
    compiled reference reader's pread loop, cache 0 and 1, delivered the
    neighbours' and expand's bytes; liblz4 1.9.3 / libzstd 1.4.9 alone decoded
    each frame to expand's bytes"""
    assert os.path.getsize(os.path.join(GOLDEN, "exec_craft.json")) < 1 << 20
    for (fmt, name, frame, dsize, want), rec in zip(maker.all_cases(with_fmt=True), record["cases"]):
        assert rec["lib"] == {"ok": True, "len": dsize, "sha": maker.sha(want)}, name
        a, b = maker.neighbours(fmt)
        for cache in (0, 1):
            ans = rec["reference"][f"cache{cache}"]
            assert ans == {"bytes": len(a) + dsize + len(b), "sha": maker.sha(a + want + b), "last": 0,
                           "error": ""}, (name, cache)


def test_reference_reader_live(ref, record, maker):
    """where the reference is built: run live, it gives the recorded answers"""
    for (fmt, name, frame, dsize, _), rec in zip(maker.all_cases(with_fmt=True), record["cases"]):
        img, total = maker.case_image(fmt, frame, dsize)
        assert maker.ref_answers(ref, img, total) == rec["reference"], name
