"""tests/lz4_craft.py's hand-built LZ4 frames on the CPU: the table's own
verdicts and expected bytes (expand, a byte-by-byte model), the oracle
(oracle/lz4_oracle.c) and the record of liblz4 1.9.3 and the compiled
reference reader (tests/golden/lz4_craft.json, made by make_lz4_craft.py)
must all say the same about every frame.  The GPU engines are held to the
same table in test_gpu_lz4_craft.py."""
from __future__ import annotations

import importlib.util
import json
import os

import pytest

import lz4_craft
from conftest import GOLDEN, sha
from test_cpu import _oracle_error

CASES = lz4_craft.CASES


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "lz4_craft.json")) as f:
        meta = json.load(f)
    assert [c["name"] for c in meta["cases"]] == [c[0] for c in CASES], "regenerate lz4_craft.json"
    assert [c["frame_sha"] for c in meta["cases"]] == [sha(c[1]) for c in CASES], "regenerate lz4_craft.json"
    assert meta["neighbour_frame_shas"] == [sha(f) for f, _ in lz4_craft.NEIGHBOURS]
    return meta


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_lz4_craft", os.path.join(GOLDEN, "make_lz4_craft.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_table_shape():
    """270 cases, 235 accepted and 35 rejected; every boundary pair has its
    accepted and its rejected member (so an edit cannot quietly turn the table
    all-accepted); frames are small but for the few that must reach a block's
    capacity or 65535 bytes back."""
    ok = [c for c in CASES if c[3] is not None]
    assert (len(CASES), len(ok)) == (270, 235)
    assert len(lz4_craft.PAIRS) == 22
    for good, bad in lz4_craft.PAIRS:
        assert lz4_craft.CASE[good][3] is not None and lz4_craft.CASE[bad][3] is None, (good, bad)
    assert all(len(c[3]) == c[2] for c in ok)
    assert sum(len(c[1]) > 8192 for c in CASES) <= 16
    for fam in "abcdefg":
        assert any(c[0].startswith(fam + "_") for c in CASES), fam
    for fam in "adfg":
        assert any(c[0].startswith(fam + "_") and c[3] is None for c in CASES), fam


def test_seq_encoding():
    """the encoder itself, on the format's documented examples: nibbles, the
    0 byte that ends a chain at 15 + 255 k, little-endian offsets"""
    assert lz4_craft.seq(b"abc", 1, 4) == b"\x30abc\x01\x00"
    assert lz4_craft.seq(b"", 0x1234, 19) == b"\x0f\x34\x12\x00"
    assert lz4_craft.seq(b"", 2, 529) == b"\x0f\x02\x00\xff\xff\x00"
    assert lz4_craft.seq(b"x" * 270)[:3] == b"\xf0\xff\x00" and len(lz4_craft.seq(b"x" * 270)) == 273
    assert lz4_craft.seq(b"x" * 15, 3, 18)[:2] == b"\xfe\x00"
    assert lz4_craft.expand([(b"ab", 2, 5), (b"", 0, 2), (b"z", None, None)]) == b"abababa\0\0z"
    assert lz4_craft.expand([(b"a", 1, 4)], bytearray(b"q")) == b"qaaaaa"


def test_liblz4_verdicts_match_table(record):
    """liblz4 1.9.3 accepts exactly the cases the table calls accepted (the
    frame decodes and to the declared size), to expand's bytes"""
    for (name, _, dsize, want), rec in zip(CASES, record["cases"]):
        lz = rec["lz4f"]
        assert (lz["ok"] and lz["len"] == dsize) == (want is not None), name
        if want is not None:
            assert lz["sha"] == sha(want), name


def test_oracle_matches_liblz4(oracle, record):
    """Every case: the oracle's status and error name on the frame alone are
    liblz4's; every accepted case: its bytes are expand's and the record's."""
    for (name, frame, dsize, want), rec in zip(CASES, record["cases"]):
        lz = rec["lz4f"]
        st, got, _, _ = oracle.decode_frame(frame, record["lz4f_cap"])
        assert (st == 0) == lz["ok"], name
        assert oracle.error_name(st) == (lz["error"] or "OK_NoError"), name
        if st == 0:
            assert len(got) == lz["len"] and sha(got) == lz["sha"], name
        st, got, _, _ = oracle.decode_frame(frame, dsize)
        assert (st == 0 and len(got) == dsize) == (want is not None), name
        if want is not None:
            assert got == want, name


def _oracle_loop(oracle, img, total, cache, dsizes):
    """the reference reader under a caller's loop, derived from the oracle's
    decode of each frame (test_cpu.py's _oracle_error): one frame per call"""
    got, pos = b"", 0
    st = oracle.seek_table(img)
    for i, dsz in enumerate(dsizes):
        err = _oracle_error(oracle, img, cache, pos, total - pos)
        if err is not None:
            return {"bytes": len(got), "sha": sha(got), "last": -1, "error": err}
        c0, c1 = int(st["c_off"][i]), int(st["c_off"][i + 1])
        got += oracle.decode_frame(img[c0:c1], dsz)[1]
        pos += dsz
    return {"bytes": len(got), "sha": sha(got), "last": 0, "error": ""}


def test_oracle_matches_reference_reader(oracle, record, maker):
    """Every case between its two neighbours in a seekable file: the oracle's
    decode and test_cpu.py's error rule give the recorded answers of the
    reference reader's pread loop, cache 0 and 1 -- for accepted cases the
    neighbours' and expand's bytes.  (The reference spins on a frame whose
    seek-table size disagrees with what it decodes: recorded as "hang".)"""
    (_, a), (_, b) = lz4_craft.NEIGHBOURS
    hangs = []
    for (name, frame, dsize, want), rec in zip(CASES, record["cases"]):
        if rec["reference"] == "hang":
            hangs.append(name)
            continue
        img, total = maker.case_image(frame, dsize)
        for cache in (0, 1):
            ans = rec["reference"][f"cache{cache}"]
            assert _oracle_loop(oracle, img, total, cache, [len(a), dsize, len(b)]) == ans, (name, cache)
            if want is not None:
                assert (ans["bytes"], ans["last"], ans["sha"]) == (total, 0, sha(a + want + b)), (name, cache)
            else:
                assert (ans["bytes"], ans["last"]) == (len(a), -1), (name, cache)
    assert hangs == ["f_dsize_plus1", "f_dsize_minus1", "f_dsize_minus1_literals"]


def test_reference_reader_live(ref, record, maker):
    """where the reference is built: run live, it gives the recorded answers"""
    for (name, frame, dsize, _), rec in zip(CASES, record["cases"]):
        if rec["reference"] != "hang":
            img, total = maker.case_image(frame, dsize)
            assert maker.ref_answers(ref, img, total) == rec["reference"], name


def test_liblz4_live(record, maker):
    """where liblz4 1.9.3 is installed: run live, it gives the recorded verdicts"""
    lz = maker.load_lz4()
    if lz is None or lz.LZ4_versionNumber() != 10903:
        pytest.skip("liblz4 1.9.3 not installed")
    for (name, frame, _, _), rec in zip(CASES, record["cases"]):
        err, got = maker.lz4f_decode(lz, frame)
        assert {"ok": err == "", "error": err, "len": len(got), "sha": sha(got) if err == "" else ""} == rec["lz4f"], name


def test_random_valid(oracle):
    """the generator's contract: the oracle accepts 2000 of 2000 frames, to
    expand's bytes; frames decode to at most 4 KiB; it is deterministic and
    reaches the edges it is biased to"""
    frames = lz4_craft.random_valid(1, 2000)
    assert len(frames) == 2000
    accepted = 0
    for f, want in frames:
        st, got, _, _ = oracle.decode_frame(f, len(want))
        accepted += st == 0 and got == want
    assert accepted == 2000
    assert max(len(w) for _, w in frames) <= 4096
    assert frames[:50] == lz4_craft.random_valid(1, 50)
    assert len({f for f, _ in frames}) > 1500
    assert any(len(w) == 0 for _, w in frames) and sum(len(w) > 1024 for _, w in frames) > 100
