"""The asynchronous zstd decode's capacity arithmetic on the CPU
(libzseek_amd/csrc/zstd_caps.h, through tests/native/zstd_caps_shim.cpp):

- the item capacity of (nframes, max_blocks, max_sequences) covers the sum of
  the plan walk's bounds (zstd_plan.h) of any batch within those counts, the
  walk run over synthetic entries of chosen blocks and sequence counts;
- zsk_zstd_bounds_default, a policy, fits the files this project knows: the
  zstd goldens, the zstd_x2 payloads, the compressor's subset frames and the
  accepted hand-built entries in batches of 64, but for NOFIT;
- the new entries are declared, listed and exported."""
from __future__ import annotations

import hashlib
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import zstd_caps_util as zu
import zstd_craft as zc
from conftest import GOLDEN, ROOT, golden_file

NEW = ["zsk_zstd_bounds_default", "zsk_zstd_decode_frames_async", "zsk_reader_set_zstd_async"]

# accepted entries of zstd_craft.CASES that the default bounds do not fit, each
# for the same reason: many tiny blocks -- 1,001 and 40 block headers in an
# entry that decodes to under 2 KiB, against two per entry plus one per 16 KiB
NOFIT = ("b_1000_empty_raw", "b_1000_empty_then_seqs", "h_40frames", "h_40frames_skips")


@pytest.fixture(scope="module")
def caps(tmp_path_factory):
    return zu.load(tmp_path_factory.mktemp("zstd_caps"))


# -- the item capacity -------------------------------------------------------------
def synth_entry(blocks) -> bytes:
    """a frame whose compressed blocks declare the given sequence counts (raw
    literals of size 0, then the count in its shortest form or, for a pair (n,
    form), the form asked for): all the plan walk reads"""
    out = bytearray(zc.MAGIC + bytes([0x20, 0]))      # single segment, 1-byte content size
    for i, b in enumerate(blocks):
        n, form = b if isinstance(b, tuple) else (b, None)
        body = bytes([0]) + zc.nseq_bytes(n, form)
        body += bytes(max(0, 3 - len(body)))
        out += (int(i + 1 == len(blocks)) | 2 << 1 | len(body) << 3).to_bytes(3, "little") + body
    return bytes(out)


def want_bound(blocks) -> int:
    items = 8
    for b in blocks:
        n = b[0] if isinstance(b, tuple) else b
        items += 4 + 2 * n + (2 * n + 62) // 63
    return (items + 3) & ~3


def check_batch(caps, batch):
    """batch: per frame its blocks' sequence counts"""
    entries = [synth_entry(f) for f in batch]
    items, blocks, seqs = zu.totals(caps, entries)
    counts = [b[0] if isinstance(b, tuple) else b for f in batch for b in f]
    assert (blocks, seqs) == (len(counts), sum(counts))
    assert items == sum(want_bound(f) for f in batch)
    cap = caps.zcaps_item_capacity(len(batch), blocks, seqs)
    assert cap >= items, (len(batch), blocks, seqs)
    # derived, not padded: at most the rounding and one pad slot per block with sequences
    assert cap - items <= 3 * len(batch) + min(blocks, seqs)
    # (bounds above the batch's counts cover it too)
    assert caps.zcaps_item_capacity(len(batch), blocks + 7, seqs + 100) >= cap


def test_walk_reads_the_synthetic_entries(caps):
    e = synth_entry([0, 1, 127, 128, 0x7EFF, 0x7F00, 0x7F00 + 65535])
    bound, blocks, cks, seqs = zu.plan(caps, e)
    assert (blocks, cks, seqs) == (7, False, 1 + 127 + 128 + 0x7EFF + 2 * 0x7F00 + 65535)
    assert bound == want_bound([0, 1, 127, 128, 0x7EFF, 0x7F00, 0x7F00 + 65535])


def test_item_capacity_covers_random_batches(caps):
    rng = np.random.default_rng(20260)
    edges = [0, 1, 2, 31, 32, 63, 64, 127, 128, 0x7EFF, 0x7F00, 0x7F00 + 65535]
    for trial in range(60):
        nframes = int(rng.integers(1, 301))
        batch = []
        for _ in range(nframes):
            nb = int(rng.integers(1, 9))
            kind = rng.integers(0, 4)
            if kind == 0:
                f = [int(rng.choice(edges[:9])) for _ in range(nb)]
            elif kind == 1:
                f = [int(rng.integers(0, 400)) for _ in range(nb)]
            elif kind == 2:
                f = [int(rng.choice(edges)) for _ in range(min(nb, 2))]
            else:
                f = [1] * nb
            batch.append(f)
        check_batch(caps, batch)


def test_item_capacity_edges(caps):
    check_batch(caps, [[0]] * 300)                           # no sequences at all
    check_batch(caps, [[0] * 40] * 7)
    check_batch(caps, [[1] * 1000])                          # a pad slot per block: the worst case
    check_batch(caps, [[1] * 50] * 300)
    check_batch(caps, [[31, 32] * 20] * 9)                   # 2 n = 62, 64: either side of a pad slot
    check_batch(caps, [[0x7F00], [0x7F00 + 65535], [0x7F00 - 1]])
    check_batch(caps, [[(5, 2), (0, 2), (127, 2), (130, 2)]])  # short counts in the two-byte form
    check_batch(caps, [[0x7F00 + 65535] * 8] * 3)


def test_no_wrap_at_a_tebibyte(caps):
    out_bytes = 1 << 40
    for nframes in (1, 1 << 24, (1 << 32) - 1):
        mb, ms = zu.defaults(caps, nframes, out_bytes)
        assert (mb, ms) == (2 * nframes + out_bytes // 16384, out_bytes // 3)
        want = 11 * nframes + 4 * mb + 2 * ms + 2 * ms // 63 + min(mb, ms)
        assert want < 1 << 64 and caps.zcaps_item_capacity(nframes, mb, ms) == want
    assert caps.zcaps_item_capacity(1, 1 << 60, 0) == (1 << 64) - 1     # refused, not wrapped
    assert caps.zcaps_item_capacity(1, 0, 1 << 62) == (1 << 64) - 1


# -- the default bounds on real files --------------------------------------------------
def seek_table(img: bytes):
    """(entries, decoded sizes) of a seekable file, from its footer"""
    assert img[-4:] == (0x8F92EAB1).to_bytes(4, "little")
    n, flags = int.from_bytes(img[-9:-5], "little"), img[-5]
    step = 12 if flags & 0x80 else 8
    at = len(img) - 9 - step * n
    entries, dsizes, c = [], [], 0
    for i in range(n):
        cs, ds = int.from_bytes(img[at: at + 4], "little"), int.from_bytes(img[at + 4: at + 8], "little")
        entries.append(img[c: c + cs])
        dsizes.append(ds)
        c, at = c + cs, at + step
    return entries, dsizes


def assert_defaults_fit(caps, entries, dsizes, what):
    mb, ms = zu.defaults(caps, len(entries), sum(dsizes))
    items, blocks, seqs = zu.totals(caps, entries)
    assert blocks <= mb and seqs <= ms and items <= caps.zcaps_item_capacity(len(entries), mb, ms), \
        (what, len(entries), sum(dsizes), blocks, mb, seqs, ms, items)


@pytest.mark.parametrize("name", ["zstd_64k_direct", "zstd_64k_buffered", "zstd_1m_direct"])
def test_defaults_fit_the_goldens(caps, name):
    entries, dsizes = seek_table(golden_file(name))
    assert len(entries) >= 2 and zu.totals(caps, entries)[2] > 0
    assert_defaults_fit(caps, entries, dsizes, name)
    for e, d in zip(entries, dsizes):          # ... and entry by entry
        assert_defaults_fit(caps, [e], [d], name)


def test_defaults_fit_the_x2_payloads(caps):
    meta = json.load(open(os.path.join(GOLDEN, "zstd_x2.json")))
    blob = open(os.path.join(GOLDEN, "zstd_x2.bin"), "rb").read()
    fa, fb = (bytes.fromhex(h) for h in meta["neighbour_frames_hex"])
    da, db = meta["neighbours"]["a"]["dsize"], meta["neighbours"]["b"]["dsize"]
    assert len(meta["cases"]) >= 10
    for i, c in enumerate(meta["cases"]):
        e = blob[c["off"]: c["off"] + c["len"]]
        assert_defaults_fit(caps, [e], [c["dsize"]], i)
        assert_defaults_fit(caps, [fa, e, fb], [da, c["dsize"], db], i)


def test_defaults_fit_the_compressors_subset(caps, tmp_path):
    spec = importlib.util.spec_from_file_location("make_zstd_enc_subset", os.path.join(GOLDEN, "make_zstd_enc_subset.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    want = json.load(open(os.path.join(GOLDEN, "zstd_enc_subset.json")))
    enc = mk.load_shim(tmp_path)
    seen = 0
    for name, content, ck in mk.inputs():
        src = np.frombuffer(content, np.uint8) if content else np.zeros(1, np.uint8)
        cap = enc.zenc_frame_bound(len(content))
        out = np.empty(cap, np.uint8)
        n = enc.zenc_compress(src.ctypes.data, len(content), ck, out.ctypes.data, cap)
        frame = out[:n].tobytes()
        assert hashlib.sha256(frame).hexdigest() == want[name]["sha256"], name
        assert zu.plan(caps, frame)[1] >= 1
        assert_defaults_fit(caps, [frame], [len(content)], name)
        seen += 1
    assert seen == len(want)


def test_defaults_fit_the_craft_batches(caps):
    ok = [c for c in zc.CASES if c[4] == 0]
    assert len(NOFIT) <= 8 and set(NOFIT) <= {c[0] for c in ok}
    for name in NOFIT:                       # the list is what it says: each alone does not fit
        c = zc.CASE[name]
        mb, ms = zu.defaults(caps, 1, c[2])
        assert zu.plan(caps, c[1])[1] > mb, name
    fit = [c for c in ok if c[0] not in NOFIT]
    assert len(fit) == len(ok) - len(NOFIT)
    for lo in range(0, len(fit), 64):
        part = fit[lo: lo + 64]
        assert_defaults_fit(caps, [c[1] for c in part], [c[2] for c in part], lo)


# -- the interface ------------------------------------------------------------------------
def test_async_entries_declared_listed_exported(zs):
    text = open(os.path.join(ROOT, "include", "zseek_hip.h")).read()
    mapped = open(os.path.join(ROOT, "libzseek_amd", "csrc", "libzseek.map")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", zs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"ZSEEK_EXPORT\s+\w+\s+%s\s*\(" % name, text), name
        assert re.search(r"^\s*%s;" % name, mapped, re.M), name
        assert name in zs.EXPORTED and hasattr(zs.lib(), name)
        assert any(ln.split()[-1] == name and ln.split()[-2] == "T" for ln in out.splitlines()), name
    assert re.search(r"#define\s+ZSK_ERR_SCRATCH\s+105\b", text)
    assert zs.ERR_SCRATCH == 105 and zs.status_string(105).startswith("ERROR_")
    for field in ("out_bytes", "max_blocks", "max_sequences"):
        assert re.search(r"uint64_t\s+%s;" % field, text), field
    # the library's defaults are the header's arithmetic
    assert zs.zstd_bounds_default(64, 1 << 20) == {"out_bytes": 1 << 20, "max_blocks": 128 + 64,
                                                  "max_sequences": (1 << 20) // 3}
    L = zs.lib()
    # NULL bounds: -1; no frames: 0, nothing queued (no device is touched)
    assert L.zsk_zstd_decode_frames_async(None, 0, None, None, None, None, None) == -1
    b = zs.ZstdBoundsC(0, 0, 0)
    import ctypes as C
    assert L.zsk_zstd_decode_frames_async(None, 0, None, None, None, C.byref(b), None) == 0
    assert L.zsk_reader_set_zstd_async(None, 3) is False
