"""The zstd census on the CPU (libzseek_amd/csrc/zstd_caps.h and zstd_plan.h
through tests/native/zstd_census_shim.cpp):

- the bounds a device-planned read derives from a file's census (max_frames x
  the largest block count, sequence count and decoded size of any one entry)
  cover every batch the call can plan: any max_frames entries of the file, and
  fewer with padding descriptors behind them -- on the zstd goldens, on a file
  of the many-tiny-block entries the default policy refuses, and on a file of
  random valid entries;
- the default policy does not fit that tiny-block file, which is the case the
  census exists for;
- the census call is declared, exported and bound."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

import zstd_census_util as cu
from conftest import ROOT, golden_file

PADDING = b""          # a padding descriptor's entry: no bytes


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return cu.load(tmp_path_factory.mktemp("zstd_census"))


def _files():
    return [("zstd_64k_direct", None), ("zstd_64k_buffered", None), ("zstd_1m_direct", None),
            ("nofit", cu.nofit_file), ("random_valid", cu.random_file)]


def _image(name, make):
    return make()[0] if make else golden_file(name)


def _fits(shim, plans, max_frames, b):
    """the device's fit check (zstd_fit_kernel) of a batch of max_frames
    descriptors with these plans against the bounds b"""
    assert len(plans) == max_frames
    out_bytes, max_blocks, max_sequences = b
    items, blocks = sum(p[0] for p in plans), sum(p[1] for p in plans)
    return blocks <= max_blocks and items <= shim.zcensus_item_capacity(max_frames, max_blocks, max_sequences)


def test_padding_walks_to_a_bound_of_8(shim):
    assert cu.plan(shim, PADDING) == (8, 0, 0)


def test_bounds_are_the_products(shim):
    cen = dict(zip(cu.FIELDS, (10, 999, 7, 300, 4096, 100)))
    assert cu.bounds(shim, 5, cen) == (5 * 4096, 35, 1500)
    assert cu.bounds(shim, 0, cen) == (0, 0, 0)
    big = dict(cen, max_sequences=1 << 40, max_blocks=1 << 34)
    top = (1 << 64) - 1
    # a product past 64 bits saturates; the item capacity then refuses
    assert cu.bounds(shim, 1 << 30, big) == ((1 << 30) * 4096, top, top)
    assert shim.zcensus_item_capacity(1 << 30, top, top) == top


@pytest.mark.parametrize("name,make", _files(), ids=[f[0] for f in _files()])
def test_census_bounds_cover_every_batch(shim, name, make):
    img = _image(name, make)
    entries, dsizes = cu.seek_table(img)
    n = len(entries)
    assert n >= 2
    plans = [cu.plan(shim, e) for e in entries]
    cen = cu.census(shim, img)
    assert cen["frames"] == n and cen["max_blocks"] >= 1 and cen["max_dsize"] == max(dsizes)
    pad = cu.plan(shim, PADDING)
    by_items = sorted(plans, key=lambda p: -p[0])
    by_blocks = sorted(plans, key=lambda p: -p[1])
    worst = (cen["max_items"], cen["max_blocks"], cen["max_sequences"])      # no entry: all three maxima at once
    rng = np.random.default_rng(5)
    for max_frames in sorted({1, 2, n}):
        b = cu.bounds(shim, max_frames, cen)
        assert b[0] == max_frames * cen["max_dsize"] >= sum(sorted(dsizes)[-max_frames:])
        # the fit check is two inequalities, one on the block total and one on
        # the item total: of all selections of k distinct entries the k with
        # the most blocks and the k with the most items are the worst for each,
        # so these cover every selection; the rest of the batch is padding
        for k in range(0, max_frames + 1):
            tail = [pad] * (max_frames - k)
            assert _fits(shim, by_items[:k] + tail, max_frames, b), (max_frames, k, "items")
            assert _fits(shim, by_blocks[:k] + tail, max_frames, b), (max_frames, k, "blocks")
        # ... and a few drawn at random, as a call would touch them
        for _ in range(20):
            k = int(rng.integers(0, max_frames + 1))
            pick = [plans[i] for i in rng.choice(n, size=k, replace=False)]
            assert _fits(shim, pick + [pad] * (max_frames - k), max_frames, b)
        # beyond anything the file holds: max_frames copies of its worst entry,
        # and of an entry with all three maxima at once
        for w in (by_items[0], by_blocks[0], worst):
            assert _fits(shim, [w] * max_frames, max_frames, b), (max_frames, w)


def test_default_policy_does_not_fit_the_tiny_block_file(shim):
    img, _ = cu.nofit_file()
    entries, dsizes = cu.seek_table(img)
    plans = [cu.plan(shim, e) for e in entries]
    n = len(entries)
    mb, ms = cu.defaults(shim, n, sum(dsizes))
    assert sum(p[1] for p in plans) > mb                     # the whole file as one batch: refused
    assert not _fits(shim, plans, n, (sum(dsizes), mb, ms))
    for e, d in zip(entries, dsizes):                        # ... and every entry alone
        mb1, _ = cu.defaults(shim, 1, d)
        assert cu.plan(shim, e)[1] > mb1
    # (zsk_preadv_device_async's policy: two blocks per frame and one per 16 KiB)
    assert sum(p[1] for p in plans) > sum(2 + d // 16384 for d in dsizes)
    assert _fits(shim, plans, n, cu.bounds(shim, n, cu.census(shim, img)))


def test_census_declared_listed_exported(zs):
    import ctypes as C
    name = "zsk_reader_zstd_census"
    text = open(os.path.join(ROOT, "include", "zseek_hip.h")).read()
    mapped = open(os.path.join(ROOT, "libzseek_amd", "csrc", "libzseek.map")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", zs.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"ZSEEK_EXPORT\s+int\s+%s\s*\(" % name, text)
    assert re.search(r"^\s*%s;" % name, mapped, re.M)
    assert name in zs.EXPORTED and hasattr(zs.lib(), name)
    assert any(ln.split()[-1] == name and ln.split()[-2] == "T" for ln in out.splitlines())
    struct = re.search(r"typedef struct \{([^}]*)\}\s*zsk_zstd_census_t;", text).group(1)
    fields = re.findall(r"(uint64_t|uint32_t)\s+(\w+);", struct)
    assert [f for _, f in fields] == list(cu.FIELDS)
    mirror = [(n, {C.c_uint64: "uint64_t", C.c_uint32: "uint32_t"}[t]) for n, t in zs.ZstdCensusC._fields_]
    assert mirror == [(f, t) for t, f in fields]
    assert C.sizeof(zs.ZstdCensusC) == 40
    assert callable(zs.Reader.zstd_census)
    # the refusals that touch no device
    err = C.create_string_buffer(b"untouched", 80)
    c = zs.ZstdCensusC()
    assert zs.lib().zsk_reader_zstd_census(None, C.byref(c), err) == -1 and err.value == b"invalid reader"
    with zs.Reader(golden_file("zstd_64k_direct"), 0) as r:          # a host image
        assert zs.lib().zsk_reader_zstd_census(r.handle, None, err) == -1 and err.value == b"invalid census pointer"
        with pytest.raises(zs.ZseekError, match="zstd census: needs a device image"):
            r.zstd_census()
