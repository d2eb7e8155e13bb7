"""zsk_zstd_decode_frames_async on the GPU: the zstd decode queued on the
caller's stream with no wait for its plan, its scratch sized from bounds and
its plan checked against them on the device.

The yardsticks are test_gpu_zstd_craft.py's: tests/zstd_craft.py's hand-built
entries, expand's bytes and libzstd 1.4.9's recorded error code per entry.
The bounds come from the plan walk on the CPU (tests/native/zstd_caps_shim.cpp
over zstd_plan.h): exact block and sequence counts, so the capacity arithmetic
of zstd_caps.h is held to its tightest case, and one less where the device
must refuse.  A refused batch has ZSK_ERR_SCRATCH in every status and leaves a
sentinel-filled output as it was."""
from __future__ import annotations

import time

import numpy as np
import pytest

import zstd_caps_util as zu
import zstd_craft as zc
from zstd_craft import CASES, DIVERGENT, DIVERGENT_BYTES, SHORT, ZSK_STATUS_ZSTD

pytestmark = pytest.mark.gpu

SENT = 0xA5
ZSK_ERR_SHORT_FRAME = 101
ZSK_ERR_SCRATCH = 105
RAW8 = zc.A                       # one raw block of 8 bytes: no Huffman literals, no sequences


def want_status(c) -> int:
    if c[0] in DIVERGENT:
        return DIVERGENT[c[0]]
    if c[3] is not None:
        return 0
    return ZSK_ERR_SHORT_FRAME if c[4] == SHORT else ZSK_STATUS_ZSTD | c[4]


def want_bytes(c):
    return c[3] if c[3] is not None else DIVERGENT_BYTES.get(c[0])


def accepted(c) -> bool:
    return want_status(c) == 0 and want_bytes(c) is not None


SMALL = [c for c in CASES if c[2] <= 4096 and len(c[1]) <= 8192]


@pytest.fixture(scope="module")
def caps(tmp_path_factory):
    return zu.load(tmp_path_factory.mktemp("zstd_caps_gpu"))


@pytest.fixture(scope="module")
def plans(caps):
    """case name -> (bound, blocks, cks, sequences), walked once"""
    return {c[0]: zu.plan(caps, c[1]) for c in CASES}


def exact(plans, batch) -> dict:
    return {"out_bytes": sum(c[2] for c in batch), "max_blocks": sum(plans[c[0]][1] for c in batch),
            "max_sequences": sum(plans[c[0]][3] for c in batch)}


class Batch:
    """entries back to back in device memory, a sentinel-filled output"""

    def __init__(self, zs, gpu, entries, dsizes):
        import torch
        n = len(entries)
        c = np.cumsum([0] + [len(f) for f in entries])
        self.d = np.cumsum([0] + list(dsizes))
        desc = np.zeros(n, zs.FRAME_DESC_DTYPE)
        desc["c_off"], desc["d_off"] = c[:-1], self.d[:-1]
        desc["c_size"], desc["d_size"] = np.diff(c), np.asarray(dsizes)
        self.td = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
        self.comp = torch.zeros(int(c[-1]) + 256, dtype=torch.uint8, device=gpu)
        self.comp[: int(c[-1])].copy_(torch.from_numpy(np.frombuffer(b"".join(entries), np.uint8).copy()))
        self.out = torch.full((int(self.d[-1]) + 64,), SENT, dtype=torch.uint8, device=gpu)
        self.status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
        self.n = n
        torch.cuda.synchronize()

    def go(self, zs, bounds, stream=None):
        zs.zstd_decode_frames_async(self.td, self.comp, self.out, self.status, bounds,
                                    stream.cuda_stream if stream is not None else None)

    def results(self):
        o = self.out.cpu().numpy()
        assert (o[int(self.d[-1]):] == SENT).all(), "bytes past the output were written"
        return [o[int(self.d[i]): int(self.d[i + 1])].tobytes() for i in range(self.n)], self.status.cpu().tolist()

    def untouched(self) -> bool:
        return bool((self.out == SENT).all().item())

    def reset(self, stream):
        import torch
        with torch.cuda.stream(stream):
            self.out.fill_(SENT)
            self.status.fill_(-1)


def run_cases(zs, gpu, batch, bounds):
    import torch
    b = Batch(zs, gpu, [c[1] for c in batch], [c[2] for c in batch])
    b.go(zs, bounds)
    torch.cuda.synchronize()
    got, st = b.results()
    bad = [(i, c[0], zs.status_string(s), zs.status_string(want_status(c)))
           for i, (c, s) in enumerate(zip(batch, st)) if s != want_status(c)]
    bad += [(i, c[0], "bytes differ") for i, (c, g) in enumerate(zip(batch, got)) if accepted(c) and g != want_bytes(c)]
    # a rejected entry's neighbours are untouched; its own bytes past what it decoded stay the sentinel's too
    if bad:
        print(len(bad), "wrong:", bad[:20])
    return bad


# ---------------------------------------------------------------------------
# every crafted case
# ---------------------------------------------------------------------------
def test_one_frame_route(gpu, zs, plans):
    """batches of 64 or fewer (the fused one-frame route), exact bounds"""
    bad = []
    for at in range(0, len(CASES), 64):
        part = CASES[at: at + 64]
        bad += run_cases(zs, gpu, part, exact(plans, part))
    assert not bad, bad[:12]


def test_lane_route_boundary(gpu, zs, plans):
    """65 entries: the first batch size past the one-frame route"""
    part = CASES[100: 165]
    assert len(part) == 65 and sum(not accepted(c) for c in part) > 3
    bad = run_cases(zs, gpu, part, exact(plans, part))
    assert not bad, bad[:12]


def test_all_cases_one_batch(gpu, zs, plans):
    bad = run_cases(zs, gpu, CASES, exact(plans, CASES))
    assert not bad, bad[:12]


@pytest.mark.parametrize("n", [4096 + 130, 16384 + 130])
def test_chunked_batches(gpu, zs, plans, n):
    """a seeded shuffle of the small cases past 4,096 entries (two pipelined
    chunks) and past 16,384 (three): every chunk's Huffman grid covers the
    whole call's block capacity and takes its own range from device memory"""
    rng = np.random.default_rng(n)
    pool = [SMALL[i] for i in rng.permutation(len(SMALL))]
    pool += [SMALL[i] for i in rng.integers(0, len(SMALL), n - len(pool))]
    assert len(pool) == n and sum(not accepted(c) for c in pool) > n // 10
    t0 = time.time()
    bad = run_cases(zs, gpu, pool, exact(plans, pool))
    print(f"n = {n}: {time.time() - t0:.2f} s")
    assert not bad, bad[:12]


# ---------------------------------------------------------------------------
# no jobs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 70])
def test_entries_without_blocks(gpu, zs, caps, n):
    """only a skippable frame per entry: no block slot, no job, no op but the
    end -- with exact bounds (no block at all) and with the defaults"""
    import torch
    c = zc.CASE["h_skippable_only"]
    assert zu.plan(caps, c[1])[1] == 0 and want_status(c) == 0
    for bounds in ({"out_bytes": n * c[2], "max_blocks": 0, "max_sequences": 0}, None):
        b = Batch(zs, gpu, [c[1]] * n, [c[2]] * n)
        b.go(zs, bounds)
        torch.cuda.synchronize()
        got, st = b.results()
        assert st == [0] * n and got == [want_bytes(c)] * n


@pytest.mark.parametrize("n", [10, 70])
def test_no_huffman_literals_anywhere(gpu, zs, caps, n):
    """raw blocks alone: zero Huffman jobs against a grid sized for the
    default bounds' 2 n blocks (one-frame route and lane route)"""
    import torch
    assert zu.plan(caps, RAW8)[1:] == (1, False, 0)
    b = Batch(zs, gpu, [RAW8] * n, [8] * n)
    bounds = zs.zstd_bounds_default(n, 8 * n)
    assert bounds["max_blocks"] == 2 * n
    b.go(zs, bounds)
    torch.cuda.synchronize()
    got, st = b.results()
    assert st == [0] * n and got == [b"abcdefgh"] * n


def test_chunk_without_huffman_beside_one_with(gpu, zs, plans, caps):
    """two chunks: the first all raw blocks (its job range is empty), the
    second the small cases, Huffman literals among them"""
    n = 4096 + 130
    rng = np.random.default_rng(7)
    raw = ("raw8", RAW8, 8, b"abcdefgh", 0)
    second = [SMALL[i] for i in rng.integers(0, len(SMALL), n - n // 2)]
    assert any("huf" in c[0] and accepted(c) for c in second)
    pool = [raw] * (n // 2) + second
    p = dict(plans)
    p["raw8"] = zu.plan(caps, RAW8)
    bad = run_cases(zs, gpu, pool, exact(p, pool))
    assert not bad, bad[:12]


# ---------------------------------------------------------------------------
# the fit boundary
# ---------------------------------------------------------------------------
def test_fit_boundary(gpu, zs, caps, plans):
    """about 40 small accepted cases with sequences.  Exact bounds decode all;
    one block less, no sequences, or an output one byte short refuse the whole
    call: ZSK_ERR_SCRATCH everywhere, the sentinel-filled output unchanged;
    the call after each refusal, same stream, exact bounds, is bit-exact."""
    import torch
    part = [c for c in SMALL if accepted(c) and plans[c[0]][3] >= 2][:40]
    assert len(part) == 40
    ex = exact(plans, part)
    entries = [c[1] for c in part]
    assert zu.fits(caps, entries, ex["out_bytes"], ex["max_blocks"], ex["max_sequences"])
    assert not zu.fits(caps, entries, ex["out_bytes"], ex["max_blocks"], 0), "the batch needs its sequences' items"
    S = torch.cuda.Stream(device=gpu)
    b = Batch(zs, gpu, entries, [c[2] for c in part])
    want = ([want_bytes(c) for c in part], [0] * len(part))
    b.go(zs, ex, S)
    S.synchronize()
    assert b.results() == want
    for tight in (dict(ex, max_blocks=ex["max_blocks"] - 1), dict(ex, max_sequences=0),
                  dict(ex, out_bytes=ex["out_bytes"] - 1)):
        b.reset(S)
        b.go(zs, tight, S)
        S.synchronize()
        assert b.status.cpu().tolist() == [ZSK_ERR_SCRATCH] * len(part), tight
        assert b.untouched(), tight
        b.reset(S)
        b.go(zs, ex, S)                     # (no host wait in between: the refusal left the stream usable)
        S.synchronize()
        assert b.results() == want, tight


# ---------------------------------------------------------------------------
# no host wait
# ---------------------------------------------------------------------------
def test_async_returns_before_its_work_runs(gpu, zs, plans):
    """two decodes queued back to back on one stream behind >= 0.25 s of
    queued work: both calls return while an event recorded before them is
    still pending.  A third call goes on a second stream meanwhile.  All three
    are bit-exact once the streams drain."""
    import torch
    from test_gpu_preadv_async import _busy_work
    part = [c for c in SMALL if accepted(c)][:150]       # the lane route
    ex = exact(plans, part)
    entries, dsizes = [c[1] for c in part], [c[2] for c in part]
    S, S2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    bs = [Batch(zs, gpu, entries, dsizes) for _ in range(4)]
    queue = _busy_work(gpu, S, 0.25)
    ev = torch.cuda.Event()
    torch.cuda.synchronize()
    bs[0].go(zs, ex, S)                                   # warm-up: the pooled scratch is grown
    S.synchronize()
    queue()
    ev.record(S)
    bs[1].go(zs, ex, S)
    bs[2].go(zs, ex, S)
    pending = not ev.query()
    bs[3].go(zs, ex, S2)
    assert pending, "a call waited for the stream"
    S.synchronize()
    S2.synchronize()
    want = ([want_bytes(c) for c in part], [0] * len(part))
    for b in bs:
        assert b.results() == want
