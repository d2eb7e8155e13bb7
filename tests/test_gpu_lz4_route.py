"""Bytes at the routing boundaries (csrc/lz4_route.h): zsk_lz4_decode_frames
under its own choice of route at the batch sizes where the choice changes --
the one-frame route's last batch and the first past it (64, 65), the block
route's bounds (1023, 1024; 32767, 32768 -- where the chunk parse's size bound
moves too).  Hand-built tiny frames of tests/lz4_craft.py repeated; the batches
of <= 65 frames also hold a frame of more than 64 KiB (the one-frame route's
big-frame kernels; past it the wave execute) and a refused frame.  Outputs go
into 0xA5-prefilled buffers; statuses and bytes are held to the CPU oracle,
which decodes each distinct frame once."""
from __future__ import annotations

import numpy as np
import pytest

import lz4_craft as lc

pytestmark = pytest.mark.gpu

TINY = [lc.NEIGHBOURS[1]] + [(lc.CASE[n][1], lc.CASE[n][3]) for n in ("e_items16", "e_items17", "c_off0_second")]
BIG = lc.CASE["d_linked_65535_block2"]       # two linked blocks, 65,549 bytes
REFUSED = lc.CASE["g_lit_count_one_more"]
FILL = 0xA5


@pytest.fixture(scope="module")
def distinct(oracle):
    """(frame, declared size) -> (accepted, bytes), one oracle decode each"""
    out = {}
    for f, ds in [(f, len(b)) for f, b in TINY] + [(BIG[1], BIG[2]), (REFUSED[1], REFUSED[2])]:
        st, data, _, _ = oracle.decode_frame(f, ds)
        out[(f, ds)] = (st == 0 and len(data) == ds, data)
    assert [ok for ok, _ in out.values()] == [True] * 5 + [False]
    assert all(len(f) < 200 for f, _ in TINY) and BIG[2] > 65536
    return out


@pytest.mark.parametrize("n", [64, 65, 1023, 1024, 32767, 32768])
def test_auto_route_at_a_boundary(gpu, zs, distinct, n):
    import torch
    frames = [(TINY[i % 4][0], len(TINY[i % 4][1])) for i in range(n)]
    if n <= 65:
        frames[5] = (BIG[1], BIG[2])
        frames[n - 2] = (REFUSED[1], REFUSED[2])
    c = np.cumsum([0] + [len(f) for f, _ in frames])
    d = np.cumsum([0] + [ds for _, ds in frames])
    desc = np.zeros(n, zs.FRAME_DESC_DTYPE)
    desc["c_off"], desc["d_off"], desc["c_size"], desc["d_size"] = c[:-1], d[:-1], np.diff(c), np.diff(d)
    comp = torch.zeros(int(c[-1]) + 256, dtype=torch.uint8, device=gpu)
    comp[: int(c[-1])].copy_(torch.from_numpy(np.frombuffer(b"".join(f for f, _ in frames), np.uint8).copy()))
    out = torch.full((int(d[-1]) + 64,), FILL, dtype=torch.uint8, device=gpu)
    status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    zs.decode_frames(torch.from_numpy(desc.view(np.uint8).copy()).to(gpu), comp, out, status)
    torch.cuda.synchronize()
    accepted = np.array([distinct[fr][0] for fr in frames])
    st = status.cpu().numpy()
    assert ((st == 0) == accepted).all(), [(i, zs.status_string(int(st[i]))) for i in np.nonzero((st == 0) != accepted)[0][:8]]
    # an accepted frame's slot holds its bytes; a refused frame's is not looked at; nothing past the last slot
    want = np.frombuffer(b"".join(distinct[fr][1] if distinct[fr][0] else bytes(fr[1]) for fr in frames), np.uint8)
    look = np.repeat(accepted, np.diff(d))
    got = out.cpu().numpy()
    bad = np.nonzero((got[: int(d[-1])] != want) & look)[0]
    assert bad.size == 0, (bad[:8], bad.size)
    assert (got[int(d[-1]):] == FILL).all()
