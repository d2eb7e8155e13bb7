"""The lean parse's byte ring at its wrap (lz4_lean.hip, lean_ring.h): frames
hand-built with tests/lz4_craft.py so that chosen bytes of a sequence sit on
chosen ring positions, through `engine="lean"` (lz4_lean_pair_kernel) and
`engine="block"` (the single-wave lz4_lean_kernel), every frame's bytes and
status against the CPU decoder.

A frame byte b of frame f lies at ring position (cx0 + b) % R, where cx0 is
the frame's offset from its wave's first frame, rounded down to the 32-byte
line of that first frame (lane_setup).  The builder knows the batch layout, so
it sizes a prefix of short sequences (at least one lap long) to put an anchor
byte on a target position -- for R = 256, 288 and 320, whichever the kernels
are built with:

  * the token, the literal-extension byte, each offset byte and the
    match-extension byte of one sequence on positions R-3 .. R+1 in turn;
  * literal runs of R-17, R-16, R-15, R, R+1, 2R and 2R+31 bytes (the fast
    step's literal half, the fill's jump), placed after the prefix as it
    comes and again with the offset word at position 1: a jump that restarts
    the fill at position 0, the mirrored piece;
  * 300 one-byte-literal sequences, two laps and more;
  * a block and a frame ending exactly at the wrap.

One block of at most 8 KiB decoded per frame; batches of 1, 64, 65 and 257
frames (a partial wave, a full one, two waves, a second workgroup)."""
from __future__ import annotations

import pytest

import lz4_craft
from lz4_craft import lits

pytestmark = pytest.mark.gpu

RINGS = (256, 288, 320)
HEAD = 11          # frame header (7) + block header (4): the block's first token
BATCHES = (1, 64, 65, 257)


def _prefix(nbytes: int, salt: int):
    """short sequences that take exactly nbytes (>= 22) of the block"""
    assert nbytes >= 22
    seqs = [(lits(8, salt), 8, 4)]                     # 11 bytes
    left = nbytes - 11
    while left > 17:
        seqs.append((lits(4, salt + len(seqs)), 3, 4))  # 7 bytes
        left -= 7
    seqs.append((lits(left - 3, salt + 1), 5, 4))      # 11..17 bytes
    return seqs


def _size(seqs) -> int:
    return sum(len(lz4_craft.seq(*s)) for s in seqs)


TAIL = (lits(16, 5), None, None)


def _specs():
    """(name, R, body sequences, anchor byte offset within the body, target
    position); the anchor may lie past the body (the frame's end)"""
    out = []
    for R in RINGS:
        probe = (lits(20, 3), 17, 30)   # token, 1 literal-extension byte, 20 literals, offset, 1 match-extension byte
        fields = {"token": 0, "lext": 1, "off0": 22, "off1": 23, "mext": 24}
        assert len(lz4_craft.seq(*probe)) == 25
        for fname, delta in fields.items():
            for t in range(R - 3, R + 2):
                out.append((f"{fname}@{t}/{R}", R, [probe, (lits(3, 1), 2, 9), TAIL], delta, t % R))
        for run in (R - 17, R - 16, R - 15, R, R + 1, 2 * R, 2 * R + 31):
            body = [(lits(run, 7), 40, 6), (lits(2, 2), 1, 20), TAIL]
            q = len(lz4_craft.seq(*body[0])) - 2   # the run's offset word (no match extension)
            out.append((f"run{run}/{R}", R, body, 0, None))
            out.append((f"run{run}->1/{R}", R, body, q, 1))
        ones = [(lits(1, i), 1 + i % 3, 4) for i in range(300)]
        out.append((f"ones/{R}", R, ones + [TAIL], 0, None))
        body = [(lits(6, 4), 6, 5), TAIL]
        out.append((f"block-end@0/{R}", R, body, _size(body), 0))
        out.append((f"frame-end@0/{R}", R, body, _size(body) + 4, 0))
    # the ring lengths interleaved, so a short batch meets all three
    per = len(out) // len(RINGS)
    return [out[r * per + i] for i in range(per) for r in range(len(RINGS))]


SPECS = _specs()


def _batch(n: int):
    """n frames back to back: spec i % len(SPECS) for frame i, its prefix sized
    for where the frame lies in the batch"""
    frames, dsizes, wants, names = [], [], [], []
    c_off = [0]
    for i in range(n):
        name, R, body, anchor, target = SPECS[i % len(SPECS)]
        cx0 = c_off[i] - (c_off[64 * (i // 64)] & ~31)
        nmin = R + 40                                     # at least one lap before the anchor
        npre = nmin if target is None else nmin + (target - (cx0 + HEAD + nmin + anchor)) % R
        assert target is None or (cx0 + HEAD + npre + anchor) % R == target
        f, want = lz4_craft._build([_prefix(npre, i) + body])
        assert len(want) <= 8192 and len(f) == HEAD + npre + _size(body) + 4
        frames.append(f)
        dsizes.append(len(want))
        wants.append(want)
        names.append(name)
        c_off.append(c_off[i] + len(f))
    return frames, dsizes, wants, names


@pytest.fixture(scope="module")
def batches(oracle):
    """each batch once, every frame held to the CPU decoder"""
    made = {}
    for n in BATCHES:
        frames, dsizes, wants, names = _batch(n)
        for f, ds, want, name in zip(frames, dsizes, wants, names):
            st, got, used, _ = oracle.decode_frame(f, ds)
            assert (st, got, used) == (0, want, len(f)), name
        made[n] = (frames, dsizes, wants, names)
    assert len(SPECS) < 257 and {s[1] for s in SPECS[:64]} == set(RINGS)
    return made


@pytest.mark.parametrize("engine", ["lean", "block"])
@pytest.mark.parametrize("n", BATCHES)
def test_ring_wrap(gpu, zs, batches, n, engine):
    frames, dsizes, wants, names = batches[n]
    got, st = lz4_craft.decode(zs, gpu, frames, dsizes, engine)
    bad = [i for i, s in enumerate(st) if s != 0]
    assert not bad, [(names[i], zs.status_string(st[i])) for i in bad][:12]
    bad = [i for i in range(n) if got[i] != wants[i]]
    assert not bad, [names[i] for i in bad][:12]
