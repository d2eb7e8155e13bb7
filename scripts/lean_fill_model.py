"""CPU model of the lean parse's ring fill (lz4_lean.hip, the pair kernel) on
config 2's LZ4 stream: how many parser sub-steps a 64 KiB frame takes, and how
many of them find their bytes not yet in the ring, for a ring of R bytes
filled in slots of S bytes.

One lane.  Parser and mover sub-steps run in lock step: sub-step t of each
sees what the other published at the end of its sub-step t - 1 (the mailbox).
The parser takes up to two sequences per sub-step, each only when every byte
up to its offset word and one more is in the ring (fast()'s s_av); a sequence
whose token is in but whose offset is not takes its literal half and moves to
the offset (a sub-step that emits nothing: it counts as waiting, as the
kernel's counter does).  The mover runs the kernel's cadence, D = 2 slots and
one retired and re-issued every other sub-step, with fill_issue's rules: a
jump to need_x & ~31 when need_x has passed the fill, 32-byte pieces while
fill + 32 <= need_x + R - 16 and the frame has bytes, at most S / 32 pieces a
slot; a slot is retired only if it holds the stream's next bytes.  A load
issued in one of the mover's fill sub-steps has landed when its slot comes up
again, four sub-steps later.

What the model leaves out, and what it is therefore good for:

  * TIME.  A sub-step here is a unit; on the GPU a mover sub-step that loads
    and stores more bytes takes longer, and parser and mover share one SIMD's
    issue slots.  The model therefore mispredicts the cadence variants (it
    likes a slot retired every sub-step, which measured slower) -- use it for
    the ring length and the slot width only, never for the cadence.
  * It over-counts waits for today's kernel: measured on an MI355X the pair
    kernel's parser runs ~900-1,000 live sub-steps per frame and waits for
    bytes in ~110-190 of them (kbench variant 0x204).
  * The exact step (block header, a block's last sequence, extension chains
    past one byte) is one sub-step per use.
  * MEASURED AFTER THE MODEL WAS WRITTEN: the ring length that the model
    rewards does nothing on the GPU (R = 256 / 288 / 320 time alike at either
    slot width); the slot width does.  The model's waits
    are lock-step artefacts of reach; the GPU's parser mostly waits a memory
    round trip after a restart, which a longer ring does not shorten.

Needs only the tools library (libzseek_tools.so: the synthetic buffer and
liblz4's frames).

    python scripts/lean_fill_model.py [frames]
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libzseek_amd as z  # noqa: E402

FRAME = 64 << 10
GRID = [(256, 64), (256, 96), (256, 128), (288, 64), (288, 96), (320, 64), (320, 96), (384, 64), (384, 96),
        (512, 128)]


def frames_of(img):
    """(start, end) of each LZ4F frame of a seekable image, by walking block headers"""
    b = img.tobytes()
    out, p = [], 0
    while b[p:p + 4] == b"\x04\x22\x4d\x18":
        s = p
        p += 7 + (8 if b[p + 4] & 8 else 0)
        while True:
            bs = int.from_bytes(b[p:p + 4], "little")
            p += 4
            if bs == 0:
                break
            p += bs & 0x7FFFFFFF
        out.append((s, p))
    return out


def steps_of(b):
    """the parser's work on frame bytes b as (position of the token, position
    of the offset word or None, position after the sequence): None marks a
    step the exact step takes whole (headers, a block's last sequence)"""
    p = 7 + (8 if b[4] & 8 else 0)
    out = []
    while True:
        bs = int.from_bytes(b[p:p + 4], "little")
        out.append((p, None, p + 4))
        p += 4
        if bs == 0:
            return out
        if bs & 0x80000000:
            p += bs & 0x7FFFFFFF
            continue
        e = p + bs
        while p < e:
            tok, t = p, b[p]
            p += 1
            n = t >> 4
            if n == 15:
                while True:
                    x = b[p]
                    p += 1
                    n += x
                    if x != 255:
                        break
            p += n
            if p >= e:
                out.append((tok, None, e))
                break
            q = p
            p += 2
            if t & 15 == 15:
                while b[p] == 255:
                    p += 1
                p += 1
            out.append((tok, q, p))


def run(b, cx0, R, S):
    """(live parser sub-steps, of which waiting for bytes) of one frame"""
    seqs = steps_of(b)
    clen, pieces = len(b), S // 32
    fill = (cx0 & ~31) + 128          # head_fill: 128 bytes, synchronously
    avail_pub = avail = fill
    slots = [None, None]              # (x, pieces) in flight
    i, ip, at_off = 0, seqs[0][0], False
    need_pub = cx0 + ip
    live = waits = t = 0
    while i < len(seqs):
        # ---- mover sub-step t (sees need_pub) ----
        # (it publishes avail after the retire and before the jump: a jump's
        # restart position goes out one sub-step later, as in mover_sub)
        need_x = need_pub
        k = (t // 2) % 2
        if t % 2 == 0 and slots[k] and slots[k][0] == avail:
            avail += 32 * slots[k][1]
        pub = avail
        if t % 2 == 0:
            if need_x >= fill:
                fill = need_x & ~31
                avail = fill
            n = 0
            while n < pieces and fill + 32 * n < cx0 + clen and fill + 32 * (n + 1) <= need_x + R - 16:
                n += 1
            slots[k] = (fill, n) if n else None
            fill += 32 * n
        # ---- parser sub-step t (sees avail_pub) ----
        live += 1
        took = 0
        for _ in range(2):
            if i >= len(seqs):
                break
            tok, q, nxt = seqs[i]
            if q is None:             # the exact step: its bytes, or the sub-step waits
                if took or cx0 + min(tok + 4, clen) > avail_pub:
                    break
                i, took = i + 1, took + 1
                ip, at_off = (seqs[i][0] if i < len(seqs) else clen), False
                break
            if cx0 + q + 3 <= avail_pub:
                i, took = i + 1, took + 1
                ip, at_off = seqs[i][0], False
            else:
                if not took and not at_off and cx0 + tok + 2 <= avail_pub:
                    ip, at_off = q, True      # the literal half
                break
        if not took:
            waits += 1
        # ---- both publish ----
        avail_pub, need_pub = pub, cx0 + ip
        t += 1
        if t > 8 * clen:
            raise RuntimeError("the model does not advance")
    return live, waits


def main():
    nframes = int(sys.argv[1]) if len(sys.argv) > 1 else 39
    data = z.synth_buffer((nframes + 1) * FRAME)
    img = z.lz4_seekable(data, FRAME)
    fr = frames_of(img)[1: nframes + 1]   # frame 0 is the buffer's random head: a stored block
    print(f"{len(fr)} frames of config 2, {sum(e - s for s, e in fr) / len(fr) / 1e3:.1f} KB compressed each")
    print("| ring / slot | parser sub-steps per frame | of which waiting |")
    print("|---|---|---|")
    for R, S in GRID:
        tot = [0, 0]
        for s, e in fr:
            live, waits = run(img[s:e].tobytes(), s & 31, R, S)
            tot[0] += live
            tot[1] += waits
        print(f"| {R} / {S} | {tot[0] / len(fr):,.0f} | {tot[1] / len(fr):,.0f} |")


if __name__ == "__main__":
    main()
