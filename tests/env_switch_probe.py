"""Single-frame read cases for tests/test_gpu_env_switches.py: run in a fresh
process (the library reads its environment switches once, at first use), it
prints one JSON object -- per case the SHA-256 of the bytes a caller's read
loop gets and the error text it ends with.  Five hand-built linked frames of
tests/lz4_linked_craft.py (the one-frame route's big frames, which
ZSEEK_ONE_BIG and ZSEEK_ONE_BLOCKS reroute) are among the cases; their answers
are also held to the byte model here, whatever the switch.  Test
infrastructure only."""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# a chain frame, a straddle frame, a 1025-tainted frame, a dense frame and a
# refused frame
LINKED = ["e_chain5_off65535", "a_straddle_k7_e15_gt", "d_tainted1025_v0", "f_dense_before", "g_truncated_seq"]


def cases():
    g = os.path.join(ROOT, "tests", "golden")
    out = {}
    for name in ("lz4_64k_direct", "zstd_64k_direct", "lz4_1m_direct"):
        img = np.frombuffer(open(os.path.join(g, name + ".zs"), "rb").read(), np.uint8).copy()
        out[name] = img
        bad = img.copy()
        bad[len(img) // 3] ^= 0x5A   # inside a middle frame's compressed bytes
        out[name + "_corrupt"] = bad
    return out


def linked_cases():
    """name -> (seekable image of the frame between lz4_craft's two intact
    neighbours, per frame (decoded size, bytes, whole): a refused frame's bytes
    are those of the blocks before its malformed one, whole False)"""
    import lz4_craft
    import lz4_linked_craft
    (fa, a), (fb, b) = lz4_craft.NEIGHBOURS
    out = {}
    for name in LINKED:
        _, frame, dsize, want = lz4_linked_craft.case(name)
        if want is None:
            blocks = lz4_linked_craft.BLOCKS[name]
            bad = [isinstance(blk, lz4_craft.R) for blk in blocks].index(True)
            want = lz4_craft._build(blocks[:bad], independent=False)[1]
        img = lz4_craft.seekable([fa, frame, fb], [len(a), dsize, len(b)])
        out["linked_" + name] = (np.frombuffer(img, np.uint8).copy(),
                                 [(len(a), a, True), (dsize, want, len(want) == dsize), (len(b), b, True)])
    return out


def model_read(parts, off, count, cache):
    """what a caller's read loop may get from `off` on, a frame a call: the
    frames' bytes up to `count` or the end of the file -> the acceptable
    (bytes, ends in an error) outcomes.  A refused frame ends the loop in an
    error.  Without a cache the frame is decoded only as far as the read
    goes, so a read that ends before the malformed block may also deliver
    (the reference does when the read starts at the frame's start; from
    inside the frame it fails while skipping): there both outcomes count,
    each with the right bytes."""
    got, at, fail_too = b"", 0, []
    for size, data, whole in parts:
        lo = max(off, at) - at
        if lo < size and len(got) < count:
            n = min(count - len(got), size - lo)
            if not whole:
                if cache != 0 or lo + n > len(data):
                    return [(got, True)]
                fail_too = [(got, True)]
            got += data[lo: lo + n]
        at += size
    return [(got, False)] + fail_too


def run():
    import libzseek_amd.zseek as zs
    res = {}
    linked = linked_cases()
    todo = dict(cases())
    todo.update({name: img for name, (img, _) in linked.items()})
    for name, img in todo.items():
        for cache in (0, 1):
            with zs.Reader(img, cache) as r:
                total = int(r.frames()[1][-1])
                rng = np.random.default_rng(7)
                offs = [0, total // 3, total // 2 + 123, max(total - 4096, 0)] + \
                    [int(x) for x in rng.integers(0, max(total - 4096, 1), 12)]
                # (the linked frames also whole: every block, every tainted byte)
                for off, count in [(off, 4096) for off in offs] + ([(0, total)] if name in linked else []):
                    got, err = b"", None
                    while len(got) < count:
                        try:
                            b = r.pread(count - len(got), off + len(got))
                        except zs.ZseekError as e:
                            err = str(e)
                            break
                        if not b:
                            break
                        got += b
                    key = f"{name}/c{cache}/{off}" if count == 4096 else f"{name}/c{cache}/whole"
                    res[key] = [hashlib.sha256(got).hexdigest(), len(got), err]
                    if name in linked:
                        assert (got, err is not None) in model_read(linked[name][1], off, count, cache), \
                            (name, cache, off, count, len(got), err)
    return res


if __name__ == "__main__":
    print(json.dumps(run()))
