"""tests/zstd_craft.py's entries for tests/test_gpu_zstd_craft.py's switch
test: run in a fresh process (the library reads its environment switches once,
at first use), it decodes every crafted entry through zsk_zstd_decode_frames
in batches of 64 or fewer (the one-frame route where it is on) and prints one
JSON object -- per case its status and the SHA-256 of its output slot where
the status is 0.  Test infrastructure only."""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def run():
    import torch

    import libzseek_amd.zseek as zs
    import zstd_craft as zc
    gpu = torch.device("cuda", 0)
    res = {}
    # batch sizes take turns so that full and partial batches both occur
    at, sizes, k = 0, [64, 1, 33, 64, 2, 31, 63], 0
    while at < len(zc.CASES):
        batch = zc.CASES[at: at + sizes[k % len(sizes)]]
        got, st = zc.decode(zs, gpu, [c[1] for c in batch], [c[2] for c in batch])
        for c, g, s in zip(batch, got, st):
            res[c[0]] = [s, hashlib.sha256(g).hexdigest() if s == 0 else ""]
        at += len(batch)
        k += 1
    return res


if __name__ == "__main__":
    print(json.dumps(run()))
