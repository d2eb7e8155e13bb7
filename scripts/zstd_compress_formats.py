#!/usr/bin/env python3
"""The three formats of the GPU zstd compressor side by side:

  sizes   synth(4 MiB, seed 1), plain and with every byte's top bit flipped, at
          64 KiB and 4 KiB frames: subset, full, wide, libzstd level 1 and -1,
          liblz4; synth(8 MiB, seed 1) at 64 KiB and 1 MiB frames: full, wide
  times   1 GiB of synth_buffer at 4 KiB, 64 KiB and 1 MiB frames: HIP events
          around one call, one warm-up, median of 5, the three formats
          alternated
  --parent LIB   the subset and the full call of this build against another
          build's libzseek.so (the commit before), alternated, four runs each

    python scripts/zstd_compress_formats.py [--gib 1] [--parent path/to/libzseek.so] [--out result.json]

Prints a table and, with --out, writes the numbers as JSON.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-sizes", action="store_true")
    args = ap.parse_args()

    import torch

    import libzseek_amd.zseek as zs
    import zstd_util
    from oracle.oracle import Oracle

    dev = torch.device("cuda", 0)
    L = zs.lib()
    result = {"device": torch.cuda.get_device_name(0), "sizes": {}, "times": {}, "parent": {}}

    FORMATS = (("subset", 0), ("full", 1), ("wide", zs.ZSTD_FORMAT_FULL_WIDE))

    def call(lib, fmt, d_desc, n, d_src, d_dst, d_cs, scratch):
        a = (d_desc.data_ptr(), n, d_src.data_ptr(), d_dst.data_ptr(), d_cs.data_ptr(), scratch.data_ptr(),
             scratch.numel(), torch.cuda.current_stream().cuda_stream)
        r = lib.zsk_zstd_compress_frames(*a) if fmt is None else lib.zsk_zstd_compress_frames_ex(*a, fmt)
        assert r == 0

    def setup(data: np.ndarray, fs: int):
        nf = data.size // fs
        desc, total = zs.zstd_compress_layout([fs] * nf)
        return (torch.from_numpy(desc.view(np.uint8).copy()).to(dev), nf, torch.from_numpy(data).to(dev),
                torch.empty(total, dtype=torch.uint8, device=dev), torch.zeros(nf, dtype=torch.int32, device=dev),
                torch.empty(zs.zstd_compress_scratch_size(nf, data.size, wide=True), dtype=torch.uint8, device=dev))

    def timed(lib, fmt, st) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(lib, fmt, *st)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    # ---- sizes
    if not args.skip_sizes:
        z = zstd_util.load()
        plain = Oracle().synth(4 << 20, 1)
        for name, data in (("plain", plain), ("xor80", plain ^ np.uint8(0x80))):
            for fs in (65536, 4096):
                st = setup(data, fs)
                row = {}
                for label, fmt in FORMATS:
                    call(L, fmt, *st)
                    torch.cuda.synchronize()
                    row[label] = int(st[4].sum().item())
                c_off, _ = zs.seek_table_of(zs.lz4_seekable(data, fs))
                row["liblz4"] = int(c_off[-1])
                if z is not None:
                    for lv in (1, -1):
                        row["libzstd_%d" % lv] = sum(
                            len(zstd_util.compress(z, data[i * fs:(i + 1) * fs].tobytes(), {zstd_util.P_LEVEL: lv}))
                            for i in range(data.size // fs))
                result["sizes"]["%s_%d" % (name, fs)] = row
                print("sizes %-6s frame %6d: " % (name, fs) +
                      "  ".join("%s %d (%.4f)" % (k, v, v / data.size) for k, v in row.items()), flush=True)

        data = Oracle().synth(8 << 20, 1)
        for fs in (65536, 1 << 20):
            st = setup(data, fs)
            row = {}
            for label, fmt in FORMATS[1:]:
                call(L, fmt, *st)
                torch.cuda.synchronize()
                row[label] = int(st[4].sum().item())
            result["sizes"]["synth8_%d" % fs] = row
            print("sizes synth(8 MiB, 1) frame %7d: full %d  wide %d (%.4f of full)" %
                  (fs, row["full"], row["wide"], row["wide"] / row["full"]), flush=True)

    # ---- times
    n = int(args.gib * (1 << 30)) & ~((1 << 20) - 1)
    big = zs.synth_buffer(n)
    for fs in (4096, 65536, 1 << 20):
        st = setup(big, fs)
        runs = {label: [] for label, _ in FORMATS}
        for label, fmt in FORMATS:
            timed(L, fmt, st)                                   # warm-up
        size = {}
        for _ in range(5):
            for label, fmt in FORMATS:
                runs[label].append(timed(L, fmt, st))
                size[label] = int(st[4].to(torch.int64).sum().item())
        row = {k: {"ms": v, "median_ms": statistics.median(v), "bytes": size[k]} for k, v in runs.items()}
        result["times"][str(fs)] = row
        for k, v in row.items():
            print("times frame %7d %-6s median %.1f ms (%.1f GB/s)  runs %s  %d bytes" %
                  (fs, k, v["median_ms"], n / v["median_ms"] / 1e6, ["%.1f" % x for x in v["ms"]], v["bytes"]), flush=True)
        if args.parent:
            P = C.CDLL(args.parent)
            P.zsk_zstd_compress_frames.restype = C.c_int
            P.zsk_zstd_compress_frames.argtypes = L.zsk_zstd_compress_frames.argtypes
            P.zsk_zstd_compress_frames_ex.restype = C.c_int
            P.zsk_zstd_compress_frames_ex.argtypes = L.zsk_zstd_compress_frames_ex.argtypes
            result["parent"][str(fs)] = {}
            for label, fmt in (("subset", None), ("full", 1)):
                timed(P, fmt, st)
                timed(L, fmt, st)
                pr = {"parent": [], "this": []}
                for _ in range(4):
                    pr["parent"].append(timed(P, fmt, st))
                    pr["this"].append(timed(L, fmt, st))
                result["parent"][str(fs)][label] = pr
                print("%s call, frame %7d: parent %s  this build %s" %
                      (label, fs, ["%.2f" % x for x in pr["parent"]], ["%.2f" % x for x in pr["this"]]), flush=True)
        del st
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
