#!/usr/bin/env python3
"""Whole frames by index: in-place decode against staging plus gather, the
numbers of DESIGN.md §6 "Frames by index".

A 64 MiB LZ4 image of 64 KiB frames built in device memory by
zsk_lz4_build_image; all 1,024 frames read in one shuffled order, packed, in
two ways that alternate inside every repetition (one process, `--runs` timed
runs after `--warmup` warm-ups; medians and min-max of the GPU time between two
events on the call's stream, and of the host time of the call itself), every
run's bytes and results checked before its time counts:

  read_frames   zsk_read_frames_indirect: the index list in device memory,
                each frame decoded at its scanned offset of the destination
  indirect      zsk_preadv_device_indirect over the same frames as ranges
                (offset = frame start, count = 64 KiB, dst_off = the same
                packed offsets, max_frames = 1,024): decoded into the slot's
                staging, then gathered into the destination

    python scripts/read_frames_probe.py [--runs K] [--warmup W] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libzseek_amd.zseek as zs  # noqa: E402

FRAME = 65536
SIZE = 64 << 20


def row(values, unit):
    v = sorted(values)
    return {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "unit": unit}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("read_frames_probe needs a GPU")
    L = zs.lib()
    n = SIZE // FRAME
    d_data = torch.from_numpy(zs.synth_buffer(SIZE)).to("cuda")
    d_img = zs.lz4_build_image(d_data, FRAME)
    err = C.create_string_buffer(zs.ERRBUF)
    h = L.zsk_reader_open_device(d_img.data_ptr(), d_img.numel(), 0, err)
    if not h:
        sys.exit("open_device: " + err.value.decode())
    S = torch.cuda.Stream()
    order = np.random.default_rng(1).permutation(n).astype(np.int64)
    d_idx = torch.from_numpy(order).to("cuda")
    rg = np.zeros(n, zs.RANGE_DTYPE)
    rg["offset"], rg["count"], rg["dst_off"] = order * FRAME, FRAME, np.arange(n, dtype=np.int64) * FRAME
    d_rg = torch.from_numpy(rg.view(np.uint8).copy()).to("cuda")
    d_buf = torch.empty(SIZE, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_res = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    # the expected bytes: the payload's frames in the list's order
    want = d_data.view(n, FRAME)[d_idx].reshape(-1).contiguous()
    want_res = torch.tensor([FRAME] * n + [n], dtype=torch.int64, device="cuda")
    want_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * FRAME
    torch.cuda.synchronize()

    def read_frames():
        return L.zsk_read_frames_indirect(h, d_idx.data_ptr(), n, 0, d_buf.data_ptr(), SIZE, d_off.data_ptr(),
                                          d_res.data_ptr(), S.cuda_stream, err)

    def indirect():
        return L.zsk_preadv_device_indirect(h, d_buf.data_ptr(), SIZE, d_rg.data_ptr(), n, n, d_res.data_ptr(),
                                            S.cuda_stream, err)

    variants = {"read_frames": read_frames, "indirect": indirect}
    gpu = {k: [] for k in variants}
    host = {k: [] for k in variants}
    with torch.cuda.stream(S):
        for rep in range(args.warmup + args.runs):
            for name, fn in variants.items():
                d_buf.zero_()
                d_res.zero_()
                d_off.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                S.synchronize()
                e0.record(S)
                t0 = time.perf_counter()
                ret = fn()
                t = time.perf_counter() - t0
                e1.record(S)
                S.synchronize()
                ok = ret == 0 and torch.equal(d_buf, want) and torch.equal(d_res, want_res)
                if name == "read_frames":
                    ok = ok and torch.equal(d_off, want_off)
                if not ok:
                    raise RuntimeError(f"{name}: wrong bytes or results ({ret}) {err.value.decode()}")
                if rep >= args.warmup:
                    gpu[name].append(e0.elapsed_time(e1))
                    host[name].append(t * 1e3)
    L.zseek_reader_close(h, None, None)
    result = {"image_bytes": int(d_img.numel()), "decoded_bytes": SIZE, "frames": n, "runs": args.runs,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "gpu_ms": {k: row(v, "ms") for k, v in gpu.items()},
              "host_call_ms": {k: row(v, "ms") for k, v in host.items()}}
    for k in variants:
        result["gpu_ms"][k]["GB_per_s"] = round(SIZE / result["gpu_ms"][k]["median"] / 1e6, 1)
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
