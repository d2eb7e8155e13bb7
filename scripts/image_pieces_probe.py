#!/usr/bin/env python3
"""The stream-ordered image builds: the numbers of DESIGN.md §7 "Images on the
caller's stream".

Input: `--size` bytes of the synthetic (default 1 GiB) in device memory, frames
of 64 KiB and 1 MiB, LZ4 and zstd; one process, `--runs` timed runs after one
warm-up, median and min-max in milliseconds.

  sync    zsk_lz4_build_image / zsk_zstd_build_image of this build alternating
          with another build of the library (`--parent`, the parent commit's
          libzseek.so): what the shared core costs the synchronous entry points
  queue   `--builds` builds queued back to back, wall time from the first call
          to the final synchronize: the synchronous call, the _pieces call with
          NULL sizes, and the _pieces call with a device list of equal sizes;
          and the host time spent inside one _pieces call (median over the
          queued calls)

Every variant's first image is compared with the synchronous builder's.

    python scripts/image_pieces_probe.py [--size N] [--runs K] [--parent LIB] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libzseek_amd.zseek as zs  # noqa: E402


def row(values):
    v = sorted(values)
    return {"median": round(statistics.median(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3), "unit": "ms"}


def bind_sync(path):
    L = C.CDLL(path)
    L.zsk_lz4_build_image.restype = C.c_ssize_t
    L.zsk_lz4_build_image.argtypes = zs.lib().zsk_lz4_build_image.argtypes
    L.zsk_zstd_build_image.restype = C.c_ssize_t
    L.zsk_zstd_build_image.argtypes = zs.lib().zsk_zstd_build_image.argtypes
    return L


def sync_build(L, codec, d_src, n, frame, d_image, err):
    if codec == "lz4":
        r = L.zsk_lz4_build_image(d_src.data_ptr(), n, frame, 0, 0, 0, d_image.data_ptr(), d_image.numel(), err)
    else:
        r = L.zsk_zstd_build_image(d_src.data_ptr(), n, frame, 0, 0, d_image.data_ptr(), d_image.numel(), err)
    if r < 0:
        raise RuntimeError("build image: " + err.value.decode())
    return int(r)


def pieces_build(L, codec, d_src, n, d_sizes, k, frame, d_image, d_res, stream, err):
    z = None if d_sizes is None else d_sizes.data_ptr()
    if codec == "lz4":
        r = L.zsk_lz4_build_image_pieces(d_src.data_ptr(), n, z, k, frame, 0, 0, 0, d_image.data_ptr(),
                                         d_image.numel(), d_res.data_ptr(), stream, err)
    else:
        r = L.zsk_zstd_build_image_pieces(d_src.data_ptr(), n, z, k, frame, 0, 0, d_image.data_ptr(),
                                          d_image.numel(), d_res.data_ptr(), stream, err)
    if r != 0:
        raise RuntimeError("build image pieces: " + err.value.decode())


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--builds", type=int, default=8)
    ap.add_argument("--frames", type=int, nargs="+", default=[65536, 1 << 20])
    ap.add_argument("--parent", default=None, help="the parent commit's libzseek.so")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("image_pieces_probe needs a GPU")
    L = zs.lib()
    P = bind_sync(args.parent) if args.parent else None
    n = args.size - args.size % max(args.frames)      # whole frames: the equal-size list is the fixed-frame build
    d_src = torch.from_numpy(zs.synth_buffer(n)).to("cuda")
    err = C.create_string_buffer(zs.ERRBUF)
    q = torch.cuda.Stream()
    result = {"input_bytes": n, "runs": args.runs, "builds": args.builds, "device": torch.cuda.get_device_name(0),
              "sync": {}, "queue": {}}
    for codec in ("lz4", "zstd"):
        bound = L.zsk_lz4_pieces_bound if codec == "lz4" else L.zsk_zstd_pieces_bound
        for frame in args.frames:
            k = n // frame
            key = "%s_%d" % (codec, frame)
            cap = bound(n, k, 0)
            d_image = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_other = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_sizes = torch.full((k,), frame, dtype=torch.int32, device="cuda")
            d_res = torch.zeros(3, dtype=torch.int64, device="cuda")
            size = sync_build(L, codec, d_src, n, frame, d_image, err)

            # -- sync: this build against the parent's, alternating -------------------------
            if P is not None:
                t = {"parent": [], "this": []}
                for rep in range(args.runs + 1):
                    for name, lib in (("parent", P), ("this", L)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        got = sync_build(lib, codec, d_src, n, frame, d_other, err)
                        dt = (time.perf_counter() - t0) * 1e3
                        if rep == 0 and (got != size or not torch.equal(d_other[:size], d_image[:size])):
                            raise RuntimeError(f"{key} {name}: the images differ")
                        if rep:
                            t[name].append(dt)
                result["sync"][key] = {name: row(v) for name, v in t.items()}
                print(json.dumps({"sync": key, **result["sync"][key]}), flush=True)

            # -- queue: builds back to back, one wait at the end ---------------------------------
            t = {"sync_calls": [], "pieces_null": [], "pieces_list": []}
            inside = {"pieces_null": [], "pieces_list": []}
            for rep in range(args.runs + 1):
                for name in t:
                    d_other.zero_()
                    torch.cuda.synchronize()
                    calls = []
                    t0 = time.perf_counter()
                    for _ in range(args.builds):
                        if name == "sync_calls":
                            sync_build(L, codec, d_src, n, frame, d_other, err)
                        else:
                            c0 = time.perf_counter()
                            pieces_build(L, codec, d_src, n, d_sizes if name == "pieces_list" else None, k, frame,
                                         d_other, d_res, q.cuda_stream, err)
                            calls.append((time.perf_counter() - c0) * 1e3)
                    q.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep == 0 and name != "sync_calls":
                        if tuple(int(x) for x in d_res.cpu()) != (size, k, n) or \
                                not torch.equal(d_other[:size], d_image[:size]):
                            raise RuntimeError(f"{key} {name}: the images differ")
                    if rep:
                        t[name].append(dt)
                        if calls:
                            inside[name].append(statistics.median(calls))
            rows = {name: row(v) for name, v in t.items()}
            rows["host_ms_in_one_call"] = {name: row(v) for name, v in inside.items()}
            rows["file_bytes"] = size
            result["queue"][key] = rows
            print(json.dumps({"queue": key, **rows}), flush=True)
            del d_image, d_other, d_sizes
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
