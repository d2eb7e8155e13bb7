#!/usr/bin/env python3
"""Seekable files in device memory: the numbers of DESIGN.md §7 "Device images".

Three sections, each variant alternating with its counterpart inside every
repetition (one process, `--runs` timed runs after one warm-up; median and
min-max), every run's bytes checked before its time counts:

  read    one zsk_pread_device call over the whole file (`--size`, default
          1 GiB of the synthetic, 64 KiB frames, LZ4 and zstd): a reader opened
          with zsk_reader_open_device on the image in HBM against a reader on a
          host copy (C in-memory pread callback, io threads 1)
  small   p50 / p99 of 4 KiB zseek_pread calls at random offsets, cache 0
          (zsk_tool_latency, as scripts/latency_probe.py), the same two readers
  build   zsk_lz4_build_image (64 KiB and 1 MiB frames, checksums off / on)
          against zsk_write_device into an in-memory sink (the gpu_dev rows of
          scripts/writer_probe.py, re-run here)

    python scripts/image_probe.py [--size N] [--runs K] [--only read small build] [--out FILE.json]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import libzseek_amd.zseek as zs  # noqa: E402
import writer_probe  # noqa: E402


def row(values, unit):
    v = sorted(values)
    return {"median": round(statistics.median(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3), "unit": unit}


def open_pair(L, T, img: np.ndarray, d_img):
    """(device-image reader, host-image reader) handles on the same bytes."""
    err = C.create_string_buffer(zs.ERRBUF)
    dev = L.zsk_reader_open_device(d_img.data_ptr(), d_img.numel(), 0, err)
    if not dev:
        raise RuntimeError("open_device: " + err.value.decode())
    host = T.zsk_tool_open_mem(C.cast(L.zseek_reader_open_full, C.c_void_p), img.ctypes.data, img.size, 0, err)
    if not host:
        raise RuntimeError("open_mem: " + err.value.decode())
    return dev, host


def close_pair(L, T, dev, host):
    L.zseek_reader_close(dev, None, None)
    T.zsk_tool_close_mem(C.cast(L.zseek_reader_close, C.c_void_p), host)


def uploaded(L, h) -> int:
    s = zs.GpuStatsC()
    L.zsk_reader_gpu_stats_ex(h, C.byref(s), C.sizeof(s))
    return int(s.bytes_uploaded)


def section_read(args, data, d_data, images, torch):
    L, T = zs.lib(), zs.tools()
    out = {}
    d_out = torch.empty(data.size + 64, dtype=torch.uint8, device="cuda")
    err = C.create_string_buffer(zs.ERRBUF)
    for codec, img in images.items():
        d_img = torch.from_numpy(img).to("cuda")
        dev, host = open_pair(L, T, img, d_img)
        times = {"device_image": [], "host_image": []}
        for rep in range(args.runs + 1):
            for name, h in (("device_image", dev), ("host_image", host)):
                d_out.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = L.zsk_pread_device(h, d_out.data_ptr(), data.size, 0, None, err)
                t = time.perf_counter() - t0
                if n != data.size or not torch.equal(d_out[: data.size], d_data):
                    raise RuntimeError(f"{codec} {name}: wrong bytes ({n}) {err.value.decode()}")
                if rep:
                    times[name].append(data.size / t / 1e9)
        rows = {k: row(v, "GB/s") for k, v in times.items()}
        rows["bytes_uploaded"] = {"device_image": uploaded(L, dev), "host_image": uploaded(L, host)}
        rows["image_bytes"] = int(img.size)
        out[codec] = rows
        print(json.dumps({"read": codec, **rows}), flush=True)
        close_pair(L, T, dev, host)
        del d_img
    return out


def section_small(args, data, images, torch):
    L, T = zs.lib(), zs.tools()
    out = {}
    n = args.requests
    pread = C.cast(L.zseek_pread, C.c_void_p)
    for codec, img in images.items():
        d_img = torch.from_numpy(img).to("cuda")
        dev, host = open_pair(L, T, img, d_img)
        rng = np.random.default_rng(1)
        offs = rng.integers(0, data.size - 4096, n).astype(np.uint64)
        us = {"device_image": [], "host_image": []}
        buf = np.empty(4096, np.uint8)
        for rep in range(args.runs + 1):
            for name, h in (("device_image", dev), ("host_image", host)):
                ns = np.zeros(n, np.uint64)
                failed = C.c_size_t(0)
                if T.zsk_tool_latency(pread, h, offs.ctypes.data, n, 4096, buf.ctypes.data, ns.ctypes.data,
                                      C.byref(failed)) != 0 or failed.value:
                    raise RuntimeError(f"{codec} {name}: a request failed")
                o = int(offs[-1])
                if bytes(buf) != data[o: o + 4096].tobytes():
                    raise RuntimeError(f"{codec} {name}: wrong bytes")
                if rep:
                    us[name].append(ns[20:].astype(np.float64) / 1e3)
        rows = {}
        for name, runs in us.items():
            rows[name] = {"p50_us": row([float(np.percentile(r, 50)) for r in runs], "us"),
                          "p99_us": row([float(np.percentile(r, 99)) for r in runs], "us")}
        out[codec] = rows
        print(json.dumps({"small": codec, **rows}), flush=True)
        close_pair(L, T, dev, host)
        del d_img
    return out


def section_build(args, data, d_data, torch):
    L, T = zs.lib(), zs.tools()
    sink_fn = C.cast(T.zsk_tool_sink_write, zs.WRITE_FN)
    W = writer_probe.bind(zs.LIB_PATH)
    store = np.empty(data.size + data.size // 16 + (1 << 20), np.uint8)
    sink = writer_probe.Sink(store.ctypes.data, store.size, 0)
    back = np.empty(data.size, np.uint8)
    d_back = torch.empty(data.size + 64, dtype=torch.uint8, device="cuda")
    err = C.create_string_buffer(zs.ERRBUF)
    out = {}
    for frame in args.frames:
        d_image = torch.empty(zs.lz4_image_bound(data.size, frame, True), dtype=torch.uint8, device="cuda")
        times = {"build_image": [], "build_image_ck": [], "write_device": [], "write_device_ck": []}
        sizes = {}
        for rep in range(args.runs + 1):
            for name in times:
                ck = name.endswith("_ck")
                if name.startswith("build"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = L.zsk_lz4_build_image(d_data.data_ptr(), data.size, frame, 0, 1 if ck else 0, 0,
                                              d_image.data_ptr(), d_image.numel(), err)
                    t = time.perf_counter() - t0
                    if n < 0:
                        raise RuntimeError("build image: " + err.value.decode())
                    # read back where it is, checksums verified when it carries them
                    h = L.zsk_reader_open_device(d_image.data_ptr(), n, 0, err)
                    if not h:
                        raise RuntimeError("open built image: " + err.value.decode())
                    L.zsk_reader_set_verify_checksums(h, ck)
                    d_back.zero_()
                    got = L.zsk_pread_device(h, d_back.data_ptr(), data.size, 0, None, err)
                    L.zseek_reader_close(h, None, None)
                    if got != data.size or not torch.equal(d_back[: data.size], d_data):
                        raise RuntimeError(f"{name}: image does not decode to the input")
                    if int(d_image[n - 5]) != (0x80 if ck else 0):
                        raise RuntimeError(f"{name}: seek-table descriptor")
                    sizes[name] = int(n)
                else:
                    t = writer_probe.write_file(W, sink, sink_fn, data, d_data.data_ptr(), frame, True, ck, True)
                    image = store[: sink.used]
                    writer_probe.read_back(image, back, ck)
                    if not np.array_equal(back, data):
                        raise RuntimeError(f"{name}: file does not decode to the input")
                    back[:4096] = 0
                    sizes[name] = int(sink.used)
                if rep:
                    times[name].append(data.size / t / 1e9)
        if sizes["build_image"] != sizes["write_device"] or sizes["build_image_ck"] != sizes["write_device_ck"]:
            raise RuntimeError(f"file sizes differ: {sizes}")
        rows = {k: row(v, "GB/s") for k, v in times.items()}
        rows["file_bytes"] = sizes["build_image"]
        out[str(frame)] = rows
        print(json.dumps({"build": frame, **rows}), flush=True)
        del d_image
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--requests", type=int, default=1000, help="4 KiB reads per latency run")
    ap.add_argument("--frames", type=int, nargs="+", default=[65536, 1 << 20], help="build: frame sizes")
    ap.add_argument("--only", nargs="+", default=["read", "small", "build"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("image_probe needs a GPU")
    zs.lib()
    data = zs.synth_buffer(args.size)
    d_data = torch.from_numpy(data).to("cuda")
    torch.cuda.synchronize()
    result = {"input_bytes": args.size, "runs": args.runs, "device": torch.cuda.get_device_name(0)}
    if "read" in args.only or "small" in args.only:
        images = {"lz4": zs.lz4_seekable(data, 65536), "zstd": zs.zstd_seekable(data, 65536)}
        if "read" in args.only:
            result["read"] = section_read(args, data, d_data, images, torch)
        if "small" in args.only:
            result["small"] = section_small(args, data, images, torch)
    if "build" in args.only:
        result["build"] = section_build(args, data, d_data, torch)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
