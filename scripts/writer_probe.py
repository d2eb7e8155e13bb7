#!/usr/bin/env python3
"""Writer throughput probe: seek-table checksums and writes from device memory.

Writes `--size` bytes (default 1 GiB) of the synthetic as an LZ4 seekable file
of `--frames` byte frames (default 64 KiB and 1 MiB) into an in-memory sink (a
C callback, libzseek_tools' zsk_tool_sink_write) and reports, per frame size,
the median and the spread (min, max) over `--runs` timed runs after one
warm-up of:

  gpu_host      GPU-mode writer fed from host memory (zseek_write per frame)
  gpu_host_ck   the same with zsk_writer_set_checksums on
  gpu_dev       zsk_write_device from device memory (one call)
  gpu_dev_ck    the same with checksums on
  host          host mode (liblz4 on one core)
  host_ck       host mode with checksums on: host - host_ck is one core's XXH64
  parent        gpu_host through another build of the library (--parent-lib,
                the parent commit's libzseek.so), alternating with this one's:
                checksums off must change nothing on the existing path

A run is open + writes + close on a host clock (close flushes and
synchronizes).  The variants alternate inside each repetition, so drift of a
shared machine hits all of them alike.  Every file written is read back whole
through the reader (verifying the checksums it carries) and compared with the
input before its time counts.  One process, the calling thread only.

    python scripts/writer_probe.py [--parent-lib PATH] [--out FILE.json]
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


class Sink(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("cap", C.c_size_t), ("used", C.c_size_t)]


def bind(path: str) -> C.CDLL:
    """The writer calls of a libzseek build (this one's or the parent's)."""
    L = C.CDLL(path)
    L.zseek_writer_open_full.restype = C.c_void_p
    L.zseek_writer_open_full.argtypes = [zs.WriteFile, C.POINTER(zs.CompressionParam), C.c_size_t, C.c_void_p,
                                         C.c_char_p]
    L.zseek_write.restype = C.c_bool
    L.zseek_write.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
    L.zseek_writer_close.restype = C.c_bool
    L.zseek_writer_close.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
    L.zsk_writer_set_gpu_compress.restype = C.c_bool
    L.zsk_writer_set_gpu_compress.argtypes = [C.c_void_p, C.c_size_t]
    if hasattr(L, "zsk_writer_set_checksums"):
        L.zsk_writer_set_checksums.restype = C.c_bool
        L.zsk_writer_set_checksums.argtypes = [C.c_void_p, C.c_bool]
        L.zsk_write_device.restype = C.c_bool
        L.zsk_write_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_char_p]
    return L


def write_file(L, sink, sink_fn, data, d_ptr, frame, gpu, checksums, device) -> float:
    """One file into the sink; seconds from open to close."""
    err = C.create_string_buffer(zs.ERRBUF)
    p = zs.CompressionParam()
    p.type = zs.ZSEEK_LZ4
    p.params.lz4_params.compression_level = 0
    sink.used = 0
    base, size = data.ctypes.data, data.size
    t0 = time.perf_counter()
    h = L.zseek_writer_open_full(zs.WriteFile(C.addressof(sink), sink_fn), C.byref(p), frame, None, err)
    if not h:
        raise RuntimeError(err.value.decode())
    ok = (not checksums or L.zsk_writer_set_checksums(h, True)) and (not gpu or L.zsk_writer_set_gpu_compress(h, 0))
    if ok and device:
        ok = L.zsk_write_device(h, d_ptr, size, frame, None, err)
    elif ok:
        write = L.zseek_write
        for o in range(0, size, frame):
            if not write(h, base + o, min(frame, size - o), None, err):
                ok = False
                break
    ok = L.zseek_writer_close(h, None, err) and ok
    t = time.perf_counter() - t0
    if not ok:
        raise RuntimeError("write failed: " + err.value.decode())
    return t


def read_back(image: np.ndarray, out: np.ndarray, verify: bool) -> None:
    with zs.Reader(image, 0) as r:
        if verify:
            r.set_verify_checksums(True)
        done = 0
        while done < out.size:
            n = r.pread_raw(out.ctypes.data + done, out.size - done, done)
            if n <= 0:
                raise RuntimeError("read back failed: " + r.error)
            done += n


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--frames", type=int, nargs="+", default=[65536, 1 << 20])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libzseek.so (variant `parent`)")
    ap.add_argument("--variants", nargs="+", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("writer_probe needs a GPU")
    zs.lib()
    T = zs.tools()
    sink_fn = C.cast(T.zsk_tool_sink_write, zs.WRITE_FN)
    new = bind(zs.LIB_PATH)
    parent = bind(args.parent_lib) if args.parent_lib else None

    data = zs.synth_buffer(args.size)
    d_data = torch.from_numpy(data).to("cuda")
    torch.cuda.synchronize()
    store = np.empty(args.size + args.size // 16 + (1 << 20), np.uint8)
    sink = Sink(store.ctypes.data, store.size, 0)
    back = np.empty(args.size, np.uint8)

    # name -> (library, gpu mode, checksums, from device memory)
    variants = {"gpu_host": (new, True, False, False), "gpu_host_ck": (new, True, True, False),
                "gpu_dev": (new, True, False, True), "gpu_dev_ck": (new, True, True, True),
                "host": (new, False, False, False), "host_ck": (new, False, True, False)}
    if parent is not None:
        variants = {"gpu_host": variants.pop("gpu_host"), "parent": (parent, True, False, False), **variants}
    if args.variants:
        variants = {k: v for k, v in variants.items() if k in args.variants}

    result = {"input_bytes": args.size, "runs": args.runs, "device": torch.cuda.get_device_name(0), "frames": {}}
    for frame in args.frames:
        times = {k: [] for k in variants}
        file_bytes = {}
        for rep in range(args.runs + 1):                # rep 0: the warm-up
            for name, (L, gpu, ck, dev) in variants.items():
                t = write_file(L, sink, sink_fn, data, d_data.data_ptr(), frame, gpu, ck, dev)
                image = store[: sink.used]
                if image[-5] != (0x80 if ck else 0):
                    raise RuntimeError(f"{name}: seek-table descriptor {image[-5]:#x}")
                read_back(image, back, ck)
                if not np.array_equal(back, data):
                    raise RuntimeError(f"{name}: file does not decode to the input")
                back[:4096] = 0
                file_bytes[name] = int(sink.used)
                if rep:
                    times[name].append(t)
        rows = {}
        for name, ts in times.items():
            gbs = sorted(args.size / t / 1e9 for t in ts)
            rows[name] = {"median_GBps": round(statistics.median(gbs), 3), "min_GBps": round(gbs[0], 3),
                          "max_GBps": round(gbs[-1], 3), "median_s": round(statistics.median(ts), 4),
                          "file_bytes": file_bytes[name]}
        result["frames"][str(frame)] = rows
        print(json.dumps({"frame": frame, **rows}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
