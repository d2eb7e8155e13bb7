#!/usr/bin/env python3
"""Appending to a seekable image in device memory: the numbers of DESIGN.md §7
"Appending to an image".

One process, the variants of a section alternating, `--runs` timed runs after
one warm-up, HIP events on the stream, median and min-max in milliseconds.

  append  `--new` pieces of 64 KiB appended to an image of `--old` such frames,
          against rebuilding all of them in one zsk_*_build_image_pieces call
          and against building the new ones alone; LZ4 and zstd.  The appended
          image is compared with the rebuilt one.
  stash   an append of no pieces to a hand-made file of 2^16 and 2^20 frames
          (8- and 12-byte entries, the image 0 and 1 bytes off alignment): the
          stash, the check and the table rewritten.  Against hipMemcpyAsync
          device-to-device of the entries' byte count.  (The stash kernel's own
          time is the kernel trace's, a run of its own.)
  core    zsk_*_build_image_pieces and zsk_*_build_image of this build
          alternating with another build of the library (`--parent`, the
          parent commit's libzseek.so) on `--size` bytes, 64 KiB and 1 MiB
          frames: what the shared core costs the existing entry points.
          `--this-first` swaps the order within a round.

    python scripts/image_append_probe.py [--sections append stash core] [--parent LIB] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libzseek_amd.zseek as zs  # noqa: E402

PIECE = 65536


def row(values):
    v = sorted(values)
    return {"median": round(statistics.median(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3), "unit": "ms",
            "runs": [round(x, 3) for x in values]}


def bind(path):
    L = C.CDLL(path)
    for name in ("zsk_lz4_build_image", "zsk_zstd_build_image", "zsk_lz4_build_image_pieces",
                 "zsk_zstd_build_image_pieces"):
        getattr(L, name).restype = getattr(zs.lib(), name).restype
        getattr(L, name).argtypes = getattr(zs.lib(), name).argtypes
    return L


def check(rc, err):
    if rc != 0:
        raise RuntimeError(err.value.decode())


def pieces_build(L, codec, src_ptr, n, sizes_ptr, k, piece, image, d_res, stream, err):
    if codec == "lz4":
        check(L.zsk_lz4_build_image_pieces(src_ptr, n, sizes_ptr, k, piece, 0, 0, 0, image.data_ptr(), image.numel(),
                                           d_res.data_ptr(), stream, err), err)
    else:
        check(L.zsk_zstd_build_image_pieces(src_ptr, n, sizes_ptr, k, piece, 0, 0, image.data_ptr(), image.numel(),
                                            d_res.data_ptr(), stream, err), err)


def append(L, codec, src_ptr, n, sizes_ptr, k, piece, image, d_prev, prev_frames, d_res, stream, err, flags=0):
    if codec == "lz4":
        check(L.zsk_lz4_append_image_pieces(src_ptr, n, sizes_ptr, k, piece, 0, flags, 0, image.data_ptr(),
                                            image.numel(), d_prev.data_ptr(), prev_frames, d_res.data_ptr(), stream,
                                            err), err)
    else:
        check(L.zsk_zstd_append_image_pieces(src_ptr, n, sizes_ptr, k, piece, flags, 0, image.data_ptr(),
                                             image.numel(), d_prev.data_ptr(), prev_frames, d_res.data_ptr(), stream,
                                             err), err)


def timed(torch, q, fn):
    """fn queued on q between two events.  -> ms"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(q):
        a.record(q)
        fn()
        b.record(q)
    q.synchronize()
    return a.elapsed_time(b)


def section_append(torch, args, result):
    L = zs.lib()
    err = C.create_string_buffer(zs.ERRBUF)
    q = torch.cuda.Stream()
    old, new = args.old, args.new
    total = old + new
    d_src = torch.from_numpy(zs.synth_buffer(total * PIECE)).to("cuda")
    d_sizes = torch.full((total,), PIECE, dtype=torch.int32, device="cuda")
    for codec in ("lz4", "zstd"):
        pieces = L.zsk_lz4_pieces_bound if codec == "lz4" else L.zsk_zstd_pieces_bound
        bound = L.zsk_lz4_append_bound if codec == "lz4" else L.zsk_zstd_append_bound
        cap = bound(pieces(old * PIECE, old, 0), old, new * PIECE, new, 0)
        d_all = torch.empty(pieces(total * PIECE, total, 0), dtype=torch.uint8, device="cuda")
        d_new = torch.empty(pieces(new * PIECE, new, 0), dtype=torch.uint8, device="cuda")
        d_img = torch.empty(cap, dtype=torch.uint8, device="cuda")
        r_all, r_new, r_old, r_app = (torch.zeros(3, dtype=torch.int64, device="cuda") for _ in range(4))
        s, z = d_src.data_ptr(), d_sizes.data_ptr()
        pieces_build(L, codec, s, old * PIECE, z, old, PIECE, d_img, r_old, q.cuda_stream, err)
        q.synchronize()
        old_size = int(r_old[0])
        table = 17 + 8 * old
        tail = d_img[old_size - table: old_size].clone()

        def put_back():
            d_img[old_size - table: old_size] = tail

        variants = {
            "rebuild_all": lambda: pieces_build(L, codec, s, total * PIECE, z, total, PIECE, d_all, r_all,
                                                q.cuda_stream, err),
            "build_new_alone": lambda: pieces_build(L, codec, s + old * PIECE, new * PIECE, z + 4 * old, new, PIECE,
                                                    d_new, r_new, q.cuda_stream, err),
            "append_new": lambda: append(L, codec, s + old * PIECE, new * PIECE, z + 4 * old, new, PIECE, d_img,
                                         r_old, old, r_app, q.cuda_stream, err),
        }
        t = {name: [] for name in variants}
        for rep in range(args.runs + 1):
            for name, fn in variants.items():
                if name == "append_new":
                    put_back()
                dt = timed(torch, q, fn)
                if rep:
                    t[name].append(dt)
            if rep == 0:
                size = int(r_all[0])
                if tuple(int(x) for x in r_app.cpu()) != (size, total, new * PIECE) or \
                        not torch.equal(d_img[:size], d_all[:size]):
                    raise RuntimeError(codec + ": the appended image differs from the rebuilt one")
        rows = {name: row(v) for name, v in t.items()}
        rows.update(old_frames=old, new_pieces=new, old_file_bytes=old_size, new_file_bytes=int(r_all[0]))
        result["append"][codec] = rows
        print(json.dumps({"append": codec, **rows}), flush=True)
        del d_all, d_new, d_img


def hand_made(frames, ck):
    """A well-formed LZ4-looking file of `frames` frames of 4 bytes (only the
    table matters to the stash): host bytes."""
    ent = np.zeros((frames, 3 if ck else 2), "<u4")
    ent[:, 0] = 4
    ent[:, 1] = 100
    body = np.zeros(4 * frames, np.uint8)
    body[:4] = np.frombuffer(struct.pack("<I", 0x184D2204), np.uint8)
    raw = ent.tobytes()
    return body.tobytes() + struct.pack("<II", 0x184D2A5E, len(raw) + 9) + raw + \
        struct.pack("<IBI", frames, 0x80 if ck else 0, 0x8F92EAB1)


def section_stash(torch, args, result):
    L = zs.lib()
    err = C.create_string_buffer(zs.ERRBUF)
    q = torch.cuda.Stream()
    d_sizes = torch.zeros(4, dtype=torch.int32, device="cuda")
    for frames in (1 << 16, 1 << 20):
        for ck in (False, True):
            data = hand_made(frames, ck)
            entry_bytes = (12 if ck else 8) * frames
            for at in (0, 1):
                key = "frames_%d_entry_%d_offset_%d" % (frames, 12 if ck else 8, at)
                buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
                image = buf[at: at + len(data) + 32]
                image[: len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to("cuda")
                d_prev = torch.tensor([len(data), frames], dtype=torch.int64, device="cuda")
                d_res = torch.zeros(3, dtype=torch.int64, device="cuda")
                a = torch.empty(entry_bytes, dtype=torch.uint8, device="cuda")
                b = torch.empty(entry_bytes, dtype=torch.uint8, device="cuda")
                variants = {
                    "append_of_nothing": lambda: append(L, "lz4", None, 0, d_sizes.data_ptr(), 0, PIECE, image, d_prev,
                                                        frames, d_res, q.cuda_stream, err, flags=1 if ck else 0),
                    "memcpy_d2d": lambda: b.copy_(a, non_blocking=True),
                }
                t = {name: [] for name in variants}
                for rep in range(args.runs + 1):
                    for name, fn in variants.items():
                        dt = timed(torch, q, fn)
                        if rep:
                            t[name].append(dt)
                    if rep == 0:
                        if tuple(int(x) for x in d_res.cpu()) != (len(data), frames, 0) or \
                                bytes(image[: len(data)].cpu().numpy()) != data:
                            raise RuntimeError(key + ": the file changed")
                rows = {name: row(v) for name, v in t.items()}
                rows["entry_bytes"] = entry_bytes
                result["stash"][key] = rows
                print(json.dumps({"stash": key, **rows}), flush=True)


def section_core(torch, args, result):
    L = zs.lib()
    P = bind(args.parent)
    err = C.create_string_buffer(zs.ERRBUF)
    q = torch.cuda.Stream()
    n = args.size - args.size % (1 << 20)
    d_src = torch.from_numpy(zs.synth_buffer(n)).to("cuda")
    d_res = torch.zeros(3, dtype=torch.int64, device="cuda")
    for codec in args.codecs:
        for frame in args.frames:
            k = n // frame
            key = "%s_%d" % (codec, frame)
            cap = (L.zsk_lz4_pieces_bound if codec == "lz4" else L.zsk_zstd_pieces_bound)(n, k, 0)
            d_image = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_first = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_sizes = torch.full((k,), frame, dtype=torch.int32, device="cuda")

            def sync_build(lib):
                if codec == "lz4":
                    r = lib.zsk_lz4_build_image(d_src.data_ptr(), n, frame, 0, 0, 0, d_image.data_ptr(), cap, err)
                else:
                    r = lib.zsk_zstd_build_image(d_src.data_ptr(), n, frame, 0, 0, d_image.data_ptr(), cap, err)
                if r < 0:
                    raise RuntimeError(err.value.decode())
                return int(r)

            size = sync_build(L)
            d_first.copy_(d_image)
            order = ("pieces_this", "pieces_parent", "sync_this", "sync_parent") if args.this_first else \
                ("pieces_parent", "pieces_this", "sync_parent", "sync_this")
            t = {name: [] for name in order}
            for rep in range(args.runs + 1):
                for name in t:
                    lib = P if name.endswith("parent") else L
                    if name.startswith("pieces"):
                        dt = timed(torch, q, lambda: pieces_build(lib, codec, d_src.data_ptr(), n, d_sizes.data_ptr(),
                                                                  k, frame, d_image, d_res, q.cuda_stream, err))
                        got = int(d_res[0]) if rep == 0 else size
                    else:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        got = sync_build(lib)
                        dt = (time.perf_counter() - t0) * 1e3
                    if rep == 0 and (got != size or not torch.equal(d_image[:size], d_first[:size])):
                        raise RuntimeError(f"{key} {name}: the images differ")
                    if rep:
                        t[name].append(dt)
            rows = {name: row(v) for name, v in t.items()}
            for kind in ("pieces", "sync"):
                a, b = rows[kind + "_parent"], rows[kind + "_this"]
                rows[kind + "_within_parent_range"] = a["min"] <= b["median"] <= a["max"]
                rows[kind + "_ranges_overlap"] = a["min"] <= b["max"] and b["min"] <= a["max"]
            rows["order"] = list(order)
            result["core"][key] = rows
            print(json.dumps({"core": key, **rows}), flush=True)
            del d_image, d_first, d_sizes


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", nargs="+", default=["append", "stash"], choices=["append", "stash", "core"])
    ap.add_argument("--old", type=int, default=12288, help="frames of the existing image")
    ap.add_argument("--new", type=int, default=4096, help="pieces appended")
    ap.add_argument("--size", type=int, default=1 << 30, help="core: input bytes")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent", default=None, help="core: the parent commit's libzseek.so")
    ap.add_argument("--codecs", nargs="+", default=["lz4", "zstd"], choices=["lz4", "zstd"], help="core")
    ap.add_argument("--frames", type=int, nargs="+", default=[65536, 1 << 20], help="core: frame sizes")
    ap.add_argument("--this-first", action="store_true", help="core: this build before the parent's in each round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if "core" in args.sections and not args.parent:
        sys.exit("the core section needs --parent")

    import torch
    if not torch.cuda.is_available():
        sys.exit("image_append_probe needs a GPU")
    result = {"runs": args.runs, "device": torch.cuda.get_device_name(0), "append": {}, "stash": {}, "core": {}}
    for name in args.sections:
        {"append": section_append, "stash": section_stash, "core": section_core}[name](torch, args, result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
