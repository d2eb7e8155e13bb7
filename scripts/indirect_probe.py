#!/usr/bin/env python3
"""Device-planned vectored reads: the numbers of DESIGN.md §7 "Device-planned reads".

A device image of `--size` bytes of the synthetic (default 1 GiB, 64 KiB
frames, LZ4), `--ranges` random ranges of `--count` bytes per call (default
4,096 of 4 KiB) whose list is in device memory, destinations back to back.
Three variants alternate inside every repetition (one process, `--runs` timed
runs after one warm-up; median and min-max of the host time from the first
step to the end of a stream synchronize), every run's bytes and results
checked before its time counts:

  today           what a caller has to do without the call: copy the list to
                  the host, synchronize, zsk_preadv_device_async, synchronize
  indirect        zsk_preadv_device_indirect with the bound a caller has
                  without looking at the list (two frames per range),
                  synchronize
  indirect_tight  the same with max_frames = the frames the list really
                  touches (rounded up to 256): what the padding costs

Then, from HIP events on the stream and zsk_kernel_timing (a run of its own):
the GPU time of one indirect call, its decode stages, and the GPU time of a
call with max_frames 1 -- it overflows, so it runs the planning, result and
fix kernels and decodes nothing: the planning kernels' share.

`--codec zstd`: the same shape on a zstd image built in device memory by
zsk_zstd_build_image.  The device-planned read needs the reader's census
(zsk_reader_zstd_census: the host time of that call is reported -- it waits for
its kernel -- taken after a small read has created the reader's lane); `today` is the host-planned zsk_preadv_device_async after
zsk_reader_set_zstd_async(3).  Also reported: the reader's device memory after
each variant's first call (each on a reader of its own), and the bounds the
two size their zstd scratch by -- the census' against the policy's.

    python scripts/indirect_probe.py [--codec lz4|zstd] [--size N] [--ranges N] [--count N] [--runs K] [--out FILE.json]
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


def row(values, unit):
    v = sorted(values)
    return {"median": round(statistics.median(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3), "unit": unit}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--codec", choices=["lz4", "zstd"], default="lz4")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("indirect_probe needs a GPU")
    L = zs.lib()
    N, cnt = args.ranges, args.count
    data = zs.synth_buffer(args.size)
    zstd = args.codec == "zstd"
    d_data = torch.from_numpy(data).to("cuda")
    if zstd:
        d_img = zs.zstd_build_image(d_data, FRAME)
        img = d_img
    else:
        img = zs.lz4_seekable(data, FRAME)
        d_img = torch.from_numpy(img).to("cuda")
    err = C.create_string_buffer(zs.ERRBUF)
    loose = 2 * N                                            # a range of <= 64 KiB touches at most two frames

    def open_reader():
        hh = L.zsk_reader_open_device(d_img.data_ptr(), d_img.numel(), 0, err)
        if not hh:
            sys.exit("open_device: " + err.value.decode())
        L.zsk_reader_set_batch_bytes(hh, loose * FRAME)      # one batch for every variant
        if zstd and not L.zsk_reader_set_zstd_async(hh, 3):
            sys.exit("set_zstd_async failed")
        return hh

    def device_memory(hh):
        g = zs.GpuStatsC()
        L.zsk_reader_gpu_stats_ex(hh, C.byref(g), C.sizeof(g))
        return int(g.device_memory)

    h = open_reader()
    census = None
    if zstd:
        c = zs.ZstdCensusC()
        # (a small read first: the reader's lane -- streams, events -- exists before the census is timed)
        warm = torch.empty(4096, dtype=torch.uint8, device="cuda")
        if L.zsk_pread_device(h, warm.data_ptr(), 4096, 0, None, err) != 4096:
            sys.exit("pread_device: " + err.value.decode())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if L.zsk_reader_zstd_census(h, C.byref(c), err) != 0:
            sys.exit("zstd census: " + err.value.decode())
        census = {k: int(getattr(c, k)) for k, _ in zs.ZstdCensusC._fields_}
        census["call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    S = torch.cuda.Stream()
    rng = np.random.default_rng(1)
    offs = np.sort(rng.integers(0, args.size - cnt, N)).astype(np.int64)
    rng.shuffle(offs)
    touched = len(set((offs // FRAME).tolist()) | set(((offs + cnt - 1) // FRAME).tolist()))
    tight = (touched + 255) // 256 * 256
    rg = np.zeros(N, zs.RANGE_DTYPE)
    rg["offset"], rg["count"], rg["dst_off"] = offs, cnt, np.arange(N, dtype=np.int64) * cnt
    d_rg = torch.from_numpy(rg.view(np.uint8).copy()).to("cuda")
    h_rg = torch.empty(d_rg.numel(), dtype=torch.uint8).pin_memory()
    d_buf = torch.empty(N * cnt, dtype=torch.uint8, device="cuda")
    d_res = torch.empty(N + 1, dtype=torch.int64, device="cuda")
    # the expected bytes, gathered once by torch from the payload
    idx = torch.from_numpy(offs).to("cuda")[:, None] + torch.arange(cnt, device="cuda")[None, :]
    want = d_data[idx.reshape(-1)]
    want_res = torch.tensor([cnt] * N + [N], dtype=torch.int64, device="cuda")
    del idx
    torch.cuda.synchronize()

    def today():
        h_rg.copy_(d_rg, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return L.zsk_preadv_device_async(h, d_buf.data_ptr(), h_rg.data_ptr(), N, d_res.data_ptr(), S.cuda_stream, None,
                                         err)

    def indirect(max_frames):
        return L.zsk_preadv_device_indirect(h, d_buf.data_ptr(), d_buf.numel(), d_rg.data_ptr(), N, max_frames,
                                            d_res.data_ptr(), S.cuda_stream, err)

    variants = {"today": today, "indirect": lambda: indirect(loose), "indirect_tight": lambda: indirect(tight)}
    memory = None
    if zstd:
        # each variant's first call on a reader of its own: what it makes the reader hold
        memory = {}
        keep = h
        for name, fn in variants.items():
            h = open_reader()
            if L.zsk_reader_zstd_census(h, C.byref(zs.ZstdCensusC()), err) != 0:
                sys.exit("zstd census: " + err.value.decode())
            base = device_memory(h)
            with torch.cuda.stream(S):
                ret = fn()
                S.synchronize()
            if ret != 0:
                sys.exit(f"{name}: {ret} {err.value.decode()}")
            memory[name] = {"before": base, "after": device_memory(h)}
            L.zseek_reader_close(h, None, None)
        h = keep
        blocks, seqs = census["max_blocks"], census["max_sequences"]
        memory["bounds"] = {
            "census": {mf: {"out_bytes": mf * FRAME, "max_blocks": mf * blocks, "max_sequences": mf * seqs}
                       for mf in (loose, tight)},
            # zsk_reader_set_zstd_async(3) for the frames the list touches
            "policy_touched": {"out_bytes": touched * FRAME, "max_blocks": touched * (2 + FRAME // 16384),
                               "max_sequences": touched * FRAME // 3}}
    times = {k: [] for k in variants}
    with torch.cuda.stream(S):
        for rep in range(args.runs + 1):
            for name, fn in variants.items():
                d_buf.zero_()
                d_res.zero_()
                S.synchronize()
                t0 = time.perf_counter()
                ret = fn()
                S.synchronize()
                t = time.perf_counter() - t0
                if ret != 0 or not torch.equal(d_buf, want) or not torch.equal(d_res, want_res):
                    raise RuntimeError(f"{name}: wrong bytes or results ({ret}) {err.value.decode()}")
                if rep:
                    times[name].append(t * 1e3)
    result = {"codec": args.codec, "input_bytes": args.size, "image_bytes": int(d_img.numel()), "ranges": N, "count": cnt, "runs": args.runs,
              "touched_frames": touched, "max_frames": {"indirect": loose, "indirect_tight": tight},
              "device": torch.cuda.get_device_name(0),
              "call_ms": {k: row(v, "ms") for k, v in times.items()}}
    if zstd:
        result["census"], result["device_memory"] = census, memory
        print(json.dumps({"census": census, "device_memory": memory}), flush=True)
    print(json.dumps({"call_ms": result["call_ms"], "touched_frames": touched}), flush=True)

    # GPU time by HIP events: a whole call, and a call that only plans (max_frames 1 overflows)
    timed = [("indirect", loose), ("indirect_tight", tight), ("plan_only", 1)]
    if zstd:
        timed.append(("today", 0))                           # the host-planned call's stages, to compare
    gpu = {name: [] for name, _ in timed}
    stages = {}
    with torch.cuda.stream(S):
        for name, mf in timed:
            L.zsk_kernel_timing(1)
            for rep in range(args.runs + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                S.synchronize()
                e0.record(S)
                ret = today() if name == "today" else indirect(mf)
                e1.record(S)
                S.synchronize()
                if ret != 0 or int(d_res[N]) != (zs.PLAN_OVERFLOW if name == "plan_only" else N):
                    raise RuntimeError(f"{name}: {ret} {err.value.decode()}")
                if rep:
                    gpu[name].append(e0.elapsed_time(e1))
            ms = (C.c_double * 8)()
            n = L.zsk_kernel_times(ms, 8)
            stages[name] = {"launches": n, "plan_parse_execute_handoff_ms": [round(ms[i], 4) for i in range(4)]}
            if zstd:   # (its spans: frame, sequence, Huffman and execute kernels, summed over the chunks)
                stages[name]["zstd_frame_seq_huf_exec_ms"] = [round(ms[i], 4) for i in range(4, 8)]
            L.zsk_kernel_timing(0)
    result["gpu_ms"] = {k: row(v, "ms") for k, v in gpu.items()}
    result["decode_stages"] = stages
    print(json.dumps({"gpu_ms": result["gpu_ms"], "decode_stages": stages}), flush=True)
    L.zseek_reader_close(h, None, None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
