"""Vectored random reads against a zseek_pread loop: N random 4 KiB reads of
a 256 MiB LZ4 image (64 KiB frames, then 4 KiB frames), N = 1, 64, 1,024 and
16,384, as ONE zsk_preadv call and as N zseek_pread calls on the same library
(cache off; the loop runs in C, tools zsk_tool_latency).  Per point: the
median wall time of `--calls` calls (default 20) after `--warmup` (default 3),
as us per read, and the ratio.  Both sides' bytes are checked against the
generator afterwards.  With --stages, the two-phase decoder's per-stage times
(zsk_kernel_timing) of one more vectored call per point are printed too.

    python scripts/preadv_probe.py [--calls 20] [--warmup 3] [--mib 256] [--stages]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libzseek_amd as z  # noqa: E402
from libzseek_amd import zseek as zs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--stages", action="store_true")
ap.add_argument("--n", type=int, nargs="*", default=[1, 64, 1024, 16384])
args = ap.parse_args()

READ = 4096
data = z.synth_buffer(args.mib << 20)
T, L = z.tools(), z.lib()
fn = [C.cast(f, C.c_void_p) for f in (L.zseek_reader_open_full, L.zseek_pread, L.zseek_reader_close)]
err = C.create_string_buffer(80)
rows = []
for frame in (65536, 4096):
    img = z.lz4_seekable(data, frame)
    r = T.zsk_tool_open_mem(fn[0], img.ctypes.data, img.size, 0, err)
    assert r, err.value
    rng = np.random.default_rng(frame)
    for n in args.n:
        offs = rng.integers(0, data.size - READ, n).astype(np.uint64)
        want = np.concatenate([data[int(o): int(o) + READ] for o in offs])
        # the loop: N zseek_pread calls, timed as one pass in C
        one = np.empty(READ, np.uint8)
        ns = np.zeros(n, np.uint64)
        failed = C.c_size_t(0)
        t_loop = []
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            assert T.zsk_tool_latency(fn[1], r, offs.ctypes.data, n, READ, one.ctypes.data, ns.ctypes.data,
                                      C.byref(failed)) == 0
            t_loop.append(time.perf_counter() - t0)
        out = np.zeros(n * READ, np.uint8)   # (an untimed pass into separate buffers, to check the bytes)
        for i in range(n):
            assert L.zseek_pread(r, out.ctypes.data + i * READ, READ, int(offs[i]), None, err) == READ
        assert np.array_equal(out, want), "zseek_pread loop mismatch"
        # the vectored call
        rg = np.zeros(n, zs.RANGE_DTYPE)
        rg["offset"], rg["count"] = offs, READ
        rg["dst_off"] = np.arange(n, dtype=np.uint64) * READ
        out = np.zeros(n * READ, np.uint8)
        t_vec = []
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            ret = L.zsk_preadv(r, out.ctypes.data, rg.ctypes.data, n, None, err)
            t_vec.append(time.perf_counter() - t0)
            assert ret == n, (ret, err.value)
        assert np.array_equal(out, want) and (rg["result"] == READ).all(), "zsk_preadv mismatch"
        loop_us = float(np.median(t_loop[args.warmup:])) * 1e6 / n
        vec_us = float(np.median(t_vec[args.warmup:])) * 1e6 / n
        row = {"frame": frame, "n": n, "pread_loop_us_per_read": round(loop_us, 2),
               "preadv_us_per_read": round(vec_us, 2), "ratio": round(loop_us / vec_us, 2)}
        if args.stages:
            z.kernel_timing(True)
            L.zsk_preadv(r, out.ctypes.data, rg.ctypes.data, n, None, err)
            launches, st = z.kernel_times()
            z.kernel_timing(False)
            row["stages_ms"] = {k: round(v, 4) for k, v in st.items()}
            row["launches"] = launches
        rows.append(row)
        print(json.dumps(row), flush=True)
    T.zsk_tool_close_mem(fn[2], r)

print("\n| frames | N | zseek_pread loop, us / read | zsk_preadv, us / read | loop / preadv |")
print("|---|---|---|---|---|")
for w in rows:
    print(f"| {w['frame'] // 1024} KiB | {w['n']:,} | {w['pread_loop_us_per_read']} | {w['preadv_us_per_read']} | "
          f"{w['ratio']} |")
