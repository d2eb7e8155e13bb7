"""Vectored random reads against a zseek_pread loop: N random 4 KiB reads of
a 256 MiB LZ4 image (64 KiB frames, then 4 KiB frames), N = 1, 64, 1,024 and
16,384, as ONE zsk_preadv call and as N zseek_pread calls on the same library
(cache off; the loop runs in C, tools zsk_tool_latency).  Per point: the
median wall time of `--calls` calls (default 20) after `--warmup` (default 3),
as us per read, and the ratio.  Both sides' bytes are checked against the
generator afterwards.  With --stages, the two-phase decoder's per-stage times
(zsk_kernel_timing) of one more vectored call per point are printed too.

    python scripts/preadv_probe.py [--calls 20] [--warmup 3] [--mib 256] [--stages]

--async-mode measures zsk_preadv_device_async instead, on one device image
(64 KiB frames) in one process, the variants alternating, each figure the
median (min to max) of 5 rounds after a warm-up round: the host time of one
call of N = 1,024 ranges (the enqueue; the stream is synchronized outside the
timed window), the wall time of K = 32 back-to-back asynchronous calls plus
one synchronize against 32 synchronous zsk_preadv_device calls, and one call
of N = 16,384 (whose range_result_kernel time a kernel trace of this mode
gives: rocprofv3 --kernel-trace --stats -- python scripts/preadv_probe.py
--async-mode).  The bytes and results of both sides are checked.

    python scripts/preadv_probe.py --async-mode [--mib 256]
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
ap.add_argument("--async-mode", action="store_true")
args = ap.parse_args()

if args.async_mode:
    import torch   # (before the library is loaded, as scripts/image_probe.py does)
    assert torch.cuda.is_available(), "--async-mode needs a GPU"

READ = 4096
data = z.synth_buffer(args.mib << 20)
T, L = z.tools(), z.lib()


def async_mode():
    dev = torch.device("cuda", 0)
    K, N, NBIG, ROUNDS = 32, 1024, 16384, 5
    img = z.lz4_seekable(data, 65536)
    d_img = torch.from_numpy(img).to(dev)
    S = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(65536)

    def case(n):
        offs = rng.integers(0, data.size - READ, n).astype(np.uint64)
        rg = np.zeros(n, zs.RANGE_DTYPE)
        rg["offset"], rg["count"] = offs, READ
        rg["dst_off"] = np.arange(n, dtype=np.uint64) * READ
        want = np.concatenate([data[int(o): int(o) + READ] for o in offs])
        return rg, want, torch.zeros(n * READ, dtype=torch.uint8, device=dev), \
            torch.zeros(n + 1, dtype=torch.int64, device=dev)

    cases = [case(N) for _ in range(K)]
    big = case(NBIG)
    err = C.create_string_buffer(80)
    with zs.Reader.open_device(d_img.data_ptr(), img.size, 0) as r:
        def go_async(c):
            rg, _, d_buf, d_res = c
            assert L.zsk_preadv_device_async(r.handle, d_buf.data_ptr(), rg.ctypes.data, rg.size, d_res.data_ptr(),
                                             S.cuda_stream, None, err) == 0, err.value

        def go_sync(c):
            rg, _, d_buf, _ = c
            assert L.zsk_preadv_device(r.handle, d_buf.data_ptr(), rg.ctypes.data, rg.size, None, err) == rg.size

        t_host, t_async, t_sync, t_big = [], [], [], []
        for k in range(1 + ROUNDS):                        # round 0: the warm-up
            t0 = time.perf_counter()
            go_async(cases[0])
            t_host.append(time.perf_counter() - t0)
            S.synchronize()
            t0 = time.perf_counter()
            for c in cases:
                go_async(c)
            S.synchronize()
            t_async.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for c in cases:
                go_sync(c)
            t_sync.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            go_async(big)
            S.synchronize()
            t_big.append(time.perf_counter() - t0)
        for rg, want, d_buf, d_res in cases + [big]:       # (the last writer of every buffer: an asynchronous call)
            assert np.array_equal(d_buf.cpu().numpy(), want), "bytes"
            res = d_res.cpu().numpy()
            assert (res[:-1] == READ).all() and res[-1] == rg.size, "results"

    def mmm(v, scale):
        v = np.array(v[1:]) * scale
        return f"{np.median(v):.1f} ({v.min():.1f} to {v.max():.1f})"

    print(f"host time of one zsk_preadv_device_async call, N = {N:,}: {mmm(t_host, 1e6)} us")
    print(f"{K} asynchronous calls of N = {N:,} + one synchronize: {mmm(t_async, 1e3)} ms")
    print(f"{K} synchronous zsk_preadv_device calls of N = {N:,}:     {mmm(t_sync, 1e3)} ms")
    print(f"one asynchronous call of N = {NBIG:,} + synchronize:    {mmm(t_big, 1e3)} ms")


if args.async_mode:
    async_mode()
    sys.exit(0)
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
