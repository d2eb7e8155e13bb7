"""Which kernels each kind of LZ4 batch gets: a fixed list of named cases in one
process, for a `rocprofv3 --kernel-trace` run (nothing else traced).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/lz4_route_probe.py DIR/probe.json

Run once per switch setting (SETTINGS: the library reads its environment once).
Before the first case and after each one the probe launches one separator
kernel no case launches (zsk_frame_checksums' frame_xxh64_store_kernel), so
tests/golden/make_lz4_route_trace.py can cut the trace into cases; every
tensor, image and reader is made before the first separator, and a case is
library calls and a synchronize, nothing of torch's.

probe.json: per case the Lz4Request(s) (csrc/lz4_route.h) its launches are made
with -- written down here from the callers (launch_lz4_frames; decode_batch and
what reader.cpp / reader_vec.cpp put into it) -- and the strings
zs.parse_kernel_name / zsk_lz4_kernel_name return for NAME_PAIRS."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEPARATOR = "frame_xxh64_store_kernel"
SETTINGS = {
    "default": {},
    "one_route_0": {"ZSEEK_ONE_ROUTE": "0"},
    "one_big_0": {"ZSEEK_ONE_BIG": "0"},
    "one_blocks_0": {"ZSEEK_ONE_BLOCKS": "0"},
    "one_exec_wave": {"ZSEEK_ONE_EXEC": "wave"},
    "parse_scan": {"ZSEEK_PARSE": "scan"},
    "parse_chunk": {"ZSEEK_PARSE": "chunk"},
    "block_route_0": {"ZSEEK_BLOCK_ROUTE": "0"},
    "hip_kernel_wave": {"ZSEEK_HIP_KERNEL": "wave"},
}
SWITCHES = ["ZSEEK_HIP_KERNEL", "ZSEEK_PARSE", "ZSEEK_BLOCK_ROUTE", "ZSEEK_ONE_ROUTE", "ZSEEK_ONE_BIG",
            "ZSEEK_ONE_BLOCKS", "ZSEEK_ONE_EXEC"]
# kOneMaxFrames, the plan's single workgroup, the block route's and the chunk
# parse's batch bounds
NFRAMES = [1, 2, 64, 65, 255, 256, 257, 1023, 1024, 32767, 32768]
NAME_CSIZES = [170, 8191, 8192, 12287, 12288, 49151, 49152, 65535, 65536, 530754]
NONE = 0xFFFFFFFF
GOLDEN = os.path.join(ROOT, "tests", "golden")


def request(nframes, route=0, stop_last=NONE, max_dsize=NONE, in_order=False, scan_layout=False, post=False):
    return {"nframes": nframes, "route": route, "stages": 15, "tune": 0, "stop_last": stop_last,
            "max_dsize": max_dsize, "in_order": in_order, "scan_layout": scan_layout, "post": post}


def main(out_path: str) -> None:
    import torch

    import libzseek_amd.zseek as zs
    gpu = torch.device("cuda", 0)
    cases = []   # (name, requests, callable)

    # ---- device API: every decoder x batch size, a few tiny frames repeated ----
    tiny = zs.lz4_seekable((np.arange(600) * 7 % 251).astype(np.uint8), 150)
    c_off, d_off = zs.seek_table_of(tiny)
    fr = [(tiny[int(c_off[i]): int(c_off[i + 1])], int(d_off[i + 1] - d_off[i])) for i in range(len(c_off) - 1)]
    assert len(fr) == 4 and all(len(f) < 200 for f, _ in fr)
    batches = {}
    for n in NFRAMES:
        pick = [fr[i % 4] for i in range(n)]
        c = np.cumsum([0] + [len(f) for f, _ in pick])
        d = np.cumsum([0] + [s for _, s in pick])
        desc = np.zeros(n, zs.FRAME_DESC_DTYPE)
        desc["c_off"], desc["d_off"], desc["c_size"], desc["d_size"] = c[:-1], d[:-1], np.diff(c), np.diff(d)
        comp = torch.zeros(int(c[-1]) + 256, dtype=torch.uint8, device=gpu)
        comp[: int(c[-1])].copy_(torch.from_numpy(np.concatenate([f for f, _ in pick])))
        batches[n] = (torch.from_numpy(desc.view(np.uint8).copy()).to(gpu), comp,
                      torch.zeros(int(d[-1]), dtype=torch.uint8, device=gpu),
                      torch.zeros(n, dtype=torch.int32, device=gpu))
    for engine, route in zs.DECODERS.items():
        for n in NFRAMES:
            cases.append((f"api/{engine}/{n}", [request(n, route)],
                          lambda n=n, engine=engine: zs.decode_frames(*batches[n], engine=engine)))

    # ---- readers: the committed 64 KiB and 1 MiB files, and 66 frames of 64 KiB ----
    img64 = np.fromfile(os.path.join(GOLDEN, "lz4_64k_direct.zs"), np.uint8)
    img1m = np.fromfile(os.path.join(GOLDEN, "lz4_1m_direct.zs"), np.uint8)
    img66 = zs.lz4_seekable(zs.synth_buffer(66 << 16), 65536)
    F, M = 65536, 1 << 20
    keep = []

    def reader(img, cache=0):
        keep.append(zs.Reader(img, cache))
        return keep[-1]

    def device_reader(img):
        t = torch.zeros(img.size + 64, dtype=torch.uint8, device=gpu)
        t[: img.size].copy_(torch.from_numpy(img))
        keep.append((t, zs.Reader.open_device(t.data_ptr(), img.size, 0)))
        return keep[-1][1]

    scattered = [(F + 10, 100), (5 * F + 7, 200), (9 * F, 300)]
    for where, opener in (("host", reader), ("image", device_reader)):
        def add(name, requests, img, call, cache=0):
            r = opener(img, cache) if opener is reader else opener(img)
            cases.append((f"{where}/{name}", requests, lambda: call(r)))

        add("4k_cache0", [request(1, 0, 4196, F, True, False, True)], img64, lambda r: r.pread(4096, 3 * F + 100))
        if opener is reader:   # (the cached frame: a host reader's)
            add("4k_cache1", [request(1, 0, NONE, F, True, False, True)], img64,
                lambda r: r.pread(4096, 3 * F + 100), cache=1)
        add("2_frames", [request(2, 0, 4564, F, True)], img64, lambda r: r.pread(70000, 3 * F + 100))
        # (a request's first batch is 4 MiB: 64 frames, then the 65th alone)
        add("65_frames_pread", [request(64, 0, NONE, F, True), request(1, 0, NONE, F, True, False, True)], img66,
            lambda r: r.pread(65 * F, 0))
        add("65_frames_preadv", [request(65, 0, NONE, F, True)], img66, lambda r: r.preadv([(0, 65 * F)]))
        add("1m_frame", [request(1, 0, NONE, M, True, False, True)], img1m, lambda r: r.pread(M, 0))
        add("1m_two_frames", [request(2, 0, NONE, M, True)], img1m, lambda r: r.pread(2 * M, 0))
        add("preadv_scattered", [request(3, 0, NONE, F, True)], img64, lambda r: r.preadv(scattered))
    # the device-planned read: max_frames descriptors anywhere in the image (the plan's scan layout)
    rg = zs.Reader._ranges(scattered)
    d_rg = torch.from_numpy(rg.view(np.uint8).copy()).to(gpu)
    d_buf = torch.zeros(1024, dtype=torch.uint8, device=gpu)
    d_res = torch.zeros(len(rg) + 1, dtype=torch.int64, device=gpu)
    for max_frames in (4, 65):
        r = device_reader(img64 if max_frames == 4 else img66)
        cases.append((f"image/indirect_{max_frames}", [request(max_frames, 0, NONE, F, False, True)],
                      lambda r=r, m=max_frames: r.preadv_device_indirect(d_buf.data_ptr(), 1024, d_rg.data_ptr(),
                                                                         len(rg), m, d_res.data_ptr())))

    # ---- the separator, and the run ----
    sep_desc = np.zeros(1, zs.FRAME_DESC_DTYPE)
    sep_desc["d_size"] = 64
    sep = (torch.from_numpy(sep_desc.view(np.uint8).copy()).to(gpu), torch.zeros(64, dtype=torch.uint8, device=gpu),
           torch.zeros(1, dtype=torch.int32, device=gpu))
    torch.cuda.synchronize()

    def separator():
        zs.frame_checksums(*sep)
        torch.cuda.synchronize()

    separator()
    for _, _, call in cases:
        call()
        torch.cuda.synchronize()
        separator()
    for k in keep:
        (k[1] if isinstance(k, tuple) else k).close()

    names = [[n, c, zs.parse_kernel_name(n, c), zs.lib().zsk_lz4_kernel_name(n).decode()]
             for n in NFRAMES for c in NAME_CSIZES]
    json.dump({"separator": SEPARATOR, "env": {k: os.environ[k] for k in SWITCHES if k in os.environ},
               "cases": [{"name": name, "requests": rq} for name, rq, _ in cases], "names": names},
              open(out_path, "w"))
    print(f"{len(cases)} cases")


if __name__ == "__main__":
    main(sys.argv[1])
