"""bench.py's command line: a plain run does the timed steps and prints the
line (everything beside it is null), `--full` adds the verification, the
stage times and the legs beside the line, and `--dump-outputs DIR` writes
what the last timed step left in the caller's buffers, the same from run to
run."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = 65536


def run_bench(*argv, timeout=110):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *map(str, argv)],
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def load_dump(path, names):
    assert sorted(os.listdir(path)) == sorted(n + ".npy" for n in names)
    d = {n: np.load(os.path.join(path, n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    return d


def frame_sums(data: np.ndarray) -> np.ndarray:
    return data.reshape(-1, FRAME).sum(axis=1, dtype=np.int64).astype(np.float64)


PLAIN_NULL = ("cpu_baseline", "end_to_end", "latency_4k_us", "reassembly", "verified_bit_exact")


def test_dump_outputs_ragged_frames_with_gaps(tmp_path):
    """Frames of unequal sizes with bytes between them (as the compressor's
    slots have): exact sums of every frame, empty frames included, and no
    sampled byte from outside a frame; groups smaller than the buffer."""
    import bench
    rng = np.random.default_rng(3)
    sizes = rng.integers(0, 5000, 301)
    sizes[[0, 17, 300]] = 0
    slots = sizes + rng.integers(0, 40, 301)
    offs = np.concatenate([[0], np.cumsum(slots)[:-1]])
    buf = np.full(int(slots.sum()), 255, np.uint8)       # 255 = outside every frame
    for o, s in zip(offs, sizes):
        buf[o:o + s] = rng.integers(0, 100, s)
    want = np.array([buf[o:o + s].sum(dtype=np.int64) for o, s in zip(offs, sizes)], np.float64)
    old = bench.DUMP_GROUP
    bench.DUMP_GROUP = 7000                               # several frames, then one, per group
    try:
        for d in ("a", "b"):
            bench.dump_outputs(str(tmp_path / d), torch, {"csize": torch.from_numpy(sizes.astype(np.int32))},
                               torch.from_numpy(buf), offs, sizes, "compressed_sample")
    finally:
        bench.DUMP_GROUP = old
    a = load_dump(tmp_path / "a", ["csize", "frame_byte_sums", "compressed_sample"])
    b = load_dump(tmp_path / "b", ["csize", "frame_byte_sums", "compressed_sample"])
    assert np.array_equal(a["csize"], sizes)
    assert np.array_equal(a["frame_byte_sums"], want)
    assert a["compressed_sample"].size == min(bench.DUMP_SAMPLE, sizes.sum())
    assert a["compressed_sample"].max() < 100
    for k in a:
        assert np.array_equal(a[k], b[k])


def test_plain_run_is_lean_and_dumps_reproducibly(tmp_path, zs):
    """The CPU rehearsal (`--harness-check`: the expected bytes stand in for
    the decode) of a plain one-GPU run, twice: --steps sets the timed steps,
    the line carries ms_per_step and nulls for what --full would add, and the
    two dumps are equal, and equal to the generator's bytes."""
    lines = [run_bench("--gpus", 1, "--harness-check", "--size", "4M", "--steps", 3, "--warmup", 1,
                       "--dump-outputs", tmp_path / d) for d in ("a", "b")]
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
        assert d["ms_per_step"] > 0 and d["unit"] == "GB/s" and d["higher_is_better"] is True
        assert d["dtype"] == "u8" and "metric" in d and "value" in d
        assert all(d[k] is None for k in PLAIN_NULL)
        assert d["roofline"]["stages"] is None and d["roofline"]["kernel"] is None
    names = ["status", "frame_byte_sums", "decoded_sample"]
    a, b = load_dump(tmp_path / "a", names), load_dump(tmp_path / "b", names)
    for k in names:
        assert np.array_equal(a[k], b[k]), k
    data = zs.synth_buffer(4 << 20, 4)
    assert np.array_equal(a["status"], np.zeros(64, np.float32))
    assert np.array_equal(a["frame_byte_sums"], frame_sums(data))
    assert a["decoded_sample"].size == 4 << 20


@pytest.mark.gpu
def test_gpu_plain_run_dump_matches_generator(gpu, zs, tmp_path):
    d = run_bench("--gpus", 1, "--size", "64M", "--steps", 3, "--warmup", 1, "--threads", 8,
                  "--dump-outputs", tmp_path)
    assert d["steps"] == 3 and d["value"] > 0
    assert d["ms_per_step"] == pytest.approx((64 << 20) / d["value"] / 1e6, rel=1e-2)
    assert all(d[k] is None for k in PLAIN_NULL)
    assert d["roofline"]["stages"] is None and d["roofline"]["achieved"] > 0
    got = load_dump(tmp_path, ["status", "frame_byte_sums", "decoded_sample"])
    data = zs.synth_buffer(64 << 20, 8)
    assert np.array_equal(got["status"], np.zeros(1024, np.float32))
    assert np.array_equal(got["frame_byte_sums"], frame_sums(data))
    # the sample is bytes of the generator's buffer: same histogram support
    assert set(np.unique(got["decoded_sample"])) <= set(np.unique(data).astype(np.float32))


@pytest.mark.gpu
def test_gpu_plain_compress_run_dump_matches_liblz4(gpu, zs, tmp_path):
    d = run_bench("--gpus", 1, "--codec", "lz4c", "--size", "64M", "--steps", 2, "--warmup", 1,
                  "--threads", 8, "--dump-outputs", tmp_path)
    assert d["steps"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
    assert all(d[k] is None for k in ("cpu_baseline", "verified_bit_exact", "launch_by_frames",
                                      "writer_end_to_end"))
    got = load_dump(tmp_path, ["csize", "frame_byte_sums", "compressed_sample"])
    data = zs.synth_buffer(64 << 20, 8)
    img = np.asarray(zs.lz4_seekable(data, FRAME, 0, 8))
    c_off, _ = zs.seek_table_of(img)
    assert np.array_equal(got["csize"], np.diff(c_off.astype(np.int64)))
    want = [img[int(c_off[f]): int(c_off[f + 1])].sum(dtype=np.int64) for f in range(1024)]
    assert np.array_equal(got["frame_byte_sums"], np.array(want, np.float64))


@pytest.mark.gpu
def test_gpu_full_run_keeps_every_leg(gpu):
    d = run_bench("--gpus", 1, "--full", "--size", "64M", "--steps", 2, "--warmup", 1, "--threads", 8)
    assert d["verified_bit_exact"] is True
    assert d["roofline"]["kernel"] and set(d["roofline"]["stages"]) >= {"plan", "parse", "execute"}
    assert d["end_to_end"]["GBps"] > 0 and d["end_to_end"]["GBps_io8"] > 0
    assert d["latency_4k_us"]["cache0"]["requests"] == 1000
    assert d["cpu_baseline"]["kind"] == "reference"
