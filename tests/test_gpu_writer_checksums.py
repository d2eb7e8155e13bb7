"""Seek-table checksums computed on the GPU and writes from device memory:
zsk_frame_checksums against the oracle's XXH64 over every tail length,
unaligned frames and partial waves; the GPU-mode writer with checksums on
against the host writer; the checksummed file back through the verifying
reader; zsk_write_device against a host writer fed the loop of zseek_write
calls it stands for, on its fast path and every fallback."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def data(zs):
    """12 MiB of the synthetic plus a tail, on the host and (lazily) the device."""
    return bytes(zs.synth_buffer(12 * MIB)) + b"end" * 1000


@pytest.fixture(scope="module")
def d_data(gpu, data):
    """The same bytes in device memory, 3 bytes into their tensor."""
    import torch
    t = torch.empty(len(data) + 3, dtype=torch.uint8, device=gpu)
    t[3:].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    torch.cuda.synchronize()
    return t


# ---------------------------------------------------------------------------
# zsk_frame_checksums
# ---------------------------------------------------------------------------
def _checksums(zs, gpu, buf: bytes, offs, sizes):
    import torch
    n = len(sizes)
    desc = np.zeros(n, zs.FRAME_DESC_DTYPE)
    desc["d_off"], desc["d_size"] = offs, sizes
    desc["c_off"], desc["c_size"] = 0xDEADBEEF, 0x7FFFFFFF      # ignored
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    d_buf = torch.frombuffer(bytearray(buf) or bytearray(1), dtype=torch.uint8).to(gpu)
    out = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    zs.frame_checksums(d_desc, d_buf, out[4: 4 + n])
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[:4] == 0x5A5A5A5A).all() and (got[4 + n:] == 0x5A5A5A5A).all(), "sentinels"
    return got[4: 4 + n]


def test_frame_checksums_lengths_and_alignment(gpu, zs, oracle, data):
    sizes = [0, 1, 3, 4, 7, 8, 12, 31, 32, 33, 64, 95, 96, 127, 128, 129, 65536, 65537, 4 * MIB + 5]
    offs = np.concatenate(([0], np.cumsum(sizes)[:-1]))      # back to back: mostly unaligned
    buf = data[: int(sum(sizes))]
    order = np.random.default_rng(3).permutation(len(sizes))
    got = _checksums(zs, gpu, buf, offs[order], np.array(sizes)[order])
    want = [oracle.xxh64(buf[int(offs[i]): int(offs[i]) + sizes[i]]) & 0xFFFFFFFF for i in order]
    assert got.tolist() == want
    assert want[list(order).index(0)] == 0x51D8E999           # the empty frame


def test_frame_checksums_one_past_a_full_wave(gpu, zs, oracle, data):
    sizes = [64] * 17
    offs = [5 + 64 * i for i in range(17)]
    got = _checksums(zs, gpu, data[: 5 + 64 * 17], offs, sizes)
    assert got.tolist() == [oracle.xxh64(data[o: o + 64]) & 0xFFFFFFFF for o in offs]


def test_frame_checksums_no_frames(gpu, zs):
    assert zs.lib().zsk_frame_checksums(None, 0, None, None, None) == 0


# ---------------------------------------------------------------------------
# the GPU-mode writer with checksums on
# ---------------------------------------------------------------------------
def _writes(data: bytes, sizes):
    out, at, i = [], 0, 0
    while at < len(data):
        n = sizes[i % len(sizes)]
        out.append(data[at: at + n])
        at += n
        i += 1
    return out


def _file(zs, chunks, min_frame, level=0, gpu_batch=None, checksums=True, **kw):
    w = zs.Writer(zs.ZSEEK_LZ4, min_frame, level=level, **kw)
    if checksums:
        assert w.set_checksums(True)
    if gpu_batch is not None:
        assert w.set_gpu_compress(gpu_batch)
    for i, c in enumerate(chunks):
        w.write(c, call_data=i + 1)
    return w.close(), w


# test_gpu_writer_compress.py's write sequences, and one whose writes span
# several flushes
CASES = [
    (65536, [65536], 0, 0),               # direct frames (config 2's writer)
    (4096, [4096], 0, 65536),             # small direct frames, batch flushed every 16
    (4096, [1000], 0, 0),                 # buffered frames (content size)
    (60000, [7000, 300, 65536], -2, 0),   # mixed buffered / direct, negative level
    (20000, [30000, 200000, 100], 0, 0),  # linked frames > 64 KiB on the GPU
    (1 << 20, [1 << 20], 0, 0),           # the reference example's 1 MiB frames
    (20000, [30000, 5 << 20, 100], 0, 0), # frames > 4 MiB go to the host, in order
    (1, [1, 2, 3], 0, 65536),             # tiny frames
    (65536, [65536], 0, 131072),          # a flush every second frame
]


@pytest.mark.parametrize("min_frame,sizes,level,batch", CASES)
def test_gpu_writer_checksums_match_host(gpu, zs, data, min_frame, sizes, level, batch):
    d = data if max(sizes) > MIB else data[: 3 * MIB] + data[-3000:]
    if min_frame == 1:
        d = d[:20000]
    chunks = _writes(d, sizes)
    host, hw = _file(zs, chunks, min_frame, level)
    dev, dw = _file(zs, chunks, min_frame, level, gpu_batch=batch)
    assert host[-5] == 0x80
    assert dev == host
    assert dw.call_data_seen == hw.call_data_seen


@pytest.mark.parametrize("cache", [0, 1])
def test_checksummed_file_reads_back_verified(gpu, zs, data, cache):
    d = data[: 3 * MIB + 777]
    dev, _ = _file(zs, _writes(d, [65536, 1000, 200000]), 20000, gpu_batch=0)
    assert dev[-5] == 0x80
    with zs.Reader(dev, cache) as r:
        r.set_verify_checksums(True)
        assert r.read_all(len(d), 0) == d


def test_corrupted_checksum_is_caught(gpu, zs, data):
    """The table the writer produced is the one the reader verifies: a flipped
    checksum bit fails the read."""
    d = data[: 4 * 65536]
    dev, _ = _file(zs, _writes(d, [65536]), 65536, gpu_batch=0)
    bad = bytearray(dev)
    bad[-9 - 12 * 2 - 1] ^= 1            # frame 2's checksum (third entry from the end: 4 entries)
    with zs.Reader(bytes(bad), 0) as r:
        r.set_verify_checksums(True)
        with pytest.raises(zs.ZseekError, match="checksum"):
            r.read_all(len(d), 0)


# ---------------------------------------------------------------------------
# zsk_write_device
# ---------------------------------------------------------------------------
def _as_if(zs, ops, data, min_frame, checksums, ctype=None, **kw):
    """A host-mode writer fed what the ops stand for.  ops: ("host", a, b) =
    zseek_write(data[a:b]); ("dev", a, b, write_size) = zsk_write_device."""
    w = zs.Writer(zs.ZSEEK_LZ4 if ctype is None else ctype, min_frame, **kw)
    if checksums:
        assert w.set_checksums(True)
    for i, op in enumerate(ops):
        if op[0] == "host":
            w.write(data[op[1]: op[2]], call_data=i + 1)
            continue
        _, a, b, ws = op
        ws = ws or (b - a)
        o = a
        while True:
            w.write(data[o: min(o + ws, b)] if ws else b"", call_data=i + 1)
            o += ws
            if o >= b or ws == 0:
                break
    return w


def _device(zs, ops, data, d_data, min_frame, checksums, gpu_batch, ctype=None, **kw):
    w = zs.Writer(zs.ZSEEK_LZ4 if ctype is None else ctype, min_frame, **kw)
    if checksums:
        assert w.set_checksums(True)
    if gpu_batch is not None:
        assert w.set_gpu_compress(gpu_batch)
    base = d_data.data_ptr() + 3
    for i, op in enumerate(ops):
        if op[0] == "host":
            w.write(data[op[1]: op[2]], call_data=i + 1)
        else:
            w.write_device(base + op[1], op[2] - op[1], op[3], call_data=i + 1)
    return w


LEN1 = MIB + 1000
# (min_frame, gpu_batch (None: GPU mode off), codec (None: LZ4), ops)
DEVICE_CASES = {
    "fast_tail": (65536, 0, None, [("dev", 0, LEN1, 65536)]),
    "fast_eight_launches": (65536, 131072, None, [("dev", 0, LEN1, 65536)]),
    "fast_linked": (20000, 0, None, [("dev", 0, MIB, 200000)]),
    "fallback_buffered": (4096, 0, None, [("dev", 0, 20500, 1000)]),
    "fallback_host_lz4": (65536, 0, None, [("dev", 0, 11 * MIB, 5 * MIB)]),
    "write_size_0": (65536, 0, None, [("dev", 0, 300000, 0)]),
    "len_0": (0, 0, None, [("dev", 0, 0, 0), ("dev", 5, 5, 4096), ("dev", 0, 1000, 0)]),
    "interleaved": (65536, 0, None, [("host", 0, 65536), ("dev", 65536, 5 * 65536, 65536), ("host", 5 * 65536, 5 * 65536 + 100),
                                     ("dev", 5 * 65536 + 100, 9 * 65536, 65536), ("host", 9 * 65536, 10 * 65536),
                                     ("dev", 10 * 65536, 10 * 65536 + 70000, 65536), ("dev", 10 * 65536 + 70000, 12 * 65536, 0)]),
    "gpu_mode_off": (65536, None, None, [("dev", 0, LEN1, 65536)]),
    "zstd": (50000, None, 0, [("dev", 0, 300000, 70000)]),
}


@pytest.mark.parametrize("checksums", [False, True])
@pytest.mark.parametrize("case", list(DEVICE_CASES))
def test_write_device_equals_the_loop_of_writes(gpu, zs, data, d_data, case, checksums):
    min_frame, batch, ctype, ops = DEVICE_CASES[case]
    hw = _as_if(zs, ops, data, min_frame, checksums, ctype)
    dw = _device(zs, ops, data, d_data, min_frame, checksums, batch, ctype)
    sh, sd = hw.stats(), dw.stats()
    for k in ("frames", "compressed_size", "seek_table_size"):
        assert sh[k] == sd[k], k
    host, dev = hw.close(), dw.close()
    assert dev == host
    assert dw.call_data_seen == hw.call_data_seen
    assert dev[-5] == (0x80 if checksums else 0)


def test_write_device_returns_with_nothing_queued(gpu, zs, data, d_data):
    """Synchronous: the frames' callbacks have run when the call returns, the
    frames queued by earlier zseek_write calls before them."""
    w = zs.Writer(zs.ZSEEK_LZ4, 65536)
    assert w.set_gpu_compress(0)
    w.write(data[:65536])
    assert w.callbacks == 0                     # queued
    w.write_device(d_data.data_ptr() + 3 + 65536, 4 * 65536, 65536)
    assert w.callbacks == 5
    w.write_device(d_data.data_ptr() + 3 + 5 * 65536, 4096, 1000)    # fallback: buffered, then flushed
    assert w.callbacks == 5 and w.stats()["frames"] == 6
    w.close()


def test_write_device_refuses_pinned_host_memory(gpu, zs, data):
    import torch
    t = torch.frombuffer(bytearray(data[:65536]), dtype=torch.uint8).pin_memory()
    for batch in (0, None):
        w = zs.Writer(zs.ZSEEK_LZ4, 65536)
        if batch is not None:
            assert w.set_gpu_compress(batch)
        with pytest.raises(zs.ZseekError, match="write from device: not device memory of the writer's device"):
            w.write_device(t.data_ptr(), 65536, 65536)
        assert w.callbacks == 0 and w.stats()["frames"] == 0
        img = w.close()
        assert len(img) == 8 + 9                # an empty seek table: nothing was written
    err = zs.C.create_string_buffer(80)
    assert zs.lib().zsk_write_device(None, t.data_ptr(), 1, 0, None, err) is False
    assert err.value == b"invalid writer"


def test_write_device_callback_failure(gpu, zs, data, d_data):
    d = data[: 8 * 65536]
    host, _ = _file(zs, _writes(d, [65536]), 65536, checksums=False)
    w = zs.Writer(zs.ZSEEK_LZ4, 65536, fail_on_callback=3)
    assert w.set_gpu_compress(0)
    with pytest.raises(zs.ZseekError):
        w.write_device(d_data.data_ptr() + 3, len(d), 65536)
    c_off, _ = zs.seek_table_of(np.frombuffer(host, np.uint8))
    assert bytes(w._out) == host[: int(c_off[2])]          # frames 1-2 written, the 3rd refused
    with pytest.raises(zs.ZseekError):
        w.write_device(d_data.data_ptr() + 3, 65536, 65536)
    with pytest.raises(zs.ZseekError):
        w.write(d[:65536])
    with pytest.raises(zs.ZseekError):
        w.close()
    assert int.from_bytes(bytes(w._out)[-9:-5], "little") == 2     # close's seek table: 2 frames
