"""The writer's seek-table checksums (zsk_writer_set_checksums, env
ZSEEK_WRITE_CHECKSUMS), on the CPU: every host write path of both codecs
produces the file it produces without checksums, with the seek table replaced
by the 12-byte-entry table (descriptor 0x80) carrying the low 32 bits of
XXH64 of each frame's bytes; stats count 12 bytes per frame; the switch only
moves before the first byte; the reference's reader and the oracle read the
files."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LZ4, ZSTD = 1, 0
# (codec, min_frame_size, write sizes (cycled), payload bytes, nb_workers)
CASES = {
    "lz4_direct_64k": (LZ4, 65536, [65536], 300000, 1),
    # every write a frame: the lengths around XXH64's 32-byte stripe and its
    # 8- and 4-byte tail steps, and an empty frame
    "lz4_every_write": (LZ4, 0, [0, 1, 31, 32, 33, 63, 64, 65, 4095], 0 + 1 + 31 + 32 + 33 + 63 + 64 + 65 + 4095, 1),
    "lz4_buffered": (LZ4, 4096, [1000], 20500, 1),
    "lz4_mixed": (LZ4, 60000, [7000, 300, 65536], 300000, 1),
    "zstd_oneshot": (ZSTD, 50000, [70000], 300000, 1),
    "zstd_workers": (ZSTD, 50000, [1000, 37, 70000, 5], 300000, 2),
}


def _chunks(data: bytes, sizes):
    out, at, i = [], 0, 0
    while at < len(data) or (i < len(sizes) and sizes[i] == 0):
        n = sizes[i % len(sizes)]
        out.append(data[at: at + n])
        at += n
        i += 1
    return out


def _write(zs, case, checksums, data):
    codec, min_frame, sizes, _, workers = CASES[case]
    w = zs.Writer(codec, min_frame, nb_workers=workers)
    if checksums:
        assert w.set_checksums(True)
    for c in _chunks(data, sizes):
        w.write(c)
    return w.close()


@pytest.fixture(scope="module")
def payload(zs):
    return bytes(zs.synth_buffer(300000))


def _expected(zs, oracle, off: bytes, data: bytes) -> bytes:
    """The checksums-off file with the checksummed seek table in place of its
    own, the frames taken from its seek table over the payload."""
    _, d_off = zs.seek_table_of(np.frombuffer(off, np.uint8))
    assert int(d_off[-1]) == len(data)
    cks = [oracle.xxh64(data[int(d_off[i]): int(d_off[i + 1])]) & 0xFFFFFFFF for i in range(len(d_off) - 1)]
    return zs.with_frame_checksums(off, cks).tobytes()


@pytest.mark.parametrize("case", list(CASES))
def test_file_is_the_plain_file_with_a_checksummed_table(zs, oracle, payload, case):
    """zstd_workers: nb_workers = 2 takes the streaming path (write_mt /
    end_frame), where a frame's bytes arrive over several writes and the hash
    state is carried in the writer; it streams on the calling thread where
    libzstd has no worker threads."""
    data = payload[: CASES[case][3]]
    off = _write(zs, case, False, data)
    on = _write(zs, case, True, data)
    assert on[-5] == 0x80 and off[-5] == 0
    assert on == _expected(zs, oracle, off, data)


def test_empty_frame_checksum_value(zs):
    """XXH64 of no bytes is 0xEF46DB3751D8E999: an empty frame's entry carries
    its low half."""
    w = zs.Writer(LZ4, 0)
    assert w.set_checksums(True)
    w.write(b"")
    img = w.close()
    assert int.from_bytes(img[-9 - 4: -9], "little") == 0x51D8E999


@pytest.mark.parametrize("codec", [LZ4, ZSTD])
def test_stats_count_twelve_bytes_per_frame(zs, payload, codec):
    w = zs.Writer(codec, 50000)
    assert w.set_checksums(True)
    w.write(payload[:70000])
    w.write(payload[70000:140000])
    st = w.stats()
    assert st["frames"] == 2 and st["seek_table_size"] == 8 + 12 * 2 + 9
    size_now = st["compressed_size"]
    w.write(payload[140000:141000])         # buffered: a pending frame
    st = w.stats()
    assert st["frames"] == 3 and st["seek_table_size"] == 8 + 12 * 2 + 9 + 12
    assert st["compressed_size"] == size_now + 12
    assert w.close()[-5] == 0x80
    # with nothing pending the stats are the closed file's
    w = zs.Writer(codec, 50000)
    assert w.set_checksums(True)
    w.write(payload[:70000])
    w.write(payload[70000:140000])
    st = w.stats()
    img = w.close()
    assert st["seek_table_size"] == 8 + 12 * 2 + 9 and st["compressed_size"] == len(img)


def test_setting_rules(zs, payload):
    w = zs.Writer(LZ4, 65536)
    assert w.set_checksums(True) and w.set_checksums(False) and w.set_checksums(True)
    assert w.set_checksums(True)            # the value it has
    assert w.set_checksums(False)
    w.write(payload[:65536])                # a first frame
    assert not w.set_checksums(True)
    assert w.set_checksums(False)           # the value it has: true, nothing changes
    img = w.close()
    assert img[-5] == 0 and len(img) == int(zs.seek_table_of(np.frombuffer(img, np.uint8))[0][-1]) + 8 + 8 + 9
    # buffered bytes count as written too
    w = zs.Writer(LZ4, 65536)
    w.write(payload[:100])
    assert not w.set_checksums(True)
    assert w.close()[-5] == 0
    w = zs.Writer(ZSTD, 65536)
    w.write(payload[:100])
    assert not w.set_checksums(True)
    assert w.close()[-5] == 0
    assert zs.lib().zsk_writer_set_checksums(None, True) is False
    assert zs.lib().zsk_writer_set_checksums(None, False) is False


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import libzseek_amd.zseek as zs
out = []
for codec in (zs.ZSEEK_LZ4, zs.ZSEEK_ZSTD):
    w = zs.Writer(codec, 4096)
    w.write(bytes(range(256)) * 40)
    out.append(w.close()[-5])
print(out)
"""


@pytest.mark.parametrize("value,want", [("1", "[128, 128]"), ("0", "[0, 0]"), (None, "[0, 0]")])
def test_env_switch(zs, value, want):
    env = {k: v for k, v in os.environ.items() if k != "ZSEEK_WRITE_CHECKSUMS"}
    if value is not None:
        env["ZSEEK_WRITE_CHECKSUMS"] = value
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == want


@pytest.mark.parametrize("case", ["lz4_mixed", "zstd_oneshot", "zstd_workers"])
def test_reference_reader_reads_checksummed_files(zs, oracle, ref, payload, case):
    img = _write(zs, case, True, payload)
    assert img[-5] == 0x80
    r = ref.open(img, 1)
    try:
        assert r.h, r.error
        got, at = [], 0
        while at < len(payload):
            n, b = r.pread(100000, at)
            assert n > 0, r.error
            got.append(b)
            at += n
        assert b"".join(got) == payload
    finally:
        r.close()


def test_oracle_decodes_checksummed_files(zs, oracle, payload):
    img = _write(zs, "lz4_mixed", True, payload)
    assert oracle.decode_file(img) == payload
    st = oracle.seek_table(img)
    assert st["checksum_flag"]
    for case in ("zstd_oneshot", "zstd_workers"):
        img = _write(zs, case, True, payload)
        st = oracle.seek_table(img)
        assert st["checksum_flag"]
        parts = []
        for i in range(st["frames"]):
            c0, c1 = int(st["c_off"][i]), int(st["c_off"][i + 1])
            d0, d1 = int(st["d_off"][i]), int(st["d_off"][i + 1])
            data, err = oracle.zstd_decode(img[c0:c1], d1 - d0)
            assert err == 0, (case, i)
            assert oracle.xxh64(data) & 0xFFFFFFFF == int(st["checksum"][i])
            parts.append(data)
        assert b"".join(parts) == payload


def test_streaming_writer_stats_and_setting_rules(zs, payload):
    """The multi-worker path ends a frame lazily, at the next write: after two
    writes of 70,000 one frame is logged and one pending (+12)."""
    w = zs.Writer(ZSTD, 50000, nb_workers=2)
    assert w.set_checksums(True)
    w.write(payload[:70000])
    assert not w.set_checksums(False)       # bytes are in the stream
    w.write(payload[70000:140000])
    st = w.stats()
    assert st["frames"] == 2 and st["seek_table_size"] == 8 + 12 * 1 + 9 + 12
    img = w.close()
    assert img[-5] == 0x80 and int.from_bytes(img[-9:-5], "little") == 2
