"""The device API's pooled scratch (csrc/pool.h) under overlapping calls:
several streams with no host wait between their calls, and several threads.
tests/test_pool.py holds the pool's policy to a model on the CPU; here the
launchers that use it -- zsk_lz4_decode_frames(_ex), zsk_zstd_decode_frames
(_async), zsk_gather_segments without a prefix sum, zsk_lz4_build_image and
zsk_zstd_build_image -- must give the yardstick's bytes while their calls
overlap: a set handed to two calls at once, or reused before the stream that
last used it has passed, shows as wrong bytes under status 0.

Yardsticks, never the library: the bytes the inputs were made from (held to
oracle.decode_file, and to libzstd for the frames libzstd wrote), zstd_craft's
expand for its hand-built entries, lz4_craft's for its generated frames, and
numpy slicing for the gather.  Every output is 0xA5 with 64 guard bytes at both
ends and is compared whole; every status starts at -7777.

Overlap is forced with a gate: 0.25 s of matrix products on a gate stream, an
event recorded behind them, every worker stream waiting on that event.  A
call queued while the event is pending has all earlier calls' work still in
front of it.  Before that, `warm` makes four sets exist for the entry point
and grows each to the largest of the workload, so no call has to grow one (a
growing set waits for its stream, and so for the gate).

Every test and fixture takes `gpu` before `zs`, as all GPU tests here do: with
libzseek.so loaded before torch the library's HIP calls found no device
("no HIP device available") and every entry returned -1."""
from __future__ import annotations

import threading
import time

import numpy as np
import pytest

import lz4_craft
import zstd_caps_util as zu
import zstd_util

pytestmark = pytest.mark.gpu

SENT = 0xA5
UNSET = -7777
GUARD = 64
GATE = 0.25
KIB, MIB = 1 << 10, 1 << 20
ENTRIES = ["lz4", "zstd_async", "gather"]


# ---------------------------------------------------------------------------
# one call's buffers
# ---------------------------------------------------------------------------
class Decode:
    """frames back to back in device memory, decoded into a 0xA5 buffer with
    guards.  kind: lz4 (engine: a forced decoder or None), zstd_async (default
    bounds), zstd (the synchronous entry)."""

    def __init__(self, zs, gpu, kind, frames, dsizes, want, engine=None):
        import torch
        self.zs, self.kind, self.engine = zs, kind, engine
        n = len(frames)
        c = np.cumsum([0] + [len(f) for f in frames])
        d = GUARD + np.cumsum([0] + list(dsizes))
        desc = np.zeros(n, zs.FRAME_DESC_DTYPE)
        desc["c_off"], desc["d_off"] = c[:-1], d[:-1]
        desc["c_size"], desc["d_size"] = np.diff(c), np.asarray(dsizes)
        self.n, self.out_bytes = n, int(d[-1]) - GUARD
        assert len(want) == self.out_bytes
        self.want = np.full(int(d[-1]) + GUARD, SENT, np.uint8)
        self.want[GUARD: int(d[-1])] = np.frombuffer(want, np.uint8)
        self.td = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
        self.comp = torch.zeros(int(c[-1]) + 256, dtype=torch.uint8, device=gpu)
        self.comp[: int(c[-1])].copy_(torch.from_numpy(np.frombuffer(b"".join(frames), np.uint8).copy()))
        self.out = torch.full((self.want.size,), SENT, dtype=torch.uint8, device=gpu)
        self.status = torch.full((n,), UNSET, dtype=torch.int32, device=gpu)
        # (out_bytes: where the last frame ends in d_out, the guard in front included)
        self.bounds = zs.zstd_bounds_default(n, int(d[-1])) if kind == "zstd_async" else None

    def go(self, S):
        zs = self.zs
        if self.kind == "lz4":
            zs.decode_frames(self.td, self.comp, self.out, self.status, S.cuda_stream, self.engine)
        elif self.kind == "zstd_async":
            zs.zstd_decode_frames_async(self.td, self.comp, self.out, self.status, self.bounds, S.cuda_stream)
        else:
            zs.zstd_decode_frames(self.td, self.comp, self.out, self.status, S.cuda_stream)

    def reset(self):
        self.out.fill_(SENT)
        self.status.fill_(UNSET)

    def check(self, what=""):
        st = self.status.cpu().numpy()
        assert (st == 0).all(), (what, "status", np.nonzero(st)[0][:8], st[st != 0][:8])
        bad = np.nonzero(self.out.cpu().numpy() != self.want)[0]
        assert bad.size == 0, (what, "bytes", bad[:8], bad.size)

    def untouched(self) -> bool:
        return bool((self.status == UNSET).all().item()) and bool((self.out == SENT).all().item())


class Gather:
    """nseg segments of 1..80 bytes at every alignment, a gap after each, no
    prefix sum from the caller"""

    def __init__(self, zs, gpu, nseg, seed):
        import torch
        self.zs, self.n = zs, nseg
        rng = np.random.default_rng(seed)
        ln = rng.integers(1, 81, nseg)
        src_off = np.cumsum(ln + rng.integers(0, 5, nseg)) - ln
        dst_off = GUARD + np.cumsum(ln + rng.integers(1, 9, nseg)) - ln
        order = rng.permutation(nseg)                   # listed in another order than laid out
        seg = np.zeros(nseg, zs.SEGMENT_DTYPE)
        seg["src_off"], seg["dst_off"], seg["len"] = src_off[order], dst_off[order], ln[order]
        src = rng.integers(0, 256, int(src_off[-1] + ln[-1]) + 16, dtype=np.uint8)
        self.want = np.full(int(dst_off[-1] + ln[-1]) + GUARD, SENT, np.uint8)
        for so, do, k in zip(src_off, dst_off, ln):
            self.want[do: do + k] = src[so: so + k]
        self.seg = torch.from_numpy(seg.view(np.uint8).copy()).to(gpu)
        self.src = torch.from_numpy(src).to(gpu)
        self.out = torch.full((self.want.size,), SENT, dtype=torch.uint8, device=gpu)
        self.out_bytes = int(ln.sum())

    def go(self, S):
        self.zs.gather_segments(self.seg, self.src, self.out, None, S.cuda_stream)

    def reset(self):
        self.out.fill_(SENT)

    def check(self, what=""):
        bad = np.nonzero(self.out.cpu().numpy() != self.want)[0]
        assert bad.size == 0, (what, "bytes", bad[:8], bad.size)


# ---------------------------------------------------------------------------
# workloads: a different payload and shape for every stream
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth(gpu, zs):
    """the synthetic buffer past its first (random) 64 KiB"""
    return zs.synth_buffer(60 * MIB)[65536:]


@pytest.fixture(scope="module")
def zstd():
    z = zstd_util.load()
    assert z is not None, "libzstd 1.4.9 is the yardstick of the frames it writes"
    return z


def _lz4_spec(zs, oracle, data, frame_size, engine=None):
    """(frames, decoded sizes, the source bytes, engine): liblz4's seekable
    file of `data`, held to the oracle"""
    img = zs.lz4_seekable(np.ascontiguousarray(data), frame_size)
    assert oracle.decode_file(img.tobytes()) == data.tobytes()
    c_off, d_off = zs.seek_table_of(img)
    frames = [img[int(a): int(b)].tobytes() for a, b in zip(c_off[:-1], c_off[1:])]
    return frames, [int(x) for x in np.diff(d_off)], data.tobytes(), engine


@pytest.fixture(scope="module")
def lz4_specs(zs, oracle, synth):
    """per stream: ~300 frames of 4 KiB, ~200 of 64 KiB, 40 of 64 KiB (the
    one-frame route), 3 of 1 MiB through the block route (its jobs and origin
    scratch), lz4_craft's generated frames, and three more shapes"""
    at = [0]

    def take(n):
        at[0] += n + 4096
        return synth[at[0] - n - 4096: at[0] - 4096]

    specs = [_lz4_spec(zs, oracle, take(300 * 4 * KIB + 100), 4 * KIB),
             _lz4_spec(zs, oracle, take(200 * 64 * KIB), 64 * KIB),
             _lz4_spec(zs, oracle, take(40 * 64 * KIB - 7), 64 * KIB),
             _lz4_spec(zs, oracle, take(3 * MIB), MIB, "block")]
    gen = lz4_craft.random_valid(29, 257)
    for f, w in gen[:32]:
        st, got, _, _ = oracle.decode_frame(f, len(w))
        assert (st, got) == (0, w)
    specs.append(([f for f, _ in gen], [len(w) for _, w in gen], b"".join(w for _, w in gen), None))
    specs += [_lz4_spec(zs, oracle, take(65 * 64 * KIB + 3), 64 * KIB),
              _lz4_spec(zs, oracle, take(129 * 16 * KIB), 16 * KIB),
              _lz4_spec(zs, oracle, take(511 * 4 * KIB), 4 * KIB)]
    assert [len(s[0]) for s in specs] == [301, 200, 40, 3, 257, 66, 129, 511]
    return specs


@pytest.fixture(scope="module")
def zstd_specs(zs, oracle, synth, zstd, tmp_path_factory):
    """per stream, alternating: 150 of zstd_craft's accepted small entries (the
    lane route) and 40 libzstd level 3 frames of 4..64 KiB (the one-frame
    route); every batch within zsk_zstd_bounds_default by the plan walk on the
    CPU"""
    from test_gpu_zstd_async import SMALL, accepted, want_bytes
    caps = zu.load(tmp_path_factory.mktemp("pool_zstd_caps"))
    ok = []
    for c in SMALL:
        if accepted(c) and c[2] > 0:
            _, blocks, _, seqs = zu.plan(caps, c[1])
            if blocks <= 2 and seqs <= c[2] // 3:        # the default bounds, entry by entry
                ok.append(c)
    assert len(ok) >= 100, len(ok)
    specs = []
    for k in range(4):
        rng = np.random.default_rng(100 + k)
        part = [ok[i] for i in rng.integers(0, len(ok), 150 + k)]
        specs.append(([c[1] for c in part], [c[2] for c in part], b"".join(want_bytes(c) for c in part), None))
        sizes = rng.integers(4 * KIB, 64 * KIB + 1, 40 - k)
        at = 20 * MIB + k * 3 * MIB
        frames, want = [], []
        for n in sizes:
            piece = synth[at: at + int(n)].tobytes()
            at += int(n)
            f = zstd_util.compress(zstd, piece, {zstd_util.P_LEVEL: 3})
            assert zstd_util.decode(zstd, f, len(piece)) == (piece, 0)
            frames.append(f)
            want.append(piece)
        specs.append((frames, [int(n) for n in sizes], b"".join(want), None))
    for frames, dsizes, _, _ in specs:
        mb, ms = zu.defaults(caps, len(frames), sum(dsizes))
        assert zu.fits(caps, frames, sum(dsizes), mb, ms)
    return specs


GATHER_SEGS = [1, 4095, 4096, 4097, 2, 4094, 4098, 700]     # either side of the 4,096-entry least allocation


def make_jobs(request, zs, gpu, entry, copies=0):
    """the entry's eight jobs (copies: that many of one payload instead)"""
    if entry == "gather":
        if copies:
            return [Gather(zs, gpu, GATHER_SEGS[3], 50) for _ in range(copies)]
        return [Gather(zs, gpu, n, 50 + i) for i, n in enumerate(GATHER_SEGS)]
    specs = request.getfixturevalue("lz4_specs" if entry == "lz4" else "zstd_specs")
    kind = "zstd" if entry == "zstd_sync" else entry
    return [Decode(zs, gpu, kind, *s) for s in (specs[:1] * copies if copies else specs)]


# ---------------------------------------------------------------------------
# the gate, the streams, the warm-up
# ---------------------------------------------------------------------------
class Rig:
    def __init__(self, gpu):
        import torch
        from test_gpu_preadv_async import _busy_work
        self.gpu = gpu
        self.G = torch.cuda.Stream(device=gpu)
        self.S = [torch.cuda.Stream(device=gpu) for _ in range(14)]     # workers
        self.T = [torch.cuda.Stream(device=gpu) for _ in range(4)]      # the warm-up's
        self.queue = _busy_work(gpu, self.G, GATE)
        self.kept = {}

    def gate(self, streams):
        """the gate's work queued, its event recorded, `streams` waiting on it"""
        import torch
        ev = torch.cuda.Event()
        self.queue()
        ev.record(self.G)
        for s in streams:
            s.wait_event(ev)
        return ev

    def drain(self):
        import torch
        torch.cuda.synchronize()

    def jobs(self, request, zs, entry):
        """-> (the entry's eight jobs, six more of one payload), made once and
        warmed: the LZ4 launcher sizes its scratch by where a batch's
        compressed bytes lie in their allocation, so the buffers the warm-up
        saw are the ones the gated rounds use."""
        if entry not in self.kept:
            main = make_jobs(request, zs, self.gpu, entry)
            same = make_jobs(request, zs, self.gpu, entry, copies=6)
            self.warm(main + same)
            self.kept[entry] = (main, same)
        main, same = self.kept[entry]
        for j in main + same:
            j.reset()
        self.drain()
        return main, same

    def warm(self, jobs):
        """Four sets of the jobs' pool, each last released on one of T and
        grown to the largest job.  A pass pins them: a call on T[k], then
        T[k] behind the gate and the call again (its set is now pending, so
        T[k + 1] cannot take it); then every job on every T[k], which takes
        its own set (same stream).  A set that had to grow from an earlier
        test's smaller size frees memory, which waits for the device and so
        for the gate: such a pass pins fewer sets, and one more pass follows."""
        pinned = False
        for _ in range(5):
            ev = self.gate([])
            for t in self.T:
                jobs[0].go(t)
                t.wait_event(ev)
                jobs[0].go(t)
            pinned = not ev.query()
            self.drain()
            for t in self.T:
                for j in jobs:
                    j.go(t)
            self.drain()
            if pinned:
                break
        assert pinned, "the warm-up never pinned four sets while its gate was pending"
        for j in jobs:
            j.check("warm-up")


@pytest.fixture(scope="module")
def rig(gpu):
    return Rig(gpu)


# ---------------------------------------------------------------------------
# growth behind queued work (first: the sets are still small)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_growth_behind_queued_work(gpu, zs, request, rig, oracle, synth, entry):
    """A small batch, then one at least 8 times larger that the set has to
    grow for, on the same stream and then on another, each behind the gate's
    work: growing waits for the stream before it frees what queued kernels
    use.  (Run behind other modules the pools may already hold sets this
    large; the calls are then only held to their bytes.)"""
    if entry == "gather":
        small = [Gather(zs, gpu, 1, 90 + i) for i in range(2)]
        large = [Gather(zs, gpu, 40000, 92 + i) for i in range(2)]
    elif entry == "lz4":
        s = _lz4_spec(zs, oracle, synth[33 * MIB: 33 * MIB + 64 * 4 * KIB], 4 * KIB)
        b = _lz4_spec(zs, oracle, synth[34 * MIB: 34 * MIB + 4200 * 4 * KIB], 4 * KIB)
        small = [Decode(zs, gpu, "lz4", *s) for _ in range(2)]
        large = [Decode(zs, gpu, "lz4", *b) for _ in range(2)]
    else:
        specs = request.getfixturevalue("zstd_specs")
        tiny = (specs[1][0][:8], specs[1][1][:8], specs[1][2][: sum(specs[1][1][:8])], None)
        frames = specs[1][0] + specs[3][0] + specs[5][0] + specs[7][0]
        big = (frames, specs[1][1] + specs[3][1] + specs[5][1] + specs[7][1],
               specs[1][2] + specs[3][2] + specs[5][2] + specs[7][2], None)
        small = [Decode(zs, gpu, "zstd_async", *tiny) for _ in range(2)]
        large = [Decode(zs, gpu, "zstd_async", *big) for _ in range(2)]
    assert large[0].out_bytes >= 8 * small[0].out_bytes and large[0].n >= 8 * small[0].n
    rig.drain()
    A, B = rig.S[12], rig.S[13]
    rig.gate([A])
    small[0].go(A)
    large[0].go(A)                  # same stream: the set of the call before, still queued
    rig.gate([B])
    small[1].go(A)
    large[1].go(B)                  # another stream, while A's calls are queued
    rig.drain()
    for i, j in enumerate(small + large):
        j.check(i)


# ---------------------------------------------------------------------------
# fan-out
# ---------------------------------------------------------------------------
QUEUE_TIMES = {}


@pytest.mark.parametrize("K", [2, 4, 5, 8])
@pytest.mark.parametrize("entry", ENTRIES)
def test_fan_out(gpu, zs, request, rig, entry, K):
    """K streams behind the gate, one call each, no host wait in between; two
    rounds, the second asserted: the gate's event is still pending after the
    last call was queued, so the K calls' work is all in front of the device
    at once.  With K > 4 the calls past the fourth take the least recently
    released set behind a stream wait; every output is the yardstick's.

    Host time to queue the K = 8 round, measured on the MI355X (and printed
    by every run): 0.26 ms for LZ4, 0.37 ms for zstd, 0.10 ms for the gather;
    the 0.25 s gate is over 600 times that."""
    jobs, streams = rig.jobs(request, zs, entry)[0][:K], rig.S[:K]
    for rnd in (1, 2):
        ev = rig.gate(streams)
        t0 = time.perf_counter()
        for j, s in zip(jobs, streams):
            j.go(s)
        dt = time.perf_counter() - t0
        pending = not ev.query()
        rig.drain()
        print(f"{entry} K = {K} round {rnd}: queued in {dt * 1e3:.3f} ms, gate pending: {pending}")
        if rnd == 2:
            QUEUE_TIMES[(entry, K)] = dt
            assert pending, f"a call waited for its stream: the K = {K} calls did not overlap"
            assert GATE >= 4 * dt, f"queuing took {dt * 1e3:.1f} ms: the gate is not 4 times that"
        for i, j in enumerate(jobs):
            j.check((rnd, i))
            j.reset()
        rig.drain()


# ---------------------------------------------------------------------------
# ping-pong
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_ping_pong(gpu, zs, request, rig, entry):
    """One batch on streams A, B, A, B, A, B (an output per call).  With a host
    wait between the calls every call finds a completed set.  Behind the gate,
    with five other streams' calls queued first, every set is pending on some
    other stream and each call waits on the least recently released one."""
    main, jobs = rig.jobs(request, zs, entry)
    A, B = rig.S[12], rig.S[13]
    for i, j in enumerate(jobs):
        j.go(B if i % 2 else A)
        rig.drain()
    for i, j in enumerate(jobs):
        j.check(("host waits", i))
        j.reset()
    rig.drain()
    others = main[1:6]
    ev = rig.gate(rig.S[:5] + [A, B])
    for j, s in zip(others, rig.S[:5]):
        j.go(s)
    for i, j in enumerate(jobs):
        j.go(B if i % 2 else A)
    pending = not ev.query()
    rig.drain()
    assert pending, "a call waited for its stream: nothing overlapped"
    for i, j in enumerate(others + jobs):
        j.check(("gated", i))


# ---------------------------------------------------------------------------
# threads
# ---------------------------------------------------------------------------
def _run_threads(bodies):
    errors = []

    def wrap(f, i):
        try:
            f(i)
        except BaseException as e:      # noqa: BLE001 (reported below, in the main thread)
            errors.append((i, repr(e)))

    th = [threading.Thread(target=wrap, args=(f, i)) for i, f in enumerate(bodies)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:4]


def test_threads_decode(gpu, zs, request, rig):
    """4 threads, a stream each, 20 calls each of zsk_lz4_decode_frames and of
    the synchronous zsk_zstd_decode_frames: four calls in progress at most, so
    every one of the 160 gets a set, returns 0 and is exact."""
    import torch
    lz = make_jobs(request, zs, gpu, "lz4")
    zd = make_jobs(request, zs, gpu, "zstd_sync")
    pairs = [(lz[0], zd[0]), (lz[2], zd[1]), (lz[4], zd[2]), (lz[6], zd[3])]
    rig.drain()
    calls = [0] * 4

    def body(i):
        S = rig.S[i]
        with torch.cuda.stream(S):
            for r in range(20):
                for j in pairs[i]:
                    j.reset()
                    j.go(S)
                    calls[i] += 1
                S.synchronize()
                for j in pairs[i]:
                    j.check((i, r))

    _run_threads([body] * 4)
    assert sum(calls) == 160


def _zstd_file(oracle, zstd, file: bytes) -> bytes:
    """every frame of a seekable zstd file through libzstd"""
    st = oracle.seek_table(file)
    assert st is not None
    parts = []
    for i in range(st["frames"]):
        n = int(st["d_off"][i + 1] - st["d_off"][i])
        got, err = zstd_util.decode(zstd, file[int(st["c_off"][i]): int(st["c_off"][i + 1])], n)
        assert err == 0 and len(got) == n, (i, err)
        parts.append(got)
    return b"".join(parts)


def test_threads_build_images(gpu, zs, rig, oracle, zstd, synth):
    """4 threads, each building its own LZ4 image and its own zstd image:
    every image decodes to its source (the oracle, libzstd) and is byte for
    byte the image of the same build made alone."""
    import torch
    shapes = [(300 * KIB + 11, 4 * KIB), (2 * MIB + 5, 64 * KIB), (MIB + 1, 16 * KIB), (3 * MIB, MIB)]
    srcs = [synth[(52 + i) * MIB: (52 + i) * MIB + n] for i, (n, _) in enumerate(shapes)]
    dev = [torch.from_numpy(np.ascontiguousarray(s)).to(gpu) for s in srcs]
    rig.drain()
    alone = [(bytes(zs.lz4_build_image(d, fs).cpu().numpy()),
              bytes(zs.zstd_build_image(d, fs).cpu().numpy())) for d, (_, fs) in zip(dev, shapes)]
    for (a, b), s in zip(alone, srcs):
        assert oracle.decode_file(a) == s.tobytes() and _zstd_file(oracle, zstd, b) == s.tobytes()
    got = [[] for _ in shapes]

    def body(i):
        fs = shapes[i][1]
        for _ in range(3):
            got[i].append((bytes(zs.lz4_build_image(dev[i], fs).cpu().numpy()),
                           bytes(zs.zstd_build_image(dev[i], fs).cpu().numpy())))

    _run_threads([body] * 4)
    for i, rounds in enumerate(got):
        assert len(rounds) == 3
        for pair in rounds:
            assert pair == alone[i], i


def test_threads_lz4_eight(gpu, zs, request, rig):
    """8 threads: more calls in progress than sets.  A call returns 0 and is
    exact, or fails before anything was queued: the wrapper raises, the status
    array is still unset and the output all 0xA5."""
    import torch
    jobs = make_jobs(request, zs, gpu, "lz4")
    for j in jobs:                  # alone, every call gets a set
        j.go(rig.S[0])
    rig.drain()
    for i, j in enumerate(jobs):
        j.check(("alone", i))
    refused = [0] * 8

    def body(i):
        S, j = rig.S[i], jobs[i]
        with torch.cuda.stream(S):
            for r in range(20):
                j.reset()
                S.synchronize()
                try:
                    j.go(S)
                except zs.ZseekError:
                    S.synchronize()
                    assert j.untouched(), (i, r, "a refused call wrote")
                    refused[i] += 1
                    continue
                S.synchronize()
                j.check((i, r))

    _run_threads([body] * 8)
    print("refused calls per thread:", refused)
    assert sum(refused) < 8 * 20
