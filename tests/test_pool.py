"""The device API's scratch pool on the CPU: libzseek_amd/csrc/pool.h -- the
text the launchers compile -- through tests/native/pool_shim.cpp, which
defines the six HIP calls the pool makes as fakes (streams with a queued and a
completed count, events that note where they were recorded, a log of stream
waits, a sticky last error).

The yardstick is the model below, written from pool.h's header comment and not
from its code.  A set released on stream R is free for R at once (stream
order), for any stream once R has passed the release, and for another stream
before that only behind a wait on the event of that release.  The pool tries,
in this order: a set last released on the acquiring stream; a set whose event
has completed; a new set while the device has fewer than four; the least
recently released set behind a wait; and gives nullptr when every set is held.

Every acquire in this file goes through Sim.acquire, which checks the returned
set against the model: safety, exclusivity, the branch taken, and that the
fake's last error is success."""
from __future__ import annotations

import ctypes as C
import os
import pathlib
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SETS = 4               # kPoolSets
STREAMS = 8
SAME, DONE, NEW, WAIT = 1, 2, 3, 4


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("pool") / "libpool.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-pthread",
                    "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", "-o", str(so),
                    str(ROOT / "tests/native/pool_shim.cpp")], check=True)
    L = C.CDLL(str(so))
    L.pool_new.restype = C.c_void_p
    L.pool_acquire.restype = C.c_int
    L.pool_acquire.argtypes = [C.c_void_p, C.c_int]
    L.pool_release.restype = None
    L.pool_release.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pool_threads.restype = None
    L.pool_threads.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.fake_work.restype = C.c_uint64
    L.fake_work.argtypes = [C.c_int]
    L.fake_set_done.restype = None
    L.fake_set_done.argtypes = [C.c_int, C.c_uint64]
    L.fake_queued.restype = C.c_uint64
    L.fake_queued.argtypes = [C.c_int]
    L.fake_fail.restype = None
    L.fake_fail.argtypes = [C.c_int, C.c_int]
    L.fake_counts.argtypes = [C.c_void_p]
    L.fake_wait_at.argtypes = [C.c_uint64, C.c_void_p]
    L.fake_record_at.argtypes = [C.c_uint64, C.c_void_p]
    return L


class Set:
    def __init__(self, ident, dev):
        self.id, self.dev = ident, dev
        self.busy = True
        self.rel = None        # (stream, position) of the last release
        self.order = 0         # releases are numbered: the least is the least recent
        self.event = None      # the fake's number of the event its releases record


class Sim:
    """The pool under test, the fake, and the model of both."""

    def __init__(self, L):
        self.L = L
        L.fake_reset()
        self.pool = L.pool_new()
        self.dev = 0
        self.queue = {s: [] for s in range(STREAMS)}    # per item: None (work) or the (stream, position) waited for
        self.done = {s: 0 for s in range(STREAMS)}
        self.sets = {}                                  # id -> Set
        self.releases = 0
        self.taken = {SAME: 0, DONE: 0, NEW: 0, WAIT: 0, None: 0}

    # ---- the fake's side
    def counts(self):
        out = (C.c_uint64 * 4)()
        self.L.fake_counts(out)
        return dict(zip(("events", "queries", "waits", "records"), out))

    def wait_at(self, i):
        out = (C.c_int64 * 5)()
        self.L.fake_wait_at(i, out)
        return dict(zip(("stream", "at", "event", "ev_stream", "ev_pos"), out))

    def record_at(self, i):
        out = (C.c_int64 * 3)()
        self.L.fake_record_at(i, out)
        return dict(zip(("event", "stream", "pos"), out))

    def device(self, d):
        self.dev = d
        self.L.fake_set_device(d)

    def work(self, stream, n=1):
        for _ in range(n):
            at = self.L.fake_work(stream)
            self.queue[stream].append(None)
            assert at == len(self.queue[stream])

    def advance(self, stream, n=None):
        """The stream completes up to n of its items (None: all it can): it
        stops in front of a wait for an event that has not completed."""
        moved = 0
        while self.done[stream] < len(self.queue[stream]) and (n is None or moved < n):
            item = self.queue[stream][self.done[stream]]
            if item is not None and self.done[item[0]] < item[1]:
                break
            self.done[stream] += 1
            moved += 1
        self.L.fake_set_done(stream, self.done[stream])
        return moved

    def drain(self):
        while sum(self.advance(s) for s in range(STREAMS)):
            pass

    # ---- the model
    def here(self):
        return [x for x in self.sets.values() if x.dev == self.dev]

    def complete(self, x):
        return x.rel is None or self.done[x.rel[0]] >= x.rel[1]

    def expected(self, stream):
        free = [x for x in self.here() if not x.busy]
        if any(x.rel[0] == stream for x in free):
            return SAME
        if any(self.complete(x) for x in free):
            return DONE
        if len(self.here()) < SETS:
            return NEW
        return WAIT if free else None

    # ---- the pool
    def acquire(self, stream, fail=None):
        """-> the set's id or None.  fail: "create" / "wait" makes that HIP
        call fail once; the acquire must then return nullptr and change
        nothing."""
        want = self.expected(stream)
        if fail:
            assert want == (NEW if fail == "create" else WAIT), "the failure would not be met"
            self.L.fake_fail(fail == "create", fail == "wait")
        before = self.counts()
        free = [x for x in self.here() if not x.busy]
        got = self.L.pool_acquire(self.pool, stream)
        after = self.counts()
        self.L.fake_fail(0, 0)
        assert self.L.fake_last_error() == 0, "acquire left an error for the launcher's hipGetLastError"
        assert after["records"] == before["records"]
        if fail or want is None:
            assert got == -1
            assert (after["events"], after["waits"]) == (before["events"], before["waits"])
            self.taken[None] += 1
            return None
        assert got >= 0, f"nullptr where branch {want} applies"
        if got not in self.sets:
            took = NEW
            assert after["events"] == before["events"] + 1
            x = self.sets[got] = Set(got, self.dev)
            x.busy = False
        else:
            x = self.sets[got]
            assert x.dev == self.dev, "a set of another device"
            assert not x.busy, "a set handed out twice"
            assert after["events"] == before["events"]
            took = WAIT if after["waits"] > before["waits"] else SAME if x.rel[0] == stream else DONE
        # safety
        waited = None
        if after["waits"] > before["waits"]:
            assert after["waits"] == before["waits"] + 1
            waited = self.wait_at(before["waits"])
            assert waited["stream"] == stream
            self.queue[stream].append((waited["ev_stream"], waited["ev_pos"]))
            assert waited["at"] == len(self.queue[stream])
        safe = x.rel is None or x.rel[0] == stream or self.complete(x) or \
            (waited is not None and waited["event"] == x.event and (waited["ev_stream"], waited["ev_pos"]) == x.rel)
        assert safe, f"set {got} handed to stream {stream} while stream {x.rel[0]} may still use it"
        # preference
        assert took == want, f"branch {took} taken where {want} is the first that applies"
        if took != WAIT:
            assert waited is None, "a wait where none is needed"
        else:
            assert x.order == min(y.order for y in free), "not the least recently released set"
        # exclusivity
        x.busy = True
        assert len(self.here()) <= SETS
        self.taken[took] += 1
        return got

    def release(self, ident, stream):
        x = self.sets[ident]
        assert x.busy and x.dev == self.dev
        before = self.counts()
        self.L.pool_release(self.pool, ident, stream)
        after = self.counts()
        assert after["records"] == before["records"] + 1, "release recorded no event"
        r = self.record_at(before["records"])
        assert (r["stream"], r["pos"]) == (stream, len(self.queue[stream]))
        assert x.event in (None, r["event"]), "a set's event changed"
        x.event = r["event"]
        x.rel = (stream, len(self.queue[stream]))
        self.releases += 1
        x.order = self.releases
        x.busy = False

    def call(self, stream, work=1):
        """What a launcher does: acquire, queue its kernels, release."""
        got = self.acquire(stream)
        if got is not None:
            self.work(stream, work)
            self.release(got, stream)
        return got


def four_pending(sim):
    """sets 0..3 released on streams 1..4, in that order, none complete"""
    for s in (1, 2, 3, 4):
        assert sim.call(s) == s - 1
    assert sim.taken[NEW] == 4


# ---------------------------------------------------------------------------
# one case per branch
# ---------------------------------------------------------------------------
def test_same_stream_takes_its_set_without_a_wait(shim):
    sim = Sim(shim)
    assert sim.call(1) == 0
    assert sim.call(1) == 0 and sim.call(1) == 0
    assert sim.taken == {SAME: 2, DONE: 0, NEW: 1, WAIT: 0, None: 0}
    assert sim.counts()["waits"] == 0 and sim.counts()["events"] == 1
    # ... also where another stream's completed set is there to take
    assert sim.call(2) == 1
    sim.drain()
    assert sim.call(2) == 1 and sim.call(1) == 0
    assert sim.taken[SAME] == 4


def test_completed_event_frees_the_set_for_any_stream(shim):
    sim = Sim(shim)
    assert sim.call(1) == 0
    sim.advance(1)
    assert sim.call(2, work=3) == 0  # not a new set
    assert sim.taken[DONE] == 1 and sim.counts()["events"] == 1
    # one item short of the release is not complete
    sim.advance(2, 2)
    assert sim.call(3) == 1 and sim.taken[NEW] == 2
    sim.advance(2, 1)
    assert sim.call(4) == 0 and sim.taken[DONE] == 2
    assert sim.counts()["waits"] == 0


def test_new_sets_up_to_four(shim):
    sim = Sim(shim)
    four_pending(sim)
    assert sim.counts() == {"events": 4, "queries": sim.counts()["queries"], "waits": 0, "records": 4}


def test_least_recent_set_behind_a_wait(shim):
    sim = Sim(shim)
    four_pending(sim)
    assert sim.call(5) == 0
    w = sim.wait_at(0)
    assert (w["stream"], w["ev_stream"], w["ev_pos"]) == (5, 1, 1)
    assert sim.call(6) == 1 and sim.call(7) == 2
    assert sim.call(1) == 3          # stream 1's own set went to stream 5
    assert sim.call(5) == 0          # its own now: no wait
    assert sim.taken == {SAME: 1, DONE: 0, NEW: 4, WAIT: 4, None: 0}
    assert sim.counts()["events"] == 4
    # the waiting streams run once the streams they wait for have
    sim.advance(5)
    assert sim.done[5] == 0
    sim.advance(1)
    assert sim.done[1] == 1          # (its second item waits for stream 4)
    sim.drain()
    assert all(sim.done[s] == len(sim.queue[s]) for s in range(STREAMS))


# ---------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------
def test_never_recorded_event_does_not_free_a_held_set(shim):
    """A held set's event was never recorded and reads as complete, and its
    last stream is still the null handle: neither makes it free."""
    sim = Sim(shim)
    a = sim.acquire(3)
    assert sim.acquire(5) == 1       # (a query of set 0's event would return success)
    assert sim.acquire(0) == 2       # the null stream is not set 0's "same stream"
    assert sim.acquire(3) == 3
    assert sim.acquire(3) is None
    sim.work(3)
    sim.release(a, 3)
    assert sim.acquire(0) == a and sim.taken[WAIT] == 1


def test_null_stream_is_a_stream(shim):
    sim = Sim(shim)
    assert sim.call(0) == 0 and sim.call(0) == 0
    assert sim.call(1) == 1          # pending on the null stream: not taken
    assert sim.call(2) == 2 and sim.call(3) == 3
    assert sim.call(4) == 0          # behind a wait on the null stream's event
    w = sim.wait_at(0)
    assert (w["stream"], w["ev_stream"], w["ev_pos"]) == (4, 0, 2)
    assert sim.call(0) == 1
    assert (sim.wait_at(1)["stream"], sim.wait_at(1)["ev_stream"]) == (0, 1)
    sim.drain()
    assert sim.call(0) == 1 and sim.taken[SAME] == 2


def test_devices_keep_separate_sets(shim):
    sim = Sim(shim)
    four_pending(sim)
    sim.device(1)
    assert [sim.call(s) for s in (1, 2, 3, 4)] == [4, 5, 6, 7]      # same handles, other device: new sets
    assert sim.call(5) == 4
    sim.device(0)
    assert sim.call(5) == 0 and sim.call(1) == 1
    sim.drain()
    sim.device(1)
    assert sim.call(7) in (4, 5, 6, 7)
    assert sim.counts()["events"] == 8


def test_event_creation_failure(shim):
    sim = Sim(shim)
    assert sim.acquire(1, fail="create") is None
    assert sim.here() == []
    assert sim.call(1) == 0 and sim.call(2) == 1
    assert sim.acquire(3, fail="create") is None
    assert len(sim.here()) == 2
    assert [sim.call(s) for s in (3, 4)] == [2, 3]      # the count was unchanged: two more fit
    assert sim.call(5) == 0 and sim.counts()["events"] == 4


def test_stream_wait_failure_leaves_the_set_free(shim):
    sim = Sim(shim)
    four_pending(sim)
    assert sim.acquire(5, fail="wait") is None
    assert sim.counts()["waits"] == 0
    got = [sim.acquire(5), sim.acquire(5), sim.acquire(6), sim.acquire(7)]
    assert got == [0, 1, 2, 3]       # none was left busy; the least recent first again
    assert sim.acquire(5) is None


def test_all_four_held(shim):
    sim = Sim(shim)
    held = [sim.acquire(s) for s in (1, 2, 3, 1)]
    assert held == [0, 1, 2, 3]
    for s in (1, 5, 0):
        assert sim.acquire(s) is None
    assert sim.counts()["events"] == 4 and sim.counts()["waits"] == 0
    sim.work(2)
    sim.release(1, 2)
    assert sim.acquire(5) == 1 and sim.taken[WAIT] == 1
    assert sim.acquire(2) is None


def test_lru_is_by_release_not_by_acquire(shim):
    sim = Sim(shim)
    held = [sim.acquire(s) for s in (1, 2, 3, 4)]
    assert held == [0, 1, 2, 3]
    for ident in (2, 0, 3, 1):
        sim.work(ident + 1)
        sim.release(ident, ident + 1)
    assert [sim.acquire(s) for s in (5, 6, 7, 5)] == [2, 0, 3, 1]
    assert sim.taken[WAIT] == 4
    # the order follows later releases too
    for ident in (3, 2):
        sim.work(5)
        sim.release(ident, 5)
    assert sim.acquire(6) == 3 and sim.acquire(7) == 2


# ---------------------------------------------------------------------------
# seeded random walks
# ---------------------------------------------------------------------------
def walk(shim, rng, ops, taken):
    """One pool, `ops` operations; -> the failures injected."""
    sim = Sim(shim)
    held = []                        # (set, stream, device)
    injected = 0
    for _ in range(ops):
        op = rng.random()
        if op < 0.30:
            stream = int(rng.integers(0, STREAMS))
            want, fail = sim.expected(stream), None
            if rng.random() < 0.05 and want in (NEW, WAIT):
                fail = "create" if want == NEW else "wait"
                injected += 1
            got = sim.acquire(stream, fail)
            if got is not None:
                held.append((got, stream, sim.dev))
        elif op < 0.60:
            if held:
                ident, stream, dev = held.pop(int(rng.integers(0, len(held))))
                keep = sim.dev
                sim.device(dev)      # (a call runs on one device from start to end)
                sim.work(stream, int(rng.integers(0, 3)))
                sim.release(ident, stream)
                sim.device(keep)
        elif op < 0.95:
            sim.advance(int(rng.integers(0, STREAMS)), None if rng.random() < 0.7 else int(rng.integers(1, 4)))
        else:
            sim.device(int(rng.integers(0, 2)))
        for s in range(STREAMS):
            assert shim.fake_queued(s) == len(sim.queue[s])
    assert len(sim.sets) <= 2 * SETS
    for ident, stream, dev in held:
        sim.device(dev)
        sim.release(ident, stream)
    sim.drain()
    assert all(sim.done[s] == len(sim.queue[s]) for s in range(STREAMS)), "the waits left a stream stuck"
    for b, n in sim.taken.items():
        taken[b] += n
    return injected


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_walk(shim, seed):
    """12,000 operations over 8 streams and 2 devices, 3,000 to a pool (a pool
    makes at most 8 new sets): acquire (now and then with a failing HIP
    call), release, advance a stream, switch device.  Sets are held across
    other operations, so acquires overlap."""
    rng = np.random.default_rng(seed)
    taken = {SAME: 0, DONE: 0, NEW: 0, WAIT: 0, None: 0}
    injected = sum(walk(shim, rng, 3000, taken) for _ in range(4))
    print(seed, taken, "injected failures", injected)
    assert all(taken[b] >= 20 for b in taken), taken
    assert injected >= 20


# ---------------------------------------------------------------------------
# threads
# ---------------------------------------------------------------------------
def test_threads_never_share_a_set(shim):
    """8 C++ threads, each with its own stream, 5,000 rounds of acquire / hold
    / release: an owner word in every set counts double hand-outs."""
    shim.fake_reset()
    out = (C.c_uint64 * 4)()
    shim.pool_threads(shim.pool_new(), 8, 5000, out)
    doubles, nulls, most, sets = out
    print(f"double hand-outs {doubles}, nullptr {nulls} of 40000, most holders {most}, sets {sets}")
    assert doubles == 0
    assert most <= SETS and sets <= SETS
