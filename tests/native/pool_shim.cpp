// pool_shim.cpp -- libzseek_amd/csrc/pool.h (host-only code) over a fake of
// the six HIP calls it makes, for tests/test_pool.py.  No HIP library is
// linked: the fakes below are the definitions the header's declarations find.
//
// The fake: a stream is a small integer (0 is the legacy null stream, a stream
// like any other) with two counters, the items queued on it and the items it
// has completed.  fake_work queues one item; hipStreamWaitEvent queues one
// too, and logs (stream, position, event, the event's stream and position).
// hipEventRecord notes the stream and its queued count: the event has
// completed once that stream has completed as many items; an event never
// recorded reads as complete, as HIP's does.  hipEventQuery on a pending event
// returns hipErrorNotReady and leaves it as the sticky last error, which
// hipGetLastError returns and clears.  The test moves a stream's completed
// count (fake_set_done) and keeps its own model of what that allows.
//
// With -DPOOL_SHIM_MAIN the file is a program: the thread entry under a
// thread sanitizer.
#include "../../libzseek_amd/csrc/pool.h"

#include <atomic>
#include <thread>

namespace {

constexpr int kStreams = 16;

struct FakeEvent {
    int id = 0;
    bool recorded = false;
    int stream = 0;
    uint64_t pos = 0;
};

struct Fake {
    std::mutex mu;
    uint64_t queued[kStreams] = {};
    uint64_t done[kStreams] = {};
    std::vector<FakeEvent *> events;
    std::vector<int64_t> waits;     // 5 per wait: stream, its position, event, the event's stream and position
    std::vector<int64_t> records;   // 3 per record: event, stream, position
    uint64_t queries = 0;
    hipError_t last = hipSuccess;
    int fail_create = 0, fail_wait = 0;
};

Fake *F = new Fake();
std::atomic<int> g_device{0};

int sid(hipStream_t s)
{
    return (int)(uintptr_t)s;
}

struct Scratch {
    std::atomic<int> owner{0};
    int id = -1;
};

struct Pool {
    zsk::ScratchPool<Scratch> pool;
    std::mutex mu;
    std::vector<Scratch *> sets;   // by id
};

}   // namespace

// ---- the six HIP calls ---------------------------------------------------------
extern "C" hipError_t hipGetDevice(int *d)
{
    *d = g_device.load();
    return hipSuccess;
}

extern "C" hipError_t hipGetLastError(void)
{
    std::lock_guard<std::mutex> g(F->mu);
    const hipError_t e = F->last;
    F->last = hipSuccess;
    return e;
}

extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    std::lock_guard<std::mutex> g(F->mu);
    if (F->fail_create > 0) {
        F->fail_create--;
        return hipErrorOutOfMemory;
    }
    FakeEvent *x = new FakeEvent();
    x->id = (int)F->events.size();
    F->events.push_back(x);
    *e = reinterpret_cast<hipEvent_t>(x);
    return hipSuccess;
}

extern "C" hipError_t hipEventQuery(hipEvent_t e)
{
    std::lock_guard<std::mutex> g(F->mu);
    const FakeEvent *x = reinterpret_cast<const FakeEvent *>(e);
    F->queries++;
    if (!x->recorded || F->done[x->stream] >= x->pos)
        return hipSuccess;
    F->last = hipErrorNotReady;
    return hipErrorNotReady;
}

extern "C" hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    std::lock_guard<std::mutex> g(F->mu);
    FakeEvent *x = reinterpret_cast<FakeEvent *>(e);
    x->recorded = true;
    x->stream = sid(s);
    x->pos = F->queued[sid(s)];
    F->records.insert(F->records.end(), {x->id, x->stream, (int64_t)x->pos});
    return hipSuccess;
}

extern "C" hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned)
{
    std::lock_guard<std::mutex> g(F->mu);
    if (F->fail_wait > 0) {
        F->fail_wait--;
        return hipErrorInvalidHandle;
    }
    const FakeEvent *x = reinterpret_cast<const FakeEvent *>(e);
    const int64_t at = (int64_t)++F->queued[sid(s)];
    F->waits.insert(F->waits.end(),
                    {sid(s), at, x->id, x->recorded ? x->stream : -1, x->recorded ? (int64_t)x->pos : 0});
    return hipSuccess;
}

// ---- the test's side of the fake -----------------------------------------------
extern "C" void fake_reset(void)
{
    F = new Fake();   // (the old one stays behind: a pool of an earlier test may still name its events)
    g_device = 0;
}

extern "C" void fake_set_device(int d)
{
    g_device = d;
}

extern "C" uint64_t fake_work(int stream)
{
    std::lock_guard<std::mutex> g(F->mu);
    return ++F->queued[stream];
}

extern "C" void fake_set_done(int stream, uint64_t pos)
{
    std::lock_guard<std::mutex> g(F->mu);
    F->done[stream] = pos < F->queued[stream] ? pos : F->queued[stream];
}

extern "C" uint64_t fake_queued(int stream)
{
    std::lock_guard<std::mutex> g(F->mu);
    return F->queued[stream];
}

extern "C" int fake_last_error(void)   // (not cleared)
{
    std::lock_guard<std::mutex> g(F->mu);
    return (int)F->last;
}

extern "C" void fake_fail(int creates, int waits)
{
    std::lock_guard<std::mutex> g(F->mu);
    F->fail_create = creates;
    F->fail_wait = waits;
}

// counts: events created, queries, waits logged, records logged
extern "C" void fake_counts(uint64_t *out)
{
    std::lock_guard<std::mutex> g(F->mu);
    out[0] = F->events.size();
    out[1] = F->queries;
    out[2] = F->waits.size() / 5;
    out[3] = F->records.size() / 3;
}

extern "C" void fake_wait_at(uint64_t i, int64_t *out)
{
    std::lock_guard<std::mutex> g(F->mu);
    for (int k = 0; k < 5; k++)
        out[k] = F->waits[5 * i + k];
}

extern "C" void fake_record_at(uint64_t i, int64_t *out)
{
    std::lock_guard<std::mutex> g(F->mu);
    for (int k = 0; k < 3; k++)
        out[k] = F->records[3 * i + k];
}

// ---- the pool -------------------------------------------------------------------
extern "C" void *pool_new(void)
{
    return new Pool();
}

// -> the set's number (in order of first hand-out), -1 for nullptr
extern "C" int pool_acquire(void *pool, int stream)
{
    Pool *p = static_cast<Pool *>(pool);
    Scratch *s = p->pool.acquire(reinterpret_cast<hipStream_t>((uintptr_t)stream));
    if (!s)
        return -1;
    std::lock_guard<std::mutex> g(p->mu);
    if (s->id < 0) {
        s->id = (int)p->sets.size();
        p->sets.push_back(s);
    }
    return s->id;
}

extern "C" void pool_release(void *pool, int set, int stream)
{
    Pool *p = static_cast<Pool *>(pool);
    Scratch *s;
    {
        std::lock_guard<std::mutex> g(p->mu);
        s = p->sets[set];
    }
    p->pool.release(s, reinterpret_cast<hipStream_t>((uintptr_t)stream));
}

// `threads` threads (at most kStreams - 1), each with its own stream, `rounds`
// rounds of acquire / hold / release on one device.  A set carries an owner
// word: a thread that finds another's in it saw a double hand-out.
// out: double hand-outs, nullptr acquires, most holders at once, sets seen.
extern "C" void pool_threads(void *pool, int threads, int rounds, uint64_t *out)
{
    Pool *p = static_cast<Pool *>(pool);
    std::atomic<uint64_t> doubles{0}, nulls{0};
    std::atomic<int> holders{0}, most{0};
    auto body = [&](int t) {
        const int stream = t + 1;
        unsigned rng = 12345u + 977u * (unsigned)t;
        for (int r = 0; r < rounds; r++) {
            const int id = pool_acquire(p, stream);
            if (id < 0) {
                nulls++;
                std::this_thread::yield();
                continue;
            }
            Scratch *s;
            {
                std::lock_guard<std::mutex> g(p->mu);
                s = p->sets[id];
            }
            if (s->owner.exchange(t + 1) != 0)
                doubles++;
            const int h = ++holders;
            int m = most.load();
            while (h > m && !most.compare_exchange_weak(m, h)) {
            }
            rng = rng * 1664525u + 1013904223u;
            (void)fake_work(stream);
            for (unsigned k = 0; k < ((rng >> 24) & 3); k++)   // hold it for a while
                std::this_thread::yield();
            holders--;
            if (s->owner.exchange(0) != t + 1)
                doubles++;
            pool_release(p, id, stream);
            if ((rng >> 16) & 1)   // the stream drains now and then
                fake_set_done(stream, fake_queued(stream));
        }
    };
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++)
        th.emplace_back(body, t);
    for (auto &x : th)
        x.join();
    out[0] = doubles;
    out[1] = nulls;
    out[2] = (uint64_t)most.load();
    std::lock_guard<std::mutex> g(p->mu);
    out[3] = p->sets.size();
}

#ifdef POOL_SHIM_MAIN
#include <stdio.h>
int main()
{
    uint64_t out[4];
    pool_threads(pool_new(), 8, 20000, out);
    printf("double hand-outs %llu, nullptr %llu, most holders %llu, sets %llu\n", (unsigned long long)out[0],
           (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3]);
    return out[0] == 0 && out[2] <= (uint64_t)zsk::kPoolSets && out[3] <= (uint64_t)zsk::kPoolSets ? 0 : 1;
}
#endif
