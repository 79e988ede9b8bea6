// alloc_model.cpp -- the device allocator (csrc/dev_alloc.h, the real header, unmodified) on the CPU, against a host model of
// the HIP calls it makes (hip/hip_runtime.h beside this file), from several threads.  Built plain, with -fsanitize=thread and with
// -fsanitize=address,undefined by tests/test_alloc_model_cpu.py; prints its counters, returns non-zero on any violation.
//
// What is checked.  A "context" here is a registered stream slot.  Just before every release(p) the checker notes, for every
// context alive on the block's device, its stream and that stream's enqueued count (a TICKET: the work that may still touch p).
//   - alloc() returns a block that was released before: every ticket is complete.
//   - alloc_ws(bytes, stream) returns one: every ticket is complete, or on `stream` itself, or covered by a wait noted on `stream`.
//   - no address is live twice; no hand-out of an address the driver has taken back; every hipFree is of a block that is not live.
//   - at the end of a run: live_bytes == 0, the per-device cached_bytes sum to the global figure, a device's cached_bytes are the
//     bytes of the blocks released and not handed out again, and a trim leaves nothing of the device outstanding in the driver.
// The tickets come from the checker's own list of contexts, not from the allocator's registrations: a context whose stream is
// unregistered while its work is still queued (the wrong order for a destroy) shows as a hand-out with an incomplete ticket.
#include "dev_alloc.h"

#include <atomic>
#include <random>

namespace {

using hipmodel::advance;
using hipmodel::drain;
using hipmodel::enqueue;

struct ctx_t {
    hipStream_t slot = nullptr;            // what the allocator reads (registered by address), re-pointed by set_stream
    std::atomic<hipStream_t> cur{nullptr}; // the checker's copy of it
    std::atomic<bool> alive{false};        // the context exists: its queued work may touch blocks
    int dev = 0;
};
struct ticket_t { hipStream_t st; unsigned long n; };
struct blk_t {
    size_t bytes = 0;
    int dev = 0;
    bool live = false;
    std::vector<ticket_t> tickets;
};
struct checker_t {
    std::mutex mu;
    std::deque<ctx_t> ctxs;
    std::unordered_map<void*, blk_t> blocks;
    long violations = 0, rehandouts = 0, fresh = 0, ws_wait_handouts = 0, printed = 0;
    bool quiet = false;                    // inside a negative control
};
checker_t& K() { static checker_t k; return k; }
long g_fails = 0;

void violation_locked(const char* what, void* p) {
    checker_t& k = K();
    k.violations++;
    if (!k.quiet && k.printed++ < 20) printf("VIOLATION: %s (block %p)\n", what, p);
}
#define EXPECT(cond) do { if (!(cond)) { g_fails++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

ctx_t* ctx_new(int dev) {
    checker_t& k = K();
    std::lock_guard<std::mutex> g(k.mu);
    k.ctxs.emplace_back();
    ctx_t* c = &k.ctxs.back();
    c->slot = hipmodel::new_stream(dev);
    c->cur.store(c->slot);
    c->dev = dev;
    return c;
}
// the calling thread's current device is c->dev
void ctx_register(ctx_t* c) { c->alive.store(true); devalloc::register_stream(&c->slot); }
// a destroy in the right order: drain, then let the allocator forget the stream
void ctx_unregister(ctx_t* c) {
    drain(c->slot);
    devalloc::unregister_stream(&c->slot);
    c->alive.store(false);
}
ctx_t* ctx_create(int dev) { ctx_t* c = ctx_new(dev); ctx_register(c); return c; }
// tfhe_ctx_set_stream: synchronise the old stream, re-point the slot under the allocator's lock
void ctx_set_stream(ctx_t* c, hipStream_t v) {
    drain(c->slot);
    devalloc::set_stream(&c->slot, v);
    c->cur.store(v);
}

void on_handout(void* p, size_t bytes, int dev, hipStream_t ws_stream) {
    checker_t& k = K();
    std::lock_guard<std::mutex> g(k.mu);
    if (!hipmodel::is_outstanding(p)) violation_locked("handed out an address the driver has taken back", p);
    auto it = k.blocks.find(p);
    if (it == k.blocks.end()) {
        blk_t b;
        b.bytes = bytes; b.dev = dev; b.live = true;
        k.blocks.emplace(p, std::move(b));
        k.fresh++;
        return;
    }
    blk_t& b = it->second;
    if (b.live) { violation_locked("address handed out while live", p); return; }
    if (b.bytes != bytes || b.dev != dev) violation_locked("block came back with another size or device", p);
    k.rehandouts++;
    bool by_wait = false;
    for (const ticket_t& t : b.tickets) {
        if (t.st->done.load() >= t.n) continue;
        if (ws_stream && t.st == ws_stream) continue;
        if (ws_stream && hipmodel::waits_for(ws_stream, t.st, t.n)) { by_wait = true; continue; }
        violation_locked(ws_stream ? "alloc_ws handed out a block whose release ticket is neither complete nor waited for"
                                   : "alloc handed out a block whose release ticket is not complete", p);
    }
    if (by_wait) k.ws_wait_handouts++;
    b.live = true;
    b.tickets.clear();
}
void before_release(void* p) {
    checker_t& k = K();
    std::lock_guard<std::mutex> g(k.mu);
    auto it = k.blocks.find(p);
    if (it == k.blocks.end() || !it->second.live) { violation_locked("release of a block that is not live", p); return; }
    blk_t& b = it->second;
    b.live = false;
    b.tickets.clear();
    for (ctx_t& c : k.ctxs) {
        if (!c.alive.load() || c.dev != b.dev) continue;
        hipStream_t st = c.cur.load();
        b.tickets.push_back(ticket_t{st, st->enq.load()});
    }
}
void on_free(void* p) {                    // the model's hipFree hook
    checker_t& k = K();
    std::lock_guard<std::mutex> g(k.mu);
    auto it = k.blocks.find(p);
    if (it == k.blocks.end()) return;
    if (it->second.live) violation_locked("hipFree of a live block", p);
    k.blocks.erase(it);
}

hipError_t c_alloc(size_t bytes, int dev, void** p) {
    const hipError_t e = devalloc::alloc(bytes, p);
    if (e == hipSuccess) on_handout(*p, bytes, dev, nullptr);
    else (void)hipGetLastError();
    return e;
}
hipError_t c_alloc_ws(size_t bytes, int dev, hipStream_t st, void** p, size_t* got) {
    const hipError_t e = devalloc::alloc_ws(bytes, st, p, got);
    if (e == hipSuccess) on_handout(*p, *got, dev, st);
    else (void)hipGetLastError();
    return e;
}
hipError_t c_release(void* p) {
    before_release(p);
    return devalloc::release(p);
}
void trim_current_device() {
    devalloc::state_t& s = devalloc::S();
    std::lock_guard<std::mutex> g(s.mu);
    devalloc::trim_locked(s);
}

struct snap_t {
    long waits, trims, reuses, mallocs, violations, rehandouts, fresh, ws_wait;
    size_t live_bytes, cached_bytes;
};
snap_t snap() {
    snap_t r;
    {
        devalloc::state_t& s = devalloc::S();
        std::lock_guard<std::mutex> g(s.mu);
        r.waits = s.n_wait; r.trims = s.n_trim; r.reuses = s.n_reuse; r.mallocs = s.n_hip_malloc;
        r.live_bytes = s.live_bytes; r.cached_bytes = s.cached_bytes;
    }
    checker_t& k = K();
    std::lock_guard<std::mutex> g(k.mu);
    r.violations = k.violations; r.rehandouts = k.rehandouts; r.fresh = k.fresh; r.ws_wait = k.ws_wait_handouts;
    return r;
}
size_t dev_cached(int dev) {
    devalloc::state_t& s = devalloc::S();
    std::lock_guard<std::mutex> g(s.mu);
    auto it = s.devs.find(dev);
    return it == s.devs.end() ? 0 : it->second.cached_bytes;
}
size_t dev_parked(int dev) {
    devalloc::state_t& s = devalloc::S();
    std::lock_guard<std::mutex> g(s.mu);
    auto it = s.devs.find(dev);
    return it == s.devs.end() ? 0 : it->second.parked.size();
}
// the accounting at the end of a run or a scenario on `dev` (everything released, the calling thread on `dev`)
void check_accounting(int dev) {
    {
        devalloc::state_t& s = devalloc::S();
        std::lock_guard<std::mutex> g(s.mu);
        EXPECT(s.live_bytes == 0);
        EXPECT(s.live.empty());
        size_t sum = 0;
        for (auto& kv : s.devs) sum += kv.second.cached_bytes;
        EXPECT(sum == s.cached_bytes);
    }
    size_t released = 0, live = 0;
    {
        checker_t& k = K();
        std::lock_guard<std::mutex> g(k.mu);
        for (auto& kv : k.blocks) {
            if (kv.second.dev != dev) continue;
            if (kv.second.live) live++; else released += kv.second.bytes;
        }
    }
    EXPECT(live == 0);
    EXPECT(released == dev_cached(dev));
    trim_current_device();
    EXPECT(dev_cached(dev) == 0);
    EXPECT(hipmodel::outstanding_blocks(dev) == 0);
}

// ---- scripted scenarios: one thread drives the allocator, each on a device of its own ------------------------------------

// a block released while another context's stream is busy comes back only after that stream has advanced
void scenario_busy_stream(int dev) {
    (void)hipSetDevice(dev);
    ctx_t *a = ctx_create(dev), *b = ctx_create(dev);
    const snap_t s0 = snap();
    void *p = nullptr, *q = nullptr, *r = nullptr;
    EXPECT(c_alloc(4096, dev, &p) == hipSuccess);
    enqueue(b->slot, 3);
    EXPECT(c_release(p) == hipSuccess);
    EXPECT(c_alloc(4096, dev, &q) == hipSuccess);
    EXPECT(q != p);
    advance(b->slot, 2);
    void* q2 = nullptr;
    EXPECT(c_alloc(4096, dev, &q2) == hipSuccess);
    EXPECT(q2 != p);                                             // one item of B's is still pending
    advance(b->slot, 1);
    EXPECT(c_alloc(4096, dev, &r) == hipSuccess);
    EXPECT(r == p);
    const snap_t s1 = snap();
    EXPECT(s1.reuses - s0.reuses == 1 && s1.mallocs - s0.mallocs == 3 && s1.violations == s0.violations);
    c_release(q); c_release(q2); c_release(r);
    ctx_unregister(a); ctx_unregister(b);
    check_accounting(dev);
}
// past the soft threshold alloc waits for the oldest parked block of its size and returns that address
void scenario_back_pressure(int dev) {
    (void)hipSetDevice(dev);
    hipmodel::set_total(dev, 48 << 10);                          // bound 16 KiB, soft threshold 4 KiB
    ctx_t *a = ctx_create(dev), *b = ctx_create(dev);
    void *p = nullptr, *p2 = nullptr, *q = nullptr;
    EXPECT(c_alloc(8192, dev, &p) == hipSuccess);
    EXPECT(c_alloc(8192, dev, &p2) == hipSuccess);
    enqueue(b->slot, 3);
    EXPECT(c_release(p) == hipSuccess);
    enqueue(b->slot, 1);
    EXPECT(c_release(p2) == hipSuccess);                         // the younger one: not the one waited for
    const snap_t s0 = snap();
    std::thread dev_thread([b] {
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
        advance(b->slot, 3);
    });
    EXPECT(c_alloc(8192, dev, &q) == hipSuccess);
    dev_thread.join();
    EXPECT(q == p);
    const snap_t s1 = snap();
    EXPECT(s1.waits - s0.waits == 1 && s1.reuses - s0.reuses == 1 && s1.mallocs == s0.mallocs && s1.violations == s0.violations);
    c_release(q);
    ctx_unregister(a); ctx_unregister(b);
    check_accounting(dev);
}
// alloc_ws takes a parked block of bytes .. 2 x bytes and makes its stream wait for the release events
void scenario_ws_wait(int dev) {
    (void)hipSetDevice(dev);
    ctx_t *a = ctx_create(dev), *b = ctx_create(dev);
    void *p = nullptr, *w = nullptr;
    size_t got = 0;
    EXPECT(c_alloc(8192, dev, &p) == hipSuccess);
    const unsigned long tb = enqueue(b->slot, 4);
    EXPECT(c_release(p) == hipSuccess);
    const snap_t s0 = snap();
    EXPECT(c_alloc_ws(6000, dev, a->slot, &w, &got) == hipSuccess);
    EXPECT(w == p && got == 8192);
    EXPECT(hipmodel::waits_for(a->slot, b->slot, tb));
    const snap_t s1 = snap();
    EXPECT(s1.reuses - s0.reuses == 1 && s1.ws_wait - s0.ws_wait == 1 && s1.mallocs == s0.mallocs && s1.violations == s0.violations);
    // A's work behind the wait does not run before B's ticket is done
    enqueue(a->slot, 1);
    advance(a->slot, 1);
    EXPECT(a->slot->done.load() == 0);
    advance(b->slot, 4);
    advance(a->slot, 1);
    EXPECT(a->slot->done.load() == 1);
    c_release(w);
    ctx_unregister(a); ctx_unregister(b);
    check_accounting(dev);
}
// a stream the caller destroyed: release takes the synchronising hipFree path and the cache does not change
void scenario_destroyed_stream(int dev) {
    (void)hipSetDevice(dev);
    ctx_t *a = ctx_create(dev), *b = ctx_create(dev);
    void* p = nullptr;
    EXPECT(c_alloc(4096, dev, &p) == hipSuccess);
    b->slot->destroyed.store(true);
    const snap_t s0 = snap();
    const long f0 = hipmodel::W().n_free;
    EXPECT(c_release(p) == hipSuccess);
    const snap_t s1 = snap();
    EXPECT(!hipmodel::is_outstanding(p));
    EXPECT(hipmodel::W().n_free - f0 == 1);
    EXPECT(s1.cached_bytes == s0.cached_bytes && dev_cached(dev) == 0 && dev_parked(dev) == 0);
    EXPECT(s1.live_bytes + 4096 == s0.live_bytes && s1.violations == s0.violations);
    b->slot->destroyed.store(false);
    ctx_unregister(a); ctx_unregister(b);
    check_accounting(dev);
}
// released by a thread whose current device differs: parked on the block's own device, the caller's device restored
void scenario_other_device(int dev, int other) {
    (void)hipSetDevice(other);
    ctx_t* o = ctx_create(other);
    (void)hipSetDevice(dev);
    ctx_t* a = ctx_create(dev);
    void* p = nullptr;
    EXPECT(c_alloc(4096, dev, &p) == hipSuccess);
    enqueue(o->slot, 2);                                         // busy, but on the other device: no event of this block's
    (void)hipSetDevice(other);
    EXPECT(c_release(p) == hipSuccess);
    int cur = -1;
    (void)hipGetDevice(&cur);
    EXPECT(cur == other);
    EXPECT(dev_cached(dev) == 4096 && dev_parked(dev) == 1 && dev_cached(other) == 0 && dev_parked(other) == 0);
    void* q = nullptr;
    EXPECT(c_alloc(4096, other, &q) == hipSuccess);              // the other device's cache has nothing to give
    EXPECT(q != p);
    c_release(q);
    ctx_unregister(o);
    check_accounting(other);
    (void)hipSetDevice(dev);
    void* r = nullptr;
    EXPECT(c_alloc(4096, dev, &r) == hipSuccess);
    EXPECT(r == p);
    c_release(r);
    ctx_unregister(a);
    check_accounting(dev);
}
// a hard hipEventQuery error on an event of the block at the FRONT of the parked queue: later blocks whose own events have
// completed still become ready, the failed block is never handed out and leaves the queue
void scenario_query_error(int dev) {
    (void)hipSetDevice(dev);
    ctx_t *a = ctx_create(dev), *b = ctx_create(dev);
    void *p1 = nullptr, *p2 = nullptr, *p3 = nullptr;
    EXPECT(c_alloc(4096, dev, &p1) == hipSuccess);
    EXPECT(c_alloc(4096, dev, &p2) == hipSuccess);
    EXPECT(c_alloc(4096, dev, &p3) == hipSuccess);
    enqueue(b->slot, 2);
    c_release(p1);
    c_release(p2);
    enqueue(b->slot, 1);
    c_release(p3);
    {
        devalloc::state_t& s = devalloc::S();
        std::lock_guard<std::mutex> g(s.mu);
        devalloc::dev_state_t& d = s.devs[dev];
        EXPECT(d.parked.size() == 3 && d.parked.front().p == p1 && d.parked.front().evs.size() == 2);
        d.parked.front().evs.back()->fail = true;
    }
    advance(b->slot, 2);                                         // p2's events are done, p3's are not
    const snap_t s0 = snap();
    void *q = nullptr, *r = nullptr;
    EXPECT(c_alloc(4096, dev, &q) == hipSuccess);
    EXPECT(q == p2);
    EXPECT(!hipmodel::is_outstanding(p1));                       // retired: back to the driver, out of the queue and the count
    EXPECT(dev_parked(dev) == 1 && dev_cached(dev) == 4096);
    EXPECT(c_alloc(4096, dev, &r) == hipSuccess);
    EXPECT(r != p1 && r != p3);
    advance(b->slot, 1);
    void* t = nullptr;
    EXPECT(c_alloc(4096, dev, &t) == hipSuccess);
    EXPECT(t == p3);
    const snap_t s1 = snap();
    EXPECT(s1.reuses - s0.reuses == 2 && s1.mallocs - s0.mallocs == 1 && s1.violations == s0.violations);
    c_release(q); c_release(r); c_release(t);
    ctx_unregister(a); ctx_unregister(b);
    check_accounting(dev);
}
// The destroy-order rule.  Context A has work queued that reads p.  A destroy that lets the allocator forget A's stream BEFORE
// draining it leaves a window in which a free of p (legal: the call that enqueued the work has returned) records no event on A,
// and the next alloc gets p while that work is pending: the checker must report it (negative control).  Drain first: no report.
void scenario_destroy_order(int dev, bool drain_first) {
    (void)hipSetDevice(dev);
    ctx_t *a = ctx_create(dev), *b = ctx_create(dev);
    void *p = nullptr, *q = nullptr;
    EXPECT(c_alloc(4096, dev, &p) == hipSuccess);
    enqueue(a->slot, 5);
    const snap_t s0 = snap();
    if (drain_first) drain(a->slot);
    devalloc::unregister_stream(&a->slot);
    K().quiet = !drain_first;
    c_release(p);                                                // "another thread", inside the destroy
    EXPECT(c_alloc(4096, dev, &q) == hipSuccess);
    K().quiet = false;
    EXPECT(q == p);
    drain(a->slot);                                              // the rest of the destroy
    a->alive.store(false);
    const snap_t s1 = snap();
    if (drain_first) EXPECT(s1.violations == s0.violations);
    else {
        EXPECT(s1.violations - s0.violations == 1);
        std::lock_guard<std::mutex> g(K().mu);
        K().violations = s0.violations;                          // expected: not counted against the run
    }
    c_release(q);
    ctx_unregister(b);
    check_accounting(dev);
}

// ---- the threaded run -----------------------------------------------------------------------------------------------------

constexpr int WORKERS = 4;
constexpr size_t SIZES[3] = {4096, 8192, 16384};

void worker(int id, int dev, ctx_t* c, hipStream_t second, long moves) {
    (void)hipSetDevice(dev);
    std::mt19937_64 rng(1000 + id);
    std::vector<void*> held;
    hipStream_t other = second;
    for (long m = 0; m < moves; m++) {
        const unsigned r = (unsigned)(rng() % 1000);
        if (r < 250) {
            enqueue(c->slot, 1 + rng() % 3);
        } else if (r < 600) {
            if (held.size() >= 8) continue;
            void* p = nullptr;
            if (c_alloc(SIZES[rng() % 3], dev, &p) != hipSuccess) continue;
            enqueue(c->slot, 1);                                 // a kernel that uses it
            held.push_back(p);
        } else if (r < 680) {
            if (held.size() >= 8) continue;
            void* p = nullptr;
            size_t got = 0;
            const size_t sz = SIZES[rng() % 3];
            if (c_alloc_ws((rng() & 1) ? sz : sz / 4 * 3, dev, c->slot, &p, &got) != hipSuccess) continue;
            enqueue(c->slot, 1);
            held.push_back(p);
        } else if (r < 960) {
            if (held.empty()) continue;
            const size_t i = rng() % held.size();
            c_release(held[i]);
            held[i] = held.back();
            held.pop_back();
        } else if (r < 995) {
            hipStream_t was = c->slot;
            ctx_set_stream(c, other);
            other = was;
        } else if (r < 997) {
            trim_current_device();
        } else {
            std::this_thread::yield();
        }
    }
    for (void* p : held) c_release(p);
}

snap_t threaded_run(const char* name, int dev, size_t total, long moves, bool lying, int device_sleep_us) {
    (void)hipSetDevice(dev);
    if (total) hipmodel::set_total(dev, total);
    ctx_t* ctx[WORKERS];
    hipStream_t second[WORKERS];
    std::vector<hipStream_t> all;
    for (int i = 0; i < WORKERS; i++) {
        ctx[i] = ctx_create(dev);
        second[i] = hipmodel::new_stream(dev);
        all.push_back(ctx[i]->slot);
        all.push_back(second[i]);
    }
    ctx_t* fifth = ctx_new(dev);
    const snap_t s0 = snap();
    K().quiet = lying;
    hipmodel::lie().store(lying);
    std::atomic<bool> stop{false};
    std::thread device([&] {
        std::mt19937_64 rng(7);
        while (!stop.load()) {
            advance(all[rng() % all.size()], 1 + rng() % 6);
            if (device_sleep_us) std::this_thread::sleep_for(std::chrono::microseconds(device_sleep_us));
            else std::this_thread::yield();
        }
    });
    std::thread churn([&] {
        (void)hipSetDevice(dev);
        while (!stop.load()) {
            ctx_register(fifth);
            std::this_thread::yield();
            ctx_unregister(fifth);
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    });
    std::vector<std::thread> ws;
    for (int i = 0; i < WORKERS; i++) ws.emplace_back(worker, i, dev, ctx[i], second[i], moves);
    for (auto& t : ws) t.join();
    stop.store(true);
    device.join();
    churn.join();
    hipmodel::lie().store(false);
    K().quiet = false;
    snap_t s1 = snap();
    for (int i = 0; i < WORKERS; i++) ctx_unregister(ctx[i]);
    if (!lying) check_accounting(dev);
    else trim_current_device();
    snap_t d;
    d.waits = s1.waits - s0.waits; d.trims = s1.trims - s0.trims; d.reuses = s1.reuses - s0.reuses; d.mallocs = s1.mallocs - s0.mallocs;
    d.violations = s1.violations - s0.violations; d.rehandouts = s1.rehandouts - s0.rehandouts; d.fresh = s1.fresh - s0.fresh;
    d.ws_wait = s1.ws_wait - s0.ws_wait; d.live_bytes = s1.live_bytes; d.cached_bytes = s1.cached_bytes;
    printf("run %s: rehandouts=%ld fresh=%ld reuses=%ld hip_mallocs=%ld waits=%ld trims=%ld ws_wait_handouts=%ld violations=%ld\n", name,
           d.rehandouts, d.fresh, d.reuses, d.mallocs, d.waits, d.trims, d.ws_wait, d.violations);
    return d;
}

}  // namespace

int main(int argc, char** argv) {
    const long moves = argc > 1 ? atol(argv[1]) : 30000;
    setvbuf(stdout, nullptr, _IOLBF, 0);
    hipmodel::W().on_free = on_free;

    scenario_busy_stream(10);
    scenario_back_pressure(11);
    scenario_ws_wait(12);
    scenario_destroyed_stream(13);
    scenario_other_device(14, 15);
    scenario_query_error(16);
    scenario_destroy_order(17, true);
    scenario_destroy_order(18, false);                           // negative control
    printf("scenarios: failed=%ld violations=%ld\n", g_fails, snap().violations);

    long bad = snap().violations;
    const snap_t ample = threaded_run("ample", 0, 0, moves, false, 0);
    // 768 KiB of device: the cache's bound is 256 KiB and its soft threshold 64 KiB, against up to 4 x 8 live blocks of 3-16 KiB
    const snap_t small = threaded_run("small", 1, (size_t)768 << 10, moves, false, 0);
    bad += ample.violations + small.violations;
    // negative control: a hipEventQuery that always answers "complete" must show as violations
    const snap_t lying = threaded_run("lying", 2, 0, moves / 4, true, 20);
    EXPECT(lying.violations > 0);
    printf("result: failed=%ld violations=%ld lying_violations=%ld\n", g_fails, bad, lying.violations);
    return (g_fails || bad) ? 1 : 0;
}
