// A host model of the eleven HIP calls csrc/dev_alloc.h makes, so that the allocator's real header runs on the CPU, on several
// threads, under ThreadSanitizer / AddressSanitizer (tests/alloc_model/alloc_model.cpp; this directory goes first on the include
// path and shadows the real <hip/hip_runtime.h>).
//
//   stream   two counters: work enqueued and work done (done <= enq).  Work item k of a stream is complete once done >= k.
//   event    remembers the stream it was recorded on and that stream's enqueued count at the record: complete once the
//            stream's done count has reached it.  A never-recorded event is complete.
//   wait     hipStreamWaitEvent notes (position, source stream, ticket) on the waiting stream: its work after `position` does not
//            complete before the source stream's done count has reached `ticket` (advance() honours the notes; they are kept
//            for the checker to read).
//   memory   hipMalloc returns unique fake addresses (never dereferenced, never reused) and fails with hipErrorOutOfMemory past
//            the modelled total of the calling thread's device; hipFree ABORTS on an address it did not hand out or has freed.
//   device   hipDeviceSynchronize completes every stream of the calling thread's device.
//
// Switches for scenarios: a stream marked `destroyed` fails hipEventRecord; an event marked `fail` makes hipEventQuery return a
// hard error; hipmodel::lie() makes hipEventQuery answer hipSuccess always (the negative control); hipmodel::set_total() sets the
// memory of a device, so that the allocator's thresholds are reached with kilobytes.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

typedef int hipError_t;
enum : int {
    hipSuccess = 0,
    hipErrorOutOfMemory = 2,
    hipErrorInvalidValue = 1,
    hipErrorContextIsDestroyed = 709,
    hipErrorNotReady = 600,
    hipErrorIllegalAddress = 700,
};
enum : unsigned { hipEventDisableTiming = 2 };

struct hipmodel_stream;
typedef hipmodel_stream* hipStream_t;
struct hipmodel_wait {
    unsigned long pos;      // the waiting stream's enqueued count when the wait was noted
    hipStream_t src;
    unsigned long ticket;
};
struct hipmodel_stream {
    std::atomic<unsigned long> enq{0}, done{0};
    std::atomic<bool> destroyed{false};
    int dev = 0;
    std::mutex wmu;                       // guards waits
    std::vector<hipmodel_wait> waits;
};
struct hipmodel_event {                   // touched only by the allocator, under its mutex (a race here is the allocator's)
    hipStream_t st = nullptr;
    unsigned long ticket = 0;
    bool fail = false;
};
typedef hipmodel_event* hipEvent_t;

namespace hipmodel {

struct world_t {
    std::mutex mu;                                    // streams, events, memory
    std::deque<hipmodel_stream> streams;              // (deque: stable addresses; owned here, so nothing leaks)
    std::deque<hipmodel_event> events;
    std::unordered_map<void*, std::pair<size_t, int>> blocks;   // outstanding address -> bytes, device
    std::map<int, size_t> total, used;                // per device
    size_t next_addr = (size_t)1 << 40;
    long n_malloc = 0, n_free = 0;
    void (*on_free)(void*) = nullptr;                 // the checker's hook, called for every hipFree before the block goes
};
inline world_t& W() { static world_t w; return w; }
inline std::atomic<bool>& lie() { static std::atomic<bool> l{false}; return l; }
inline int& cur_dev() { static thread_local int d = 0; return d; }
inline hipError_t& last_err() { static thread_local hipError_t e = hipSuccess; return e; }
inline hipError_t ret(hipError_t e) { if (e != hipSuccess) last_err() = e; return e; }

inline void set_total(int dev, size_t bytes) { std::lock_guard<std::mutex> g(W().mu); W().total[dev] = bytes; }
inline size_t outstanding_blocks(int dev) {
    std::lock_guard<std::mutex> g(W().mu);
    size_t n = 0;
    for (auto& kv : W().blocks) n += kv.second.second == dev;
    return n;
}
inline bool is_outstanding(void* p) { std::lock_guard<std::mutex> g(W().mu); return W().blocks.count(p) != 0; }
inline hipStream_t new_stream(int dev) {
    std::lock_guard<std::mutex> g(W().mu);
    W().streams.emplace_back();
    W().streams.back().dev = dev;
    return &W().streams.back();
}
inline void raise(std::atomic<unsigned long>& a, unsigned long v) {
    unsigned long c = a.load();
    while (c < v && !a.compare_exchange_weak(c, v)) {}
}
inline unsigned long enqueue(hipStream_t s, unsigned long n = 1) { return s->enq.fetch_add(n) + n; }
// the device makes progress on one stream: up to n more items, none past a noted wait whose source has not got there
inline void advance(hipStream_t s, unsigned long n) {
    std::lock_guard<std::mutex> g(s->wmu);
    const unsigned long d = s->done.load();
    unsigned long target = std::min(s->enq.load(), d + n);
    for (const hipmodel_wait& w : s->waits)
        if (w.pos < target && w.src->done.load() < w.ticket) target = w.pos;
    if (target > d) raise(s->done, target);
}
// the host waits for a stream (hipStreamSynchronize): time passes until everything enqueued so far is done, which takes what
// the stream waits for with it.  (Waits point at events recorded earlier, so the recursion ends.)
inline void complete_to(hipStream_t s, unsigned long upto) {
    if (s->done.load() >= upto) return;
    std::vector<hipmodel_wait> ws;
    { std::lock_guard<std::mutex> g(s->wmu); ws = s->waits; }
    for (const hipmodel_wait& w : ws)
        if (w.pos < upto) complete_to(w.src, w.ticket);
    raise(s->done, upto);
}
inline void drain(hipStream_t s) { complete_to(s, s->enq.load()); }
inline bool waits_for(hipStream_t s, hipStream_t src, unsigned long ticket) {
    std::lock_guard<std::mutex> g(s->wmu);
    for (const hipmodel_wait& w : s->waits)
        if (w.src == src && w.ticket >= ticket) return true;
    return false;
}

}  // namespace hipmodel

inline hipError_t hipGetLastError() { hipError_t e = hipmodel::last_err(); hipmodel::last_err() = hipSuccess; return e; }
inline hipError_t hipGetDevice(int* d) { *d = hipmodel::cur_dev(); return hipSuccess; }
inline hipError_t hipSetDevice(int d) {
    if (d < 0 || d >= 64) return hipmodel::ret(hipErrorInvalidValue);
    hipmodel::cur_dev() = d;
    return hipSuccess;
}
inline hipError_t hipMemGetInfo(size_t* fr, size_t* tot) {
    hipmodel::world_t& w = hipmodel::W();
    std::lock_guard<std::mutex> g(w.mu);
    const int d = hipmodel::cur_dev();
    auto it = w.total.find(d);
    *tot = it == w.total.end() ? (size_t)288 << 30 : it->second;
    const size_t u = w.used[d];
    *fr = u < *tot ? *tot - u : 0;
    return hipSuccess;
}
inline hipError_t hipDeviceSynchronize() {
    hipmodel::world_t& w = hipmodel::W();
    std::lock_guard<std::mutex> g(w.mu);
    for (hipmodel_stream& s : w.streams)
        if (s.dev == hipmodel::cur_dev()) hipmodel::raise(s.done, s.enq.load());
    return hipSuccess;
}
template <class T>
inline hipError_t hipMalloc(T** out, size_t bytes) {
    hipmodel::world_t& w = hipmodel::W();
    std::lock_guard<std::mutex> g(w.mu);
    const int d = hipmodel::cur_dev();
    auto it = w.total.find(d);
    const size_t tot = it == w.total.end() ? (size_t)288 << 30 : it->second;
    if (w.used[d] + bytes > tot) return hipmodel::ret(hipErrorOutOfMemory);
    void* p = (void*)w.next_addr;
    w.next_addr += (bytes + 255) / 256 * 256 + 256;
    w.blocks[p] = {bytes, d};
    w.used[d] += bytes;
    w.n_malloc++;
    *out = (T*)p;
    return hipSuccess;
}
inline hipError_t hipFree(void* p) {
    if (!p) return hipSuccess;
    hipmodel::world_t& w = hipmodel::W();
    void (*hook)(void*) = nullptr;
    {
        std::lock_guard<std::mutex> g(w.mu);
        if (!w.blocks.count(p)) {
            fprintf(stderr, "hip model: hipFree(%p) of an address that was not handed out or has been freed\n", p);
            abort();
        }
        hook = w.on_free;
    }
    if (hook) hook(p);
    std::lock_guard<std::mutex> g(w.mu);
    auto it = w.blocks.find(p);
    w.used[it->second.second] -= it->second.first;
    w.blocks.erase(it);
    w.n_free++;
    return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) {
    hipmodel::world_t& w = hipmodel::W();
    std::lock_guard<std::mutex> g(w.mu);
    w.events.emplace_back();
    *ev = &w.events.back();
    return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t ev, hipStream_t s) {
    if (!ev || !s) return hipmodel::ret(hipErrorInvalidValue);
    if (s->destroyed.load()) return hipmodel::ret(hipErrorContextIsDestroyed);
    ev->st = s;
    ev->ticket = s->enq.load();
    return hipSuccess;
}
inline hipError_t hipEventQuery(hipEvent_t ev) {
    if (!ev) return hipmodel::ret(hipErrorInvalidValue);
    if (hipmodel::lie().load()) return hipSuccess;
    if (ev->fail) return hipmodel::ret(hipErrorIllegalAddress);
    if (!ev->st || ev->st->done.load() >= ev->ticket) return hipSuccess;
    return hipmodel::ret(hipErrorNotReady);
}
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t ev, unsigned) {
    if (!ev || !s) return hipmodel::ret(hipErrorInvalidValue);
    if (!ev->st || ev->st == s) return hipSuccess;               // stream order covers it
    std::lock_guard<std::mutex> g(s->wmu);
    s->waits.push_back(hipmodel_wait{s->enq.load(), ev->st, ev->ticket});
    return hipSuccess;
}
