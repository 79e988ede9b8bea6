// toyfhe_hip.hip -- context management and the C ABI of libtoyfhe_hip.so (see include/toyfhe_hip.h).
// gfx950 only.  No torch types, no oracle code, no CPU fallback: every compute entry point launches
// HIP kernels and fails with TFHE_E_HIP if the device is unavailable.
#include <hip/hip_runtime.h>
#include <chrono>

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/toyfhe_hip.h"
#include "bfv_tables.h"
#include "plain_tables.h"
#include "host_math.h"
#include "kernels.h"
#include "mul_core.h"
#include "ckks_kernels.h"
#include "sample_kernels.h"
#include "enc_core.h"
#include "keygen_core.h"
#include "dot_core.h"
#include "ntt_tables.h"
#include "dev_alloc.h"
#include "ws_layout.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail(TFHE_E_HIP, "%s: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

struct prof_pair {
    hipEvent_t a, b;
    int64_t limb_polys;
};

// The environment switches, each read once where it is used.  A switch that defaults to on is
// turned off by a value starting with '0'; one that defaults to off is turned on by a value starting with '1'.
bool env_flag(const char* name, bool dflt) {
    const char* e = getenv(name);
    return dflt ? !(e && e[0] == '0') : (e && e[0] == '1');
}
int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
size_t env_gib(const char* name, long dflt) {   // a positive number of GiB, in bytes
    const char* e = getenv(name);
    const long g = e ? atol(e) : 0;
    return (size_t)(g > 0 ? g : dflt) << 30;
}

}  // namespace

struct tfhe_ctx {
    int64_t N = 0;
    int logN = 0, L = 0;
    std::vector<u64> q, psi;
    std::vector<ntt_limb_t> limbs_host;
    ntt_limb_t* limbs_dev = nullptr;
    std::vector<void*> tabs;   // device twiddle tables (W, Winv and their fp64 twins per limb)
    int num_cus = 256;
    hipStream_t stream = nullptr;        // the stream launches go to: main_stream, or side_stream inside a forked region (lanes_t)
    hipStream_t main_stream = nullptr;   // the context's stream as its users know it (the slot the allocator records release events on)
    bool own_stream = false;
    // second lane (r06): rings that mix the two arithmetic policies (60-bit q0 / special prime beside 40-bit primes) run the
    // launches of one policy on side_stream beside those of the other, forked from and joined back into main_stream by events
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int lane_depth = 0;                  // > 0: inside a forked region (nested lanes_t objects only switch streams)
    bool lanes_broken = false;           // creating the second stream failed once: stay serial
    int variant = 0;
    int chunk_cap = 0;                   // tfhe_ctx_set_chunk: bound on every internal chunk (0 = the defaults)
    // workspace (grown on demand, reused)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    bool ws_pooled = false;   // the block came from the recycling allocator (large per-call workspaces, ws_borrow_t)
    ws_scratch_state_t ws_scratch;   // the layout in force, if any: what of the block's start the transforms may take (ws_layout.h)
    // profiling
    bool prof = false;
    std::vector<prof_pair> prof_pairs;
    // CKKS encode / decode tables (built on first use): FFT roots, twist, scatter / gather positions
    void *ckks_roots = nullptr, *ckks_tw = nullptr, *ckks_pos = nullptr, *ckks_gpos = nullptr;
    // exact-reconstruction tables of the window key switch, per level (built on first use)
    std::map<int, conv_tab_t*> ksw_tabs;
    std::vector<void*> ksw_allocs;
    // the tables of the grouped key switch, one conv_tab_t per digit, per (key_limbs, level, n_special, group) (same lock, same frees)
    std::map<std::array<int, 4>, conv_tab_t*> ksg_tabs;
    std::mutex ksw_mu;
    // N zero words (the "+ c" stream of the fused contraction for the component that has no addend), made on first use
    // (under zero_mu; a failed attempt is retried by the next call)
    u64* zero_row = nullptr;
    std::mutex zero_mu;
};

namespace {

// pooled: the block is taken from (and, by ws_borrow_t, returned to) the recycling allocator instead of being owned by the
// context for its lifetime -- for the large per-call workspaces (tfhe_matmul_diag: tens of GiB).  A parked block is reused by
// the next call of the same shape without a synchronisation, counts against the allocator's cache bound, and is given back to
// the driver by tfhe_alloc_trim and by every out-of-memory retry of the library (devalloc::malloc_retry).
int ensure_ws(tfhe_ctx* c, size_t bytes, void** out, bool pooled = false) {
    if (bytes > c->ws_bytes) {
        if (c->ws) {
            // the slot is cleared BEFORE anything can return (r05, ADVICE r04: devalloc::release erases the block from its live
            // table even when it reports an error -- a context left pointing at it would hand a stale pointer to the next free)
            void* old = c->ws;
            const bool old_pooled = c->ws_pooled;
            c->ws = nullptr;
            c->ws_bytes = 0;
            c->ws_pooled = false;
            if (old_pooled) {
                HIP_TRY(devalloc::release(old));                 // parked behind events on every context stream: no wait
            } else {
                HIP_TRY(hipStreamSynchronize(c->stream));
                HIP_TRY(hipFree(old));
            }
        }
        size_t got = bytes;
        hipError_t e = pooled ? devalloc::alloc_ws(bytes, c->stream, &c->ws, &got) : devalloc::malloc_retry(&c->ws, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); c->ws = nullptr; return fail(TFHE_E_NOMEM, "workspace hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); }
        c->ws_bytes = got;
        c->ws_pooled = pooled;
    }
    *out = c->ws;
    return TFHE_OK;
}
// The one allocation of a call that lays out the block (ws_layout.h): the context's own, grown to the layout, or -- for a nested user --
// the span its caller carved for it, which must hold the layout.  `scope`: the layout is in force until it goes (nullptr: the caller
// sets its own scope later).
int ws_begin(tfhe_ctx* c, const ws_layout_t& L, int64_t chunk, const ws_span_t* span, void** ws, ws_scope_t* scope) {
    const size_t bytes = L.bytes(chunk);
    if (span) {
        if (bytes > span->bytes) return fail(TFHE_E_HIP, "internal: a nested workspace of %zu bytes, its span holds %zu", bytes, span->bytes);
        *ws = span->ptr;
    } else if (int rc = ensure_ws(c, bytes, ws)) return rc;
    if (scope) scope->set(c->ws_scratch, L.region0(chunk));
    return TFHE_OK;
}
// The intermediate of a transform (run_ntt_large, run_ntt's two lanes, the mixed lifts of ks_digits_fwd and md_lift_fwd): the start of
// the context's block -- grown to the request when no layout is in force, region 0 of the layout otherwise, never more
int ws_scratch(tfhe_ctx* c, size_t bytes, void** out) {
    switch (ws_scratch_decide(c->ws_scratch, bytes)) {
    case WS_SCRATCH_GROW: return ensure_ws(c, bytes, out);
    case WS_SCRATCH_FITS: *out = c->ws; return TFHE_OK;
    default: return fail(TFHE_E_HIP, "internal: transform scratch of %zu bytes, region 0 holds %zu", bytes, c->ws_scratch.region0);
    }
}
// The ciphertexts (polynomials, for the samplers and codecs) one iteration of a chunked entry point takes: the whole batch, at
// most `dflt` of it, at most what `bytes_cap` holds at `per_ct` bytes each (per_ct = 0: no such bound), at most the context's
// cap (tfhe_ctx_set_chunk), at least one.  EVERY chunked entry point sizes its chunk here.
int64_t chunk_of(const tfhe_ctx* c, int64_t batch, int64_t dflt, size_t bytes_cap = 0, size_t per_ct = 0) {
    int64_t m = std::min(batch, dflt);
    if (per_ct) m = std::min(m, (int64_t)(bytes_cap / per_ct));
    if (c->chunk_cap) m = std::min(m, (int64_t)c->chunk_cap);
    return std::max<int64_t>(1, m);
}
// A pooled workspace lives for ONE call: the context's own (long-lived, small) workspace is set aside while the call runs --
// the transforms inside it take their scratch from c->ws -- and comes back untouched when the call returns; the pooled block
// goes back to the allocator.  (First form, r04: the pooled block REPLACED the context's workspace; every large call then cost
// the next small operation a hipMalloc and itself a stream synchronisation + hipFree of that small block: the encrypted-MNIST
// pass went from 78 to 145 ms.)
struct ws_borrow_t {
    tfhe_ctx* c;
    void* ws = nullptr;
    size_t bytes = 0;
    bool pooled = false, active = false;
    explicit ws_borrow_t(tfhe_ctx* ctx) : c(ctx) {}
    void begin() {
        ws = c->ws; bytes = c->ws_bytes; pooled = c->ws_pooled; active = true;
        c->ws = nullptr; c->ws_bytes = 0; c->ws_pooled = false;
    }
    ~ws_borrow_t() {
        if (!active) return;
        if (c->ws) { if (c->ws_pooled) (void)devalloc::release(c->ws); else { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->ws); } }
        c->ws = ws; c->ws_bytes = bytes; c->ws_pooled = pooled;
    }
};
// workspaces above this size are per-call (pooled); TFHE_WS_KEEP_GIB overrides
size_t ws_keep_bytes() {
    static const size_t keep = env_gib("TFHE_WS_KEEP_GIB", 4);
    return keep;
}

// ---- two lanes ------------------------------------------------------------------------------------------------------------
// A ring that mixes fp64-size moduli with larger ones runs every transform / key-switch step as two sets of launches, one per
// arithmetic policy, over DISJOINT limb rows.  Serialised on one stream each set drains before the other starts, and on small
// batches (one ciphertext = a few dozen workgroup items) each leaves most of the 256 CUs idle.  lanes_t forks the context's
// stream: lane 0 stays on main_stream, lane 1 goes to side_stream, which starts after everything main_stream held at the fork;
// the outermost lanes_t joins the side lane back in its destructor (main waits for an event recorded on side), so the caller
// -- and the allocator, which records release events on main_stream only -- see ONE stream as before.  Nested lanes_t objects
// (a step inside a forked region) only switch lanes: data that stays within one policy's limbs flows in stream order on its
// own lane across steps without a join.  Whatever both lanes need (workspace growth: ensure_ws may synchronise or free) must be
// done BEFORE the fork.  TFHE_LANES=0 keeps everything on one stream (comparisons).
struct lanes_t {
    tfhe_ctx* c;
    bool owner = false, on = false;
    hipStream_t entry = nullptr;
    explicit lanes_t(tfhe_ctx* ctx, bool want = true) : c(ctx) {
        static const bool enabled = env_flag("TFHE_LANES", true);
        entry = c->stream;
        if (!want || !enabled || c->lanes_broken) return;
        if (c->lane_depth > 0) { on = true; c->lane_depth++; return; }
        if (!c->side_stream) {
            bool ok = hipStreamCreate(&c->side_stream) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) == hipSuccess;
            if (!ok) { (void)hipGetLastError(); c->lanes_broken = true; return; }
        }
        if (hipEventRecord(c->ev_fork, c->main_stream) != hipSuccess || hipStreamWaitEvent(c->side_stream, c->ev_fork, 0) != hipSuccess) {
            (void)hipGetLastError();
            c->lanes_broken = true;
            return;
        }
        owner = on = true;
        c->lane_depth = 1;
    }
    // launches that follow go to lane `l` (0 = main, 1 = side); without a fork both are the entry stream
    void use(int l) { if (on) c->stream = l ? c->side_stream : c->main_stream; }
    int join() {   // idempotent; the destructor calls it
        if (!on) return TFHE_OK;
        on = false;
        c->lane_depth--;
        c->stream = entry;
        if (!owner) return TFHE_OK;
        c->stream = c->main_stream;
        hipError_t e = hipEventRecord(c->ev_join, c->side_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->main_stream, c->ev_join, 0);
        if (e != hipSuccess) {   // never leave the side lane unordered: wait for it on the host
            (void)hipGetLastError();
            (void)hipStreamSynchronize(c->side_stream);
            c->lanes_broken = true;
        }
        return TFHE_OK;
    }
    ~lanes_t() { (void)join(); }
    lanes_t(const lanes_t&) = delete;
    lanes_t& operator=(const lanes_t&) = delete;
};

int make_sel(const tfhe_ctx* c, int limbs, const int32_t* idx, limb_sel_t* sel) {
    if (limbs < 1 || limbs > TFHE_MAX_LIMBS) return fail(TFHE_E_BADARG, "limbs=%d out of range [1,%d]", limbs, TFHE_MAX_LIMBS);
    sel->n = limbs;
    for (int j = 0; j < limbs; j++) {
        const int v = idx ? idx[j] : j;
        if (v < 0 || v >= c->L) return fail(TFHE_E_LEVEL_MISMATCH, "limb_idx[%d]=%d outside the ring's %d moduli", j, v, c->L);
        sel->idx[j] = v;
    }
    return TFHE_OK;
}


}  // namespace
#include "launch.h"
namespace {

bool sel_fp(const tfhe_ctx* c, const limb_sel_t& sel, int x) {
    (void)x;  // sub-blocks of N > 2^14 transforms use the same fp64 block kernels (top stages stay u64)
    if (c->variant == 2) return false;
    for (int j = 0; j < sel.n; j++)
        if (!c->limbs_host[sel.idx[j]].Wd) return false;
    return true;
}

// By-value kernel arguments are value-initialised (`T x{}`) throughout: the kernels read named members only, so the padding
// bytes of these structs never matter and none of them needs a memset.
ntt_io_t io_plain() { return ntt_io_t{}; }
// a ring of mixed modulus sizes is split into one pass per arithmetic policy only when there is enough work to pay for the
// second set of launches (a single ciphertext at N = 2^16 is 0.9 M words and stays on the u64 kernels)
static long long mixed_min_words() {   // TFHE_MIXED_MIN_LOG2 overrides (measurements)
    static const long long v = [] { const int l = env_int("TFHE_MIXED_MIN_LOG2", -1); return 1ll << ((l >= 0 && l < 40) ? l : 20); }();
    return v;
}
#define TFHE_MIXED_MIN_WORDS mixed_min_words()

// the first `level` moduli of the ring: a ciphertext's own limbs
limb_sel_t first_limbs(int level) {
    limb_sel_t s{};
    s.n = level;
    for (int j = 0; j < level; j++) s.idx[j] = j;
    return s;
}
// working limbs of a key switch: key limbs 0 .. level-1 (+ the special prime, the key's last limb: downswitch_keyelement,
// modulusraising.jl:43-49)
limb_sel_t working_limbs(int Lk, int level, int special) {
    limb_sel_t w = first_limbs(level);
    if (special) w.idx[w.n++] = Lk - 1;
    return w;
}
// the same with the key's last `n_special` limbs as special primes (the grouped key switch)
limb_sel_t working_limbs_k(int Lk, int level, int n_special) {
    limb_sel_t w = first_limbs(level);
    for (int t = 0; t < n_special; t++) w.idx[w.n++] = Lk - n_special + t;
    return w;
}
ks_arg_t make_ks_arg(int Lk, int level, int special, int polys) {
    ks_arg_t A{};
    A.level = level; A.special = special; A.polys = polys;
    A.w = working_limbs(Lk, level, special);
    A.nw = A.w.n;
    return A;
}
// the row bookkeeping of the key sums of the grouped key switch: `digits` components over the working limbs with n_special special primes
ks_arg_t make_ks_arg_grouped(int Lk, int level, int n_special, int digits, int polys) {
    ks_arg_t A{};
    A.level = digits; A.special = n_special ? 1 : 0; A.polys = polys;
    A.w = working_limbs_k(Lk, level, n_special);
    A.nw = A.w.n;
    return A;
}
// P^-1 mod q_j for j < level, P the special prime (the key's last limb), as Shoup multipliers: the ModulusRaised contraction
void special_inv_table(const tfhe_ctx* c, int Lk, int level, tw_t* out) {
    const u64 P = c->q[Lk - 1];
    for (int j = 0; j < level; j++) out[j] = hostmath::make_tw(hostmath::invmod_prime(P % c->q[j], c->q[j]), c->q[j]);
}

// Per-limb routing masks are 32 bits wide (ntt_io_t::limb_mask, the key-switch kernels' limb_mask); TFHE_MAX_LIMBS is 40
// and the special prime is one of the key's at most 40 limbs (ks_check: level <= Lk - 1 with it), so a key switch has at most
// 40 working limbs -- limb_sel_t::idx holds them all -- and rings with more than 32 selected limbs cannot be split by policy: they
// run whole on the policy that takes every limb (all fp64-size / all narrow: the fast kernels unmasked; otherwise the
// u64 / generic kernels unmasked).
static inline u32 mask_all(int n) { return n >= 32 ? ~0u : ((1u << n) - 1u); }
template <class F>
static inline u32 mask_of(int n, F pred) {  // bit j set where pred(j); for n > 32: all-ones if pred holds everywhere, else 0
    if (n > 32) {
        for (int j = 0; j < n; j++)
            if (!pred(j)) return 0u;
        return ~0u;
    }
    u32 m = 0;
    for (int j = 0; j < n; j++)
        if (pred(j)) m |= 1u << j;
    return m;
}
// how a selection splits between the arithmetic policies: the limbs with fp64 twiddle tables (moduli of fp64 size: the fp64
// transforms), the limbs below 2^52 (the carry-free key sums), and all of them
struct policy_split_t {
    u32 fpmask, narrow, all;
    bool mixed_fp() const { return fpmask != 0 && fpmask != all; }
};
policy_split_t policy_split(const tfhe_ctx* c, const limb_sel_t& sel) {
    policy_split_t p;
    p.fpmask = mask_of(sel.n, [&](int j) { return c->limbs_host[sel.idx[j]].Wd != nullptr; });
    p.narrow = mask_of(sel.n, [&](int j) { return (c->limbs_host[sel.idx[j]].q >> 52) == 0; });
    p.all = mask_all(sel.n);
    return p;
}

// ---- the fused row kernels (row_core.h): what tfhe_mul_relin, tfhe_encrypt, tfhe_decrypt_phase and tfhe_evalkey_gen route alike ----
// the sizes they are built for; the per-policy limb masks hold 32 limbs
bool fused_rows_ok(const tfhe_ctx* c, int limbs) { return c->variant == 0 && c->logN >= 12 && c->logN <= 14 && limbs <= 32; }
// the limbs of `mask` among the first `level`
limb_sel_t limb_subset(int level, u32 mask) {
    limb_sel_t s{};
    for (int j = 0; j < level; j++)
        if ((mask >> j) & 1u) s.idx[s.n++] = j;
    return s;
}
// The two policies side by side over disjoint limb rows, on the context's two lanes when both have limbs: run(policy, mask) for the
// u64 limbs (the long pole) first, on the main lane, then for the fp64-size ones on the side lane.  The lanes join on return.
template <class F>
int both_policies(tfhe_ctx* c, u32 int_mask, u32 fp_mask, F&& run) {
    lanes_t lanes(c, fp_mask != 0 && int_mask != 0);
    lanes.use(0);
    const int rc = run(ArithInt{}, int_mask);
    if (rc) return rc;
    lanes.use(1);
    return run(ArithFp{}, fp_mask);
}
// One launch of persistent workgroups over `items` (item, limb) rows, N = 2^12 .. 2^14: the LDS image is the transform's padded
// row; kernel_for(LOGB) names the kernel, `transforms` is the launch's count for the profile.
template <class K, class... Args>
int launch_fused_rows(tfhe_ctx* c, unsigned items, int64_t transforms, K&& kernel_for, const Args&... args) {
    return dispatch_int<12, 14>(c->logN, [&](auto lb) {
        constexpr int LOGB = decltype(lb)::value, LOGT = logt_for(LOGB);
        const size_t lds = (size_t)lds_words<LOGB, LOGT>() * 8;
        return launch_prof(c, transforms, kernel_for(lb), dim3(persistent_grid(c, items, lds, LOGT)), dim3(1 << LOGT), lds, args...);
    });
}
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

template <class A, int LOGB, int IOMODE = 0>
int launch_block_fwd(tfhe_ctx* c, const u64* src, u64* dst, int64_t rows, const limb_sel_t& sel, int x, const ntt_io_t& io) {
    if constexpr (IOMODE == 0) {
        if (io.mode == 1) return launch_block_fwd<A, LOGB, 1>(c, src, dst, rows, sel, x, io);
    }
    constexpr int LOGT = logt_for(LOGB);
    const size_t lds = (size_t)lds_words<LOGB, LOGT>() * 8;
    const dim3 block(1 << LOGT);
    if constexpr (IOMODE == 1) {
        // digit lift, whole-transform blocks: read each source row once and produce all nw lifted transforms from it
        if (x == 0 && c->variant != 3 && io.nw >= 2 && rows % io.nw == 0) {
            const unsigned litems = (unsigned)(rows / io.nw);
            return launch_prof(c, rows, k_ntt_fwd_lift<A, LOGB, LOGT>, dim3(persistent_grid(c, litems, lds, LOGT)), block, lds, src, dst,
                               c->limbs_dev, sel, litems, io);
        }
    }
    if constexpr (std::is_same<A, ArithFp>::value && LOGB == 14 && IOMODE == 0) {
        if (x == 0 && c->variant == 0 && io.limb_mask == 0)  // next row prefetched into registers under the middle pass: +6 % stand-alone, neutral inside the BFV pipeline
            return launch_prof(c, rows, k_ntt_fwd_pf<A, LOGB, LOGT>, dim3(cu_grid(c, (unsigned)rows)), block, lds, src, dst, c->limbs_dev, sel, (u32)rows);
    }
    const unsigned items = (unsigned)(rows << x);
    return launch_prof(c, rows, k_ntt_fwd_block<A, LOGB, LOGT, IOMODE>, dim3(persistent_grid(c, items, lds, LOGT)), block, lds, src, dst,
                       c->limbs_dev, sel, x, items, io);
}
template <class A, int LOGB, int IOMODE = 0>
int launch_block_inv(tfhe_ctx* c, const u64* src, u64* dst, int64_t rows, const limb_sel_t& sel, int x, const ntt_io_t& io) {
    if constexpr (IOMODE == 0) {
        if (io.mode == 2) return launch_block_inv<A, LOGB, 2>(c, src, dst, rows, sel, x, io);
    }
    constexpr int LOGT = logt_for(LOGB);
    const size_t lds = (size_t)lds_words<LOGB, LOGT>() * 8;
    const dim3 block(1 << LOGT);
    if constexpr (std::is_same<A, ArithFp>::value && LOGB == 14) {
        // whole 2^14 rows in fp64: the staged kernel (next row copied HBM -> LDS under the last pass)
        if (x == 0 && c->variant != 3 && io.limb_mask == 0)
            return launch_prof(c, rows, k_ntt_inv_staged<A, LOGB, LOGT, IOMODE>, dim3(cu_grid(c, (unsigned)rows)), block, lds, src, dst,
                               c->limbs_dev, sel, (u32)rows, io);
    }
    const unsigned items = (unsigned)(rows << x);
    return launch_prof(c, rows, k_ntt_inv_block<A, LOGB, LOGT, IOMODE>, dim3(persistent_grid(c, items, lds, LOGT)), block, lds, src, dst,
                       c->limbs_dev, sel, x, items, io);
}

// sub-blocks of N >= 2^16 rows, two per workgroup (k_ntt_*_subpair); plain I/O, 16-byte aligned rows
template <class A>
int launch_subpair(tfhe_ctx* c, bool inverse, const u64* src, u64* dst, int64_t rows, const limb_sel_t& sel, int x, u32 mask) {
    constexpr int LOGB = 14, LOGT = logt_for(LOGB);
    const size_t lds = (size_t)lds_words<LOGB, LOGT>() * 8;
    const unsigned items = (unsigned)(rows << (x - 1));
    auto kern = inverse ? k_ntt_inv_subpair<A, LOGB, LOGT> : k_ntt_fwd_subpair<A, LOGB, LOGT>;
    return launch_prof(c, rows, kern, dim3(cu_grid(c, items)), dim3(1 << LOGT), lds, src, dst, c->limbs_dev, sel, x, items, mask);
}

int launch_generic(tfhe_ctx* c, bool inverse, const u64* src, u64* dst, int64_t rows, const limb_sel_t& sel, const ntt_io_t& io) {
    const size_t lds = (size_t)c->N * 8;
    const int threads = (int)std::min<int64_t>(1024, std::max<int64_t>(64, c->N / 2));
    return launch_prof(c, rows, inverse ? k_ntt_inv_generic : k_ntt_fwd_generic, dim3((unsigned)rows), dim3(threads), lds, src, dst, c->limbs_dev,
                       sel, c->logN, io);
}

// N > 2^14 with one arithmetic policy (`fp`) for the block stage: x top stages on global memory + 2^14 blocks (needs an
// out-of-place intermediate), or the one-kernel variants of the fp64 policy.  io.limb_mask restricts every kernel of the
// call to those limbs (rings that mix modulus sizes: one call per policy).
int run_ntt_large(tfhe_ctx* c, bool inverse, const u64* src, u64* dst, int64_t rows, const limb_sel_t& sel, const ntt_io_t& io,
                  const ntt_io_t* iop, bool fp, bool wide_lift = false) {
    const int n = c->logN, x = n - 14;
    constexpr int LOGT = logt_for(14);
    const size_t lds = (size_t)lds_words<14, LOGT>() * 8;
    const dim3 block(1 << LOGT);
    const bool pair15 = x == 1 && c->variant == 0 && fp;
    if (iop && x == 1 && !(pair15 && !inverse && io.mode == 1))
        return fail(TFHE_E_UNSUPPORTED, "fused NTT I/O transforms need N <= 2^14 (digit lift: N <= 2^16, fp64 policy)");
    if (pair15) {
        // N = 2^15, fp64 policy: top stage and both 2^14 sub-blocks in one kernel (one read + one write of the row)
        const dim3 grid(cu_grid(c, (unsigned)rows));
        if (inverse) return launch_prof(c, rows, k_ntt_inv_pair<ArithFp, 14, LOGT>, grid, block, lds, src, dst, c->limbs_dev, sel, (u32)rows, io.limb_mask);
        auto pk = io.mode == 1 ? (wide_lift ? k_ntt_fwd_pair<ArithFpWide, 14, LOGT, true> : k_ntt_fwd_pair<ArithFp, 14, LOGT, true>)
                               : k_ntt_fwd_pair<ArithFp, 14, LOGT>;
        return launch_prof(c, rows, pk, grid, block, lds, src, dst, c->limbs_dev, sel, (u32)rows, io);
    }
    if (x > 3) return fail(TFHE_E_UNSUPPORTED, "N = 2^%d not supported (max 2^17)", n);
    // fp64 policy: two sub-blocks per workgroup (16-byte pieces on the natural-order side)
    const bool pairable = x >= 2 && c->variant == 0 && fp && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0;
    if (iop && !(pairable && x == 2 && !inverse && io.mode == 1 && src != dst))
        return fail(TFHE_E_UNSUPPORTED, "fused NTT I/O transforms need N <= 2^14 (digit lift: N <= 2^16, fp64 policy)");
    if (!inverse && pairable && x == 2 && src != dst) {
        // N = 2^16 forward in one kernel: top stages folded into the paired sub-block kernel (out of place only: the
        // row's other workgroup reads the same source words)
        auto qk = io.mode == 1 ? (wide_lift ? k_ntt_fwd_quad<ArithFpWide, 14, LOGT, true> : k_ntt_fwd_quad<ArithFp, 14, LOGT, true>)
                               : k_ntt_fwd_quad<ArithFp, 14, LOGT, false>;
        const unsigned items = (unsigned)(rows << 1);
        return launch_prof(c, rows, qk, dim3(cu_grid(c, items)), block, lds, src, dst, c->limbs_dev, sel, items, io);
    }
    // There is no one-kernel inverse with the sub-blocks FIRST (one row per workgroup pass, sub-block results parked in a
    // per-workgroup scratch row, top stages on the thread's own columns).  MEASURED (r03, 512 polys x 7 limbs of 50 bits): 1.75 TB/s
    // against 1.98 for the two-kernel path below (1.64 with device-scope atomic loads of the parked words instead of an
    // L1-invalidating acquire fence; 1.14 with a release fence, which writes the L2 back) -- one 512-thread workgroup per CU runs
    // its load, four sub-block transforms, parking, read-back, top stages and stores strictly one after the other, where the
    // two-kernel path has two workgroups per row in flight and streaming kernels around them (profiles/LOG.md r03).
    // N = 2^16 inverse, out of place, in ONE pass (k_ntt_inv_quad2: the two top stages first, r04): 2 N 8 bytes per row instead of
    // the 4 N 8 of the sub-block kernel + k_ntt_inv_top<2> below; TFHE_INV_I2=0 keeps the two-kernel path (comparisons)
    static const bool inv_i2 = env_flag("TFHE_INV_I2", true);
    if (inverse && pairable && x == 2 && !iop && src != dst && inv_i2) {
        const unsigned items = (unsigned)(rows << 1);
        return launch_prof(c, rows, k_ntt_inv_quad2<ArithFp, 14, LOGT>, dim3(cu_grid(c, items)), block, lds, src, dst, c->limbs_dev, sel, items, io.limb_mask);
    }
    void* tmp = nullptr;
    int rc = ws_scratch(c, (size_t)rows * c->N * 8, &tmp);
    if (rc) return rc;
    u64* t = (u64*)tmp;
    const dim3 tg((unsigned)((((c->N >> x) + 255) / 256) * rows));
    if (!inverse) {
        rc = dispatch_int<1, 3>(x, [&](auto xc) {
            return launch_prof(c, 0, k_ntt_fwd_top<decltype(xc)::value>, tg, dim3(256), 0, src, t, c->limbs_dev, sel, n, io.limb_mask);
        });
        if (rc) return rc;
        if (pairable) return launch_subpair<ArithFp>(c, false, t, dst, rows, sel, x, io.limb_mask);
        return fp ? launch_block_fwd<ArithFp, 14>(c, t, dst, rows, sel, x, io) : launch_block_fwd<ArithInt, 14>(c, t, dst, rows, sel, x, io);
    }
    if (pairable) rc = launch_subpair<ArithFp>(c, true, src, t, rows, sel, x, io.limb_mask);
    else rc = fp ? launch_block_inv<ArithFp, 14>(c, src, t, rows, sel, x, io) : launch_block_inv<ArithInt, 14>(c, src, t, rows, sel, x, io);
    if (rc) return rc;
    return dispatch_int<1, 3>(x, [&](auto xc) {
        return launch_prof(c, 0, k_ntt_inv_top<decltype(xc)::value>, tg, dim3(256), 0, t, dst, c->limbs_dev, sel, n, io.limb_mask);
    });
}

// forward / inverse transform of `rows` limb-polynomials; src == dst allowed
// `io` (optional) selects the fused global-I/O transforms of ntt_io_t; only for N <= 2^14 (single-block transforms)
int run_ntt(tfhe_ctx* c, bool inverse, const u64* src, u64* dst, int64_t rows, const limb_sel_t& sel, const ntt_io_t* iop = nullptr) {
    if (rows == 0) return TFHE_OK;
    const ntt_io_t io = iop ? *iop : io_plain();
    if (rows < 0 || (rows << std::max(0, c->logN - 14)) > 0x7fffffffll) return fail(TFHE_E_BADARG, "bad polynomial count");
    const int n = c->logN;
    const bool use_block = (c->variant != 1 && n >= 10) || n > 14;
    if (!use_block) return launch_generic(c, inverse, src, dst, rows, sel, io);
    // a ring that mixes fp64-size moduli with larger ones (60-bit q0 / special prime next to 40-bit primes): one launch (N > 2^14:
    // one pass) per policy, each taking its limbs (ntt_io_t::limb_mask)
    const policy_split_t ps = policy_split(c, sel);
    ntt_io_t a = io, b = io;
    a.limb_mask = ps.fpmask;
    b.limb_mask = ps.all & ~ps.fpmask;
    const bool enough = sel.n <= 32 && ps.mixed_fp() && (rows << n) >= TFHE_MIXED_MIN_WORDS;
    if (n <= 14) {
        const bool fp = sel_fp(c, sel, 0);
        if (!fp && c->variant == 0 && enough && (io.mode != 1 || n >= 12)) {
            // the two policies side by side (lanes_t): the u64 launches -- the long pole -- first, on the main lane
            lanes_t lanes(c);
            if (io.mode == 1) {
                // (digit-lift mode: the mask is on the TARGET limb j of item (b, i, j); the fp64 lift takes source limbs of either
                // size through ArithFpWide, instantiated for N >= 2^12)
                return dispatch_int<12, 14>(n, [&](auto lb) {
                    constexpr int LB = decltype(lb)::value;
                    lanes.use(0);
                    const int rc1 = launch_block_fwd<ArithInt, LB, 1>(c, src, dst, rows, sel, 0, b);
                    if (rc1) return rc1;
                    lanes.use(1);
                    return launch_block_fwd<ArithFpWide, LB, 1>(c, src, dst, rows, sel, 0, a);
                });
            }
            return dispatch_int<10, 14>(n, [&](auto lb) {
                constexpr int LB = decltype(lb)::value;
                lanes.use(0);
                const int rc1 = inverse ? launch_block_inv<ArithInt, LB>(c, src, dst, rows, sel, 0, b) : launch_block_fwd<ArithInt, LB>(c, src, dst, rows, sel, 0, b);
                if (rc1) return rc1;
                lanes.use(1);
                return inverse ? launch_block_inv<ArithFp, LB>(c, src, dst, rows, sel, 0, a) : launch_block_fwd<ArithFp, LB>(c, src, dst, rows, sel, 0, a);
            });
        }
        return dispatch_int<10, 14>(n, [&](auto lb) {
            constexpr int LB = decltype(lb)::value;
            if (fp) return inverse ? launch_block_inv<ArithFp, LB>(c, src, dst, rows, sel, 0, io) : launch_block_fwd<ArithFp, LB>(c, src, dst, rows, sel, 0, io);
            return inverse ? launch_block_inv<ArithInt, LB>(c, src, dst, rows, sel, 0, io) : launch_block_fwd<ArithInt, LB>(c, src, dst, rows, sel, 0, io);
        });
    }
    // N > 2^14
    if (!iop && c->variant == 0 && enough) {
        // the transform scratch of both policies (disjoint rows of it) is sized before the fork: growing it synchronises
        void* tmp = nullptr;
        int rc1 = ws_scratch(c, (size_t)rows * c->N * 8, &tmp);
        if (rc1) return rc1;
        lanes_t lanes(c);
        // (which policy is enqueued first makes no difference: TFHE_LANE_FP_FIRST A/B, profiles/r06b_lane_order_ab.txt)
        lanes.use(0);   // the u64 launches (top stages + block kernel: the long pole) first, on the main lane
        rc1 = run_ntt_large(c, inverse, src, dst, rows, sel, b, nullptr, false);
        if (rc1) return rc1;
        lanes.use(1);
        return run_ntt_large(c, inverse, src, dst, rows, sel, a, nullptr, true);
    }
    return run_ntt_large(c, inverse, src, dst, rows, sel, io, iop, sel_fp(c, sel, n - 14));
}


bool bfv_core_fusable(const tfhe_ctx* c, const limb_sel_t& sel) { return c->variant == 0 && c->logN >= 12 && c->logN <= 14 && sel_fp(c, sel, 0); }
// forward transforms + tensor + inverse transforms of one BFV multiplication chunk in one kernel (fp64 policy, N = 2^12 .. 2^14:
// the reference's own BFV tests run at 2^11 - 2^12, test/bfv_crt.jl:8, and its MNIST parameters at 2^13, infer.jl:97);
// *done = false when the configuration is not covered.  scratch: one row per workgroup.  limbs: the limb table the kernel reads
// (nullptr: the context's; the BFV plan passes its copy with the contraction's input constants folded in, bfv_api.inc).
int launch_bfv_core_fused(tfhe_ctx* c, const u64* Ea, const u64* Eb, u64* T, u64* scratch, int64_t nct, const limb_sel_t& sel, bool* done,
                          const core_alt_t* altp = nullptr, bool out_double = false, const ntt_limb_t* limbs = nullptr) {
    *done = false;
    if (!bfv_core_fusable(c, sel) || nct * sel.n > 0x7fffffffll) return TFHE_OK;
    core_alt_t alt{};
    if (altp) alt = *altp;
    const unsigned items = (unsigned)(nct * sel.n);
    const int rc = dispatch_int<12, 14>(c->logN, [&](auto lb) {
        constexpr int LOGB = decltype(lb)::value, LOGT = logt_for(LOGB);
        auto kern = out_double ? k_bfv_core_fused<ArithFp, LOGB, LOGT, true> : k_bfv_core_fused<ArithFp, LOGB, LOGT, false>;
        // one 512-thread workgroup fills a CU at 2^14; the 256-thread workgroups of the smaller rings leave room for a second one
        const unsigned grid = cu_grid(c, items, LOGB == 14 ? 1u : 2u);
        // limb transforms inside this launch: 4 forward + 3 inverse per item
        return launch_prof(c, (int64_t)items * 7, kern, dim3(grid), dim3(1 << LOGT), fused_lds_bytes<LOGB, LOGT>(), Ea, Eb, T, scratch,
                           limbs ? limbs : c->limbs_dev, sel, items, alt);
    });
    if (rc) return rc;
    *done = true;
    return TFHE_OK;
}

template <int OP>
int run_pointwise(tfhe_ctx* c, const u64* a, const u64* b, const u64* acc, u64* dst, int64_t count, int limbs,
                  const int32_t* idx, const scal_arg_t* sc) {
    if (!c) return fail(TFHE_E_BADARG, "null context");
    limb_sel_t sel;
    int rc = make_sel(c, limbs, idx, &sel);
    if (rc) return rc;
    if (count == 0) return TFHE_OK;
    if (count < 0 || count * limbs > 0x7fffffffll) return fail(TFHE_E_BADARG, "bad polynomial count");
    const scal_arg_t s0{};
    return launch(c, k_pointwise<OP>, row_grid((unsigned)(count * limbs), (size_t)c->N), dim3(256), 0, a, b, acc, dst, c->limbs_dev, sel,
                  sc ? *sc : s0, (u32)c->N);
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* tfhe_last_error(void) { return g_err.c_str(); }

int tfhe_device_count(int* n) {
    if (!n) return fail(TFHE_E_BADARG, "null out pointer");
    hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) { *n = 0; return fail(TFHE_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    return TFHE_OK;
}
int tfhe_set_device(int dev) { HIP_TRY(hipSetDevice(dev)); return TFHE_OK; }

int tfhe_ctx_create(int64_t N, int L, const uint64_t* q, const uint64_t* psi, tfhe_ctx** out) {
    using namespace hostmath;
    if (!out) return fail(TFHE_E_BADARG, "null out pointer");
    *out = nullptr;
    if (N < 2 || (N & (N - 1)) || N > (1 << 17)) return fail(TFHE_E_BADARG, "N=%lld must be a power of two in [2, 2^17]", (long long)N);
    if (L < 1 || L > TFHE_MAX_LIMBS || !q) return fail(TFHE_E_BADARG, "L=%d out of range [1,%d]", L, TFHE_MAX_LIMBS);
    int logN = 0;
    while ((1ll << logN) < N) logN++;
    for (int l = 0; l < L; l++) {
        if (q[l] < 3 || q[l] >= (1ull << 62) || !is_prime(q[l])) return fail(TFHE_E_BADARG, "q[%d]=%llu is not a prime below 2^62", l, (unsigned long long)q[l]);
        if ((q[l] - 1) % (2 * (u64)N)) return fail(TFHE_E_BADARG, "q[%d]=%llu: 2N does not divide q-1 (no 2N-th root of unity; the reference's naive ψ=0 path is host-only)", l, (unsigned long long)q[l]);
        for (int m = 0; m < l; m++)
            if (q[m] == q[l]) return fail(TFHE_E_BADARG, "q[%d] repeats q[%d]", l, m);
    }
    tfhe_ctx* c = new tfhe_ctx();
    c->N = N; c->logN = logN; c->L = L;
    c->q.assign(q, q + L);
    c->psi.resize(L);
    c->limbs_host.resize(L);
    ntt_host_tabs_t HT;
    auto up = [&](const void* host, size_t bytes, const void** dev) -> bool {
        if (!host || !bytes) { *dev = nullptr; return true; }
        void* d = nullptr;
        if (devalloc::malloc_retry(&d, bytes) != hipSuccess) return false;
        c->tabs.push_back(d);
        if (hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return false;
        *dev = d;
        return true;
    };
    for (int l = 0; l < L; l++) {
        const u64 ql = q[l];
        u64 p = (psi && psi[l]) ? psi[l] : minimal_primitive_root(ql, 2 * (u64)N);
        ntt_limb_t& LL = c->limbs_host[l];
        if (build_ntt_tables_all(N, ql, p, HT, &LL) != 0) {  // pow2_cyc_rings.jl:31,61 (+ primitivity: psi^N == -1)
            tfhe_ctx_destroy(c);
            return fail(TFHE_E_BADARG, "psi[%d]=%llu is not a primitive 2N-th root of unity mod q[%d]", l, (unsigned long long)p, l);
        }
        c->psi[l] = p;
        const size_t tb = (size_t)N * sizeof(twd_t), fb = (size_t)N * sizeof(ftwd_t);
        bool ok = up(HT.W.data(), tb, (const void**)&LL.W) && up(HT.Wi.data(), tb, (const void**)&LL.Winv) &&
                  up(LL.Wb ? HT.Wb.data() : nullptr, tb, (const void**)&LL.Wb) && up(LL.Winvb ? HT.Wib.data() : nullptr, tb, (const void**)&LL.Winvb) &&
                  up(LL.Wd ? HT.Wd.data() : nullptr, fb, (const void**)&LL.Wd) && up(LL.Winvd ? HT.Wid.data() : nullptr, fb, (const void**)&LL.Winvd) &&
                  up(LL.Wdb ? HT.Wdb.data() : nullptr, fb, (const void**)&LL.Wdb) && up(LL.Winvdb ? HT.Widb.data() : nullptr, fb, (const void**)&LL.Winvdb) &&
                  up(LL.i2_t0 ? HT.I2t0.data() : nullptr, HT.I2t0.size() * sizeof(ftwd_t), (const void**)&LL.i2_t0) &&
                  up(LL.i2_winvb ? HT.I2wib.data() : nullptr, HT.I2wib.size() * sizeof(ftwd_t), (const void**)&LL.i2_winvb);
        if (!ok) {
            tfhe_ctx_destroy(c);
            return fail(TFHE_E_HIP, "allocating the twiddle tables failed (no usable HIP device?)");
        }
    }
    if (devalloc::malloc_retry(&c->limbs_dev, L * sizeof(ntt_limb_t)) != hipSuccess) { tfhe_ctx_destroy(c); return fail(TFHE_E_HIP, "hipMalloc failed"); }
    hipMemcpy(c->limbs_dev, c->limbs_host.data(), L * sizeof(ntt_limb_t), hipMemcpyHostToDevice);
    if (hipStreamCreate(&c->stream) != hipSuccess) { tfhe_ctx_destroy(c); return fail(TFHE_E_HIP, "hipStreamCreate failed"); }
    {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            c->num_cus = cus;
    }
    c->own_stream = true;
    c->main_stream = c->stream;
    devalloc::register_stream(&c->main_stream);
    *out = c;
    return TFHE_OK;
}

int tfhe_ctx_destroy(tfhe_ctx* c) {
    if (!c) return TFHE_OK;
    // Drain BEFORE the allocator forgets the stream: while work is still queued here another thread may tfhe_free a buffer that
    // work reads (its call has returned, so the free is legal), and only a release event recorded on this stream keeps the block
    // from the next tfhe_malloc.  Once both streams are empty nothing of this context can touch a block any more.
    if (c->main_stream) hipStreamSynchronize(c->main_stream);
    if (c->side_stream) hipStreamSynchronize(c->side_stream);
    devalloc::unregister_stream(&c->main_stream);
    if (c->side_stream) hipStreamDestroy(c->side_stream);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    c->stream = c->main_stream;
    for (auto* t : c->tabs) hipFree(t);
    for (auto* t : c->ksw_allocs) hipFree(t);
    if (c->limbs_dev) hipFree(c->limbs_dev);
    if (c->ws) { if (c->ws_pooled) (void)devalloc::release(c->ws); else hipFree(c->ws); }
    if (c->zero_row) hipFree(c->zero_row);
    for (auto& p : c->prof_pairs) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;
    return TFHE_OK;
}

int tfhe_ctx_psi(const tfhe_ctx* c, uint64_t* out) {
    if (!c || !out) return fail(TFHE_E_BADARG, "null argument");
    memcpy(out, c->psi.data(), c->L * 8);
    return TFHE_OK;
}
int tfhe_ctx_set_stream(tfhe_ctx* c, void* s) {
    if (!c) return fail(TFHE_E_BADARG, "null context");
    if (c->stream) HIP_TRY(hipStreamSynchronize(c->stream));
    hipStream_t old = c->own_stream ? c->stream : nullptr, fresh = (hipStream_t)s;
    if (!s) HIP_TRY(hipStreamCreate(&fresh));
    devalloc::set_stream(&c->main_stream, fresh);                  // the allocator reads the slot under its mutex (tfhe_free)
    c->stream = fresh;
    c->own_stream = (s == nullptr);
    if (old) hipStreamDestroy(old);
    return TFHE_OK;
}
int tfhe_ctx_sync(tfhe_ctx* c) {
    if (!c) return fail(TFHE_E_BADARG, "null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return TFHE_OK;
}
// Work submitted to `c` after this call starts after everything submitted to `producer` before it (one recorded event, no
// host wait): the way two contexts with their own streams hand device buffers to each other.
int tfhe_ctx_wait_for(tfhe_ctx* c, tfhe_ctx* producer) {
    if (!c || !producer) return fail(TFHE_E_BADARG, "null context");
    if (c == producer || c->stream == producer->stream) return TFHE_OK;
    hipEvent_t ev;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, producer->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev, 0);
    hipEventDestroy(ev);  // deferred by the runtime until the event has completed
    if (e != hipSuccess) return fail(TFHE_E_HIP, "tfhe_ctx_wait_for: %s", hipGetErrorString(e));
    return TFHE_OK;
}
int tfhe_ctx_set_ntt_variant(tfhe_ctx* c, int v) {
    if (!c || v < 0 || v > 3) return fail(TFHE_E_BADARG, "variant must be 0, 1, 2 or 3");
    c->variant = v;
    return TFHE_OK;
}
int tfhe_ctx_set_chunk(tfhe_ctx* c, int chunk) {
    if (chunk < 0) return fail(TFHE_E_BADARG, "chunk cap must be >= 0 (0 = default), got %d", chunk);
    if (!c) return fail(TFHE_E_BADARG, "null context");
    c->chunk_cap = chunk;
    return TFHE_OK;
}
int tfhe_ctx_workspace(const tfhe_ctx* c, void** ptr, size_t* bytes) {
    if (!c || !ptr || !bytes) return fail(TFHE_E_BADARG, "null argument");
    *ptr = c->ws;
    *bytes = c->ws_bytes;
    return TFHE_OK;
}

int tfhe_malloc(size_t bytes, void** p) {
    if (!p) return fail(TFHE_E_BADARG, "null out pointer");
    hipError_t e = devalloc::alloc(bytes, p);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? TFHE_E_NOMEM : TFHE_E_HIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return TFHE_OK;
}
int tfhe_free(void* p) { if (p) HIP_TRY(devalloc::release(p)); return TFHE_OK; }
int tfhe_alloc_stats(uint64_t* live_bytes, uint64_t* cached_bytes, uint64_t* hip_mallocs, uint64_t* reuses) {
    devalloc::state_t& s = devalloc::S();
    std::lock_guard<std::mutex> g(s.mu);
    if (live_bytes) *live_bytes = s.live_bytes;
    if (cached_bytes) *cached_bytes = s.cached_bytes;
    if (hip_mallocs) *hip_mallocs = (uint64_t)s.n_hip_malloc;
    if (reuses) *reuses = (uint64_t)s.n_reuse;
    return TFHE_OK;
}
int tfhe_alloc_trim(void) {
    devalloc::state_t& s = devalloc::S();
    std::lock_guard<std::mutex> g(s.mu);
    devalloc::trim_locked(s);
    return TFHE_OK;
}
int tfhe_memcpy_h2d(void* d, const void* s, size_t n) { HIP_TRY(hipMemcpy(d, s, n, hipMemcpyHostToDevice)); return TFHE_OK; }
int tfhe_memcpy_d2h(void* d, const void* s, size_t n) { HIP_TRY(hipMemcpy(d, s, n, hipMemcpyDeviceToHost)); return TFHE_OK; }
int tfhe_memcpy_d2d(tfhe_ctx* c, void* d, const void* s, size_t n) {
    if (!c) return fail(TFHE_E_BADARG, "null context");
    HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, c->stream));
    return TFHE_OK;
}
// component p of a packed batch [count][polys][words] <-> a batch of single polynomials [count][words]: one strided copy
int tfhe_pack_poly(tfhe_ctx* c, uint64_t* packed, const uint64_t* src, int polys, int p, size_t words, int64_t count) {
    if (!c || !packed || !src) return fail(TFHE_E_BADARG, "null argument");
    if (polys < 1 || p < 0 || p >= polys || count < 0) return fail(TFHE_E_BADARG, "bad component index");
    if (count == 0 || words == 0) return TFHE_OK;
    HIP_TRY(hipMemcpy2DAsync(packed + (size_t)p * words, (size_t)polys * words * 8, src, words * 8, words * 8, (size_t)count,
                             hipMemcpyDeviceToDevice, c->stream));
    return TFHE_OK;
}
int tfhe_unpack_poly(tfhe_ctx* c, uint64_t* dst, const uint64_t* packed, int polys, int p, size_t words, int64_t count) {
    if (!c || !packed || !dst) return fail(TFHE_E_BADARG, "null argument");
    if (polys < 1 || p < 0 || p >= polys || count < 0) return fail(TFHE_E_BADARG, "bad component index");
    if (count == 0 || words == 0) return TFHE_OK;
    HIP_TRY(hipMemcpy2DAsync(dst, words * 8, packed + (size_t)p * words, (size_t)polys * words * 8, words * 8, (size_t)count,
                             hipMemcpyDeviceToDevice, c->stream));
    return TFHE_OK;
}
// dst[k][:] = src[:] for k < count: one ring element (a plaintext, a key) broadcast over a batch
__global__ __launch_bounds__(256) void k_broadcast(u64* __restrict__ dst, const u64* __restrict__ src, size_t words) {
    const size_t w = (size_t)blockIdx.x * 512 + threadIdx.x * 2;
    if (w + 1 < words) {
        const ulonglong2 v = *(const ulonglong2*)(src + w);
        *(ulonglong2*)(dst + (size_t)blockIdx.y * words + w) = v;
    } else if (w < words) {
        dst[(size_t)blockIdx.y * words + w] = src[w];
    }
}
int tfhe_broadcast_poly(tfhe_ctx* c, uint64_t* dst, const uint64_t* src, size_t words, int64_t count) {
    if (!c || !dst || !src) return fail(TFHE_E_BADARG, "null argument");
    if (count < 0 || count > 65535 || (words & 1)) return fail(TFHE_E_BADARG, "count must be in [0, 65535], words even");
    if (count == 0 || words == 0) return TFHE_OK;
    return launch(c, k_broadcast, dim3((unsigned)((words + 511) / 512), (unsigned)count), dim3(256), 0, dst, src, words);
}
int tfhe_memset(tfhe_ctx* c, void* d, int byte, size_t n) {
    if (!c) return fail(TFHE_E_BADARG, "null context");
    HIP_TRY(hipMemsetAsync(d, byte, n, c->stream));
    return TFHE_OK;
}

int tfhe_nntt(tfhe_ctx* c, const uint64_t* src, uint64_t* dst, int64_t count, int limbs, const int32_t* idx) {
    if (!c || !src || !dst) return fail(TFHE_E_BADARG, "null argument");
    limb_sel_t sel;
    int rc = make_sel(c, limbs, idx, &sel);
    if (rc) return rc;
    return run_ntt(c, false, src, dst, count * limbs, sel);
}
int tfhe_inntt(tfhe_ctx* c, const uint64_t* src, uint64_t* dst, int64_t count, int limbs, const int32_t* idx) {
    if (!c || !src || !dst) return fail(TFHE_E_BADARG, "null argument");
    limb_sel_t sel;
    int rc = make_sel(c, limbs, idx, &sel);
    if (rc) return rc;
    return run_ntt(c, true, src, dst, count * limbs, sel);
}

int tfhe_add(tfhe_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* d, int64_t n, int l, const int32_t* i) { return run_pointwise<OP_ADD>(c, a, b, nullptr, d, n, l, i, nullptr); }
int tfhe_sub(tfhe_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* d, int64_t n, int l, const int32_t* i) { return run_pointwise<OP_SUB>(c, a, b, nullptr, d, n, l, i, nullptr); }
int tfhe_neg(tfhe_ctx* c, const uint64_t* a, uint64_t* d, int64_t n, int l, const int32_t* i) { return run_pointwise<OP_NEG>(c, a, nullptr, nullptr, d, n, l, i, nullptr); }
int tfhe_mul(tfhe_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* d, int64_t n, int l, const int32_t* i) { return run_pointwise<OP_MUL>(c, a, b, nullptr, d, n, l, i, nullptr); }
int tfhe_mad(tfhe_ctx* c, const uint64_t* acc, const uint64_t* a, const uint64_t* b, uint64_t* d, int64_t n, int l, const int32_t* i) { return run_pointwise<OP_MAD>(c, a, b, acc, d, n, l, i, nullptr); }
int tfhe_scalar_mul(tfhe_ctx* c, const uint64_t* scal, const uint64_t* a, uint64_t* d, int64_t n, int l, const int32_t* idx) {
    if (!c || !scal) return fail(TFHE_E_BADARG, "null argument");
    limb_sel_t sel;
    int rc = make_sel(c, l, idx, &sel);
    if (rc) return rc;
    scal_arg_t sc{};
    for (int j = 0; j < l; j++) { const u64 q = c->q[sel.idx[j]]; sc.s[j] = hostmath::make_tw(scal[j] % q, q); }
    return run_pointwise<OP_SCAL>(c, a, nullptr, nullptr, d, n, l, idx, &sc);
}

int tfhe_dot(tfhe_ctx* c, const uint64_t* acc, const uint64_t* const* a, const uint64_t* const* b, int n_terms, uint64_t* dst,
             int64_t count, int limbs, const int32_t* idx) {
    if (!c || !a || !b || !dst) return fail(TFHE_E_BADARG, "null argument");
    if (n_terms < 1) return fail(TFHE_E_BADARG, "tfhe_dot needs at least one term");
    limb_sel_t sel;
    int rc = make_sel(c, limbs, idx, &sel);
    if (rc) return rc;
    if (count < 0) return fail(TFHE_E_BADARG, "negative count");
    if (count == 0) return TFHE_OK;
    for (int k = 0; k < n_terms; k++)
        if (!a[k] || !b[k]) return fail(TFHE_E_BADARG, "null operand %d", k);
    const u64* running = acc;
    for (int k0 = 0; k0 < n_terms; k0 += TFHE_DOT_MAX) {   // more than 64 terms: further launches accumulate onto dst
        dot_arg_t D;
        D.n = std::min(TFHE_DOT_MAX, n_terms - k0);
        for (int k = 0; k < D.n; k++) { D.a[k] = a[k0 + k]; D.b[k] = b[k0 + k]; }
        rc = launch(c, k_dot, row_grid((unsigned)(count * limbs), (size_t)c->N), dim3(256), 0, D, running, dst, c->limbs_dev, sel, (u32)c->N);
        if (rc) return rc;
        running = dst;
    }
    return TFHE_OK;
}

int tfhe_lincomb(tfhe_ctx* c, const uint64_t* scalars, const uint64_t* const* a, int n_terms, uint64_t* dst, int64_t count, int limbs,
                 const int32_t* idx) {
    if (!c || !scalars || !a || !dst) return fail(TFHE_E_BADARG, "null argument");
    if (n_terms < 1) return fail(TFHE_E_BADARG, "tfhe_lincomb needs at least one term");
    if (n_terms > TFHE_DOT_MAX) return fail(TFHE_E_UNSUPPORTED, "tfhe_lincomb takes at most %d terms per call", TFHE_DOT_MAX);
    limb_sel_t sel;
    int rc = make_sel(c, limbs, idx, &sel);
    if (rc) return rc;
    if (count < 0) return fail(TFHE_E_BADARG, "negative count");
    if (count == 0) return TFHE_OK;
    for (int k = 0; k < n_terms; k++)
        if (!a[k]) return fail(TFHE_E_BADARG, "null operand %d", k);
    std::vector<u64> sc((size_t)n_terms * limbs);
    for (int k = 0; k < n_terms; k++)
        for (int j = 0; j < limbs; j++) {
            const u64 q = c->q[sel.idx[j]], v = scalars[(size_t)k * limbs + j];
            if (v >= q) return fail(TFHE_E_BADARG, "scalar %d, limb %d is not a residue", k, j);
            sc[(size_t)k * limbs + j] = v;
        }
    void* dsc = nullptr;
    hipError_t e = devalloc::alloc(sc.size() * 8, &dsc);
    if (e != hipSuccess) return fail(TFHE_E_NOMEM, "hipMalloc(%zu): %s", sc.size() * 8, hipGetErrorString(e));
    e = hipMemcpyAsync(dsc, sc.data(), sc.size() * 8, hipMemcpyHostToDevice, c->stream);   // pageable source: staged before the call returns
    if (e != hipSuccess) {
        (void)hipGetLastError();
        devalloc::release(dsc);
        return fail(TFHE_E_HIP, "hipMemcpyAsync: %s", hipGetErrorString(e));
    }
    dot_arg_t D;
    D.n = n_terms;
    for (int k = 0; k < n_terms; k++) { D.a[k] = a[k]; D.b[k] = nullptr; }
    rc = launch(c, k_lincomb, row_grid((unsigned)(count * limbs), (size_t)c->N), dim3(256), 0, D, (const u64*)dsc, dst, c->limbs_dev, sel, (u32)c->N);
    devalloc::release(dsc);   // parked until the launch above has run
    return rc;
}

int tfhe_lincomb_many(tfhe_ctx* c, const uint64_t* scalars, const uint64_t* const* a, int n_terms, uint64_t* const* dst, int n_out, int64_t count,
                      int limbs, const int32_t* idx) {
    if (!c || !scalars || !a || !dst) return fail(TFHE_E_BADARG, "null argument");
    if (n_terms < 1 || n_out < 1) return fail(TFHE_E_BADARG, "tfhe_lincomb_many needs at least one term and one output");
    if (n_terms > TFHE_DOT_MAX) return fail(TFHE_E_UNSUPPORTED, "tfhe_lincomb_many takes at most %d terms per call", TFHE_DOT_MAX);
    limb_sel_t sel;
    int rc = make_sel(c, limbs, idx, &sel);
    if (rc) return rc;
    if (count < 0) return fail(TFHE_E_BADARG, "negative count");
    for (int k = 0; k < n_terms; k++)
        if (!a[k]) return fail(TFHE_E_BADARG, "null operand %d", k);
    for (int o = 0; o < n_out; o++)
        if (!dst[o]) return fail(TFHE_E_BADARG, "null output %d", o);
    const size_t per_out = (size_t)n_terms * limbs;
    for (int o = 0; o < n_out; o++)
        for (int k = 0; k < n_terms; k++)
            for (int j = 0; j < limbs; j++)
                if (scalars[(size_t)o * per_out + (size_t)k * limbs + j] >= c->q[sel.idx[j]])
                    return fail(TFHE_E_BADARG, "scalar of output %d, term %d, limb %d is not a residue", o, k, j);
    if (count == 0) return TFHE_OK;
    void* dsc = nullptr;
    hipError_t e = devalloc::alloc((size_t)n_out * per_out * 8, &dsc);
    if (e != hipSuccess) return fail(TFHE_E_NOMEM, "hipMalloc(%zu): %s", (size_t)n_out * per_out * 8, hipGetErrorString(e));
    e = hipMemcpyAsync(dsc, scalars, (size_t)n_out * per_out * 8, hipMemcpyHostToDevice, c->stream);   // pageable source: staged before the call returns
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)devalloc::release(dsc);
        return fail(TFHE_E_HIP, "hipMemcpyAsync: %s", hipGetErrorString(e));
    }
    dot_arg_t D;
    D.n = n_terms;
    for (int k = 0; k < n_terms; k++) { D.a[k] = a[k]; D.b[k] = nullptr; }
    const dim3 grid = row_grid((unsigned)(count * limbs), (size_t)c->N);
    for (int o0 = 0; o0 < n_out && !rc; o0 += 4) {   // four outputs per pass over the operands
        const int no = std::min(4, n_out - o0);
        lincomb_out_t O;
        for (int o = 0; o < 4; o++) O.dst[o] = o < no ? dst[o0 + o] : nullptr;
        const u64* sc = (const u64*)dsc + (size_t)o0 * per_out;
        rc = dispatch_int<1, 4>(no, [&](auto k) {
            return launch(c, k_lincomb_many<decltype(k)::value>, grid, dim3(256), 0, D, sc, O, c->limbs_dev, sel, (u32)c->N);
        });
    }
    devalloc::release(dsc);   // parked until the launches above have run
    return rc;
}

int tfhe_tensor(tfhe_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* out, int64_t batch, int limbs, const int32_t* idx) {
    if (!c || !a || !b || !out) return fail(TFHE_E_BADARG, "null argument");
    limb_sel_t sel;
    int rc = make_sel(c, limbs, idx, &sel);
    if (rc) return rc;
    if (batch == 0) return TFHE_OK;
    return launch(c, k_tensor, row_grid((unsigned)(batch * limbs), (size_t)c->N), dim3(256), 0, a, b, out, c->limbs_dev, sel, (u32)c->N);
}

static int do_rescale(tfhe_ctx* c, const u64* src, u64* dst, int64_t count, const limb_sel_t& sel) {
    if (sel.n < 2) return fail(TFHE_E_LEVEL_MISMATCH, "modswitch needs at least 2 limbs");
    rescale_arg_t ra{};
    const u64 ql = c->q[sel.idx[sel.n - 1]];
    for (int j = 0; j < sel.n - 1; j++) {
        const u64 qj = c->q[sel.idx[j]];
        ra.qlinv[j] = hostmath::make_tw(hostmath::invmod_prime(ql % qj, qj), qj);
    }
    if (count == 0) return TFHE_OK;
    static const bool row_major = env_flag("TFHE_RESCALE_ROWS", false);
    if (!row_major && c->N >= 512 && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {   // coefficient-major: the last limb read once per polynomial
        const unsigned want = (unsigned)((2048 + count - 1) / count), cap = (unsigned)(c->N / 512);
        return launch(c, k_rescale_cm, dim3((unsigned)count, std::max(1u, std::min(want, cap))), dim3(256), 0, src, dst, c->limbs_dev, sel, ra, (u32)c->N);
    }
    return launch(c, k_rescale, row_grid((unsigned)(count * (sel.n - 1)), (size_t)c->N), dim3(256), 0, src, dst, c->limbs_dev, sel, ra, (u32)c->N);
}
int tfhe_rescale(tfhe_ctx* c, const uint64_t* src, uint64_t* dst, int64_t count, int limbs, const int32_t* idx) {
    if (!c || !src || !dst) return fail(TFHE_E_BADARG, "null argument");
    limb_sel_t sel;
    int rc = make_sel(c, limbs, idx, &sel);
    if (rc) return rc;
    return do_rescale(c, src, dst, count, sel);
}

int tfhe_select_limbs(tfhe_ctx* c, const uint64_t* src, uint64_t* dst, int64_t count, int src_limbs, const int32_t* which, int nw) {
    if (!c || !src || !dst || !which) return fail(TFHE_E_BADARG, "null argument");
    if (nw < 1 || nw > TFHE_MAX_LIMBS) return fail(TFHE_E_BADARG, "bad limb count");
    limb_sel_t w;
    w.n = nw;
    for (int j = 0; j < nw; j++) {
        if (which[j] < 0 || which[j] >= src_limbs) return fail(TFHE_E_LEVEL_MISMATCH, "which[%d]=%d outside source limbs", j, which[j]);
        w.idx[j] = which[j];
    }
    if (count == 0) return TFHE_OK;
    return launch(c, k_select, row_grid((unsigned)(count * nw), (size_t)c->N), dim3(256), 0, src, dst, w, src_limbs, (u32)c->N);
}

static int do_galois(tfhe_ctx* c, const u64* src, u64* dst, u64 g, int64_t rows, const limb_sel_t& sel) {
    if ((g & 1) == 0) return fail(TFHE_E_BADARG, "galois element %llu must be odd", (unsigned long long)g);
    if (src == dst) return fail(TFHE_E_BADARG, "tfhe_galois cannot run in place");
    const u64 m = 2 * (u64)c->N;
    g %= m;
    u64 ginv = 1;  // inverse modulo 2N by Newton iteration (g odd)
    for (int i = 0; i < 6; i++) ginv = (ginv * (2 - g * ginv)) & (m - 1);
    if (rows == 0) return TFHE_OK;
    if (c->variant == 0 && c->logN >= 11 && c->logN <= 14 && rows >= (int64_t)c->num_cus / 2 && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
        // rows that fit the LDS, enough of them to fill the chip: scatter through the LDS, coalesced on both sides
        constexpr int T = 512;
        const size_t lds = (size_t)c->N * 8;
        const unsigned per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(4, (size_t)(160 * 1024) / lds));
        const unsigned grid = (unsigned)std::min<int64_t>(rows, (int64_t)c->num_cus * per_cu);
        return launch(c, k_galois_lds<T>, dim3(grid), dim3(T), lds, src, dst, c->limbs_dev, sel, g, (u32)c->N, (u32)rows);
    }
    if (c->variant == 0 && c->logN >= 15 && rows % sel.n == 0 && rows / sel.n >= 16) {
        // whole polynomials, enough of them: the XCD-cooperative scatter (k_galois_xcd)
        return launch(c, k_galois_xcd, dim3(8 * TFHE_ROT_TAIL_SLOTS), dim3(256), 0, src, dst, c->limbs_dev, sel, g, (u32)c->N, (u32)(rows / sel.n));
    }
    return launch(c, k_galois, row_grid((unsigned)rows, (size_t)c->N), dim3(256), 0, src, dst, c->limbs_dev, sel, ginv, (u32)c->N);
}
int tfhe_galois(tfhe_ctx* c, const uint64_t* src, uint64_t* dst, uint64_t g, int64_t count, int limbs, const int32_t* idx) {
    if (!c || !src || !dst) return fail(TFHE_E_BADARG, "null argument");
    limb_sel_t sel;
    int rc = make_sel(c, limbs, idx, &sel);
    if (rc) return rc;
    return do_galois(c, src, dst, g, count * limbs, sel);
}

#include "ks_api.inc"
#include "md_api.inc"

// ---- CKKS encode / decode (float; ckksencoding.jl:56-97, ckks.jl:35-59) -------------------------------------------
static int ckks_tables(tfhe_ctx* c) {
    std::lock_guard<std::mutex> g(c->ksw_mu);
    if (c->ckks_roots) return TFHE_OK;
    const size_t n = (size_t)c->N, n2 = n / 2;
    const int logn = c->logN;
    std::vector<double> roots(n2 * 2 + 2), tw(n * 2);
    for (size_t t = 0; t < n2; t++) {
        const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)t / (long double)n;
        roots[2 * t] = (double)cosl(a);
        roots[2 * t + 1] = (double)sinl(a);
    }
    for (size_t k = 0; k < n; k++) {
        // ckksencoding.jl:84: the angle 2k/(2N)*pi is evaluated in Float64 first, then exponentiated
        const double ang = ((double)(2 * k) / (double)(2 * n)) * 3.14159265358979323846;
        tw[2 * k] = cos(ang);
        tw[2 * k + 1] = sin(ang);
    }
    auto brev = [&](u32 x) { u32 r = 0; for (int i = 0; i < logn; i++) r |= ((x >> i) & 1u) << (logn - 1 - i); return r; };
    std::vector<u32> pos(2 * n2), gpos(n2);
    const u64 M = 2 * n;
    u64 e = 1;
    for (size_t i = 0; i < n2; i++) {
        e = (e * 3) % M;                       // 3^(i+1) mod 2N   (ZmstarPermutation, ckksencoding.jl:49-54)
        pos[2 * i] = brev((u32)(e >> 1));
        pos[2 * i + 1] = brev((u32)(((M - e) % M) >> 1));
        gpos[i] = brev((u32)(e >> 1));
    }
    auto up = [&](const void* h, size_t bytes, void** d) -> bool {
        if (devalloc::malloc_retry(d, bytes ? bytes : 8) != hipSuccess) return false;
        c->ksw_allocs.push_back(*d);
        return hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
    };
    void *r = nullptr, *t = nullptr, *p = nullptr, *gp = nullptr;
    if (!up(roots.data(), (n2 ? n2 : 1) * 16, &r) || !up(tw.data(), n * 16, &t) || !up(pos.data(), pos.size() * 4, &p) ||
        !up(gpos.data(), gpos.size() * 4, &gp))
        return fail(TFHE_E_NOMEM, "allocating the CKKS tables failed");
    c->ckks_tw = t; c->ckks_pos = p; c->ckks_gpos = gp; c->ckks_roots = r;
    return TFHE_OK;
}
static int ckks_check(tfhe_ctx* c, int level, uint64_t smant, const void* a, const void* b, int64_t batch) {
    if (!c || !a || !b) return fail(TFHE_E_BADARG, "null argument");
    if (level < 1 || level > c->L) return fail(TFHE_E_LEVEL_MISMATCH, "level=%d outside [1,%d]", level, c->L);
    if (smant == 0) return fail(TFHE_E_BADARG, "scale must be positive");
    if (c->N < 4) return fail(TFHE_E_UNSUPPORTED, "CKKS encoding needs N >= 4");
    if (batch < 0) return fail(TFHE_E_BADARG, "negative batch");
    return TFHE_OK;
}
static int ckks_fft(tfhe_ctx* c, cplx_t* buf, int64_t nb, bool dif, bool conj_roots) {
    const u32 n = (u32)c->N;
    const dim3 grid((n / 2 + 255) / 256, (unsigned)nb);
    int rc = TFHE_OK;
    if (dif) for (u32 h = n / 2; h >= 1 && !rc; h >>= 1) rc = launch(c, k_fft_pass, grid, dim3(256), 0, buf, (const cplx_t*)c->ckks_roots, n, h, 1, conj_roots ? 1 : 0);
    else for (u32 h = 1; h < n && !rc; h <<= 1) rc = launch(c, k_fft_pass, grid, dim3(256), 0, buf, (const cplx_t*)c->ckks_roots, n, h, 0, conj_roots ? 1 : 0);
    return rc;
}

int tfhe_ckks_encode(tfhe_ctx* c, int level, uint64_t scale_mant, int scale_exp2, const double* slots, uint64_t* out, int64_t batch) {
    int rc = ckks_check(c, level, scale_mant, slots, out, batch);
    if (rc || batch == 0) return rc;
    rc = ckks_tables(c);
    if (rc) return rc;
    const u32 n = (u32)c->N;
    const limb_sel_t sel = first_limbs(level);
    const int64_t chunk = chunk_of(c, batch, 4096);
    void* ws = nullptr;
    rc = ensure_ws(c, (size_t)chunk * n * 16, &ws);
    if (rc) return rc;
    cplx_t* buf = (cplx_t*)ws;
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        rc = launch(c, k_ckks_scatter, dim3((n / 2 + 255) / 256, (unsigned)nb), dim3(256), 0, (const cplx_t*)slots + (size_t)b0 * (n / 2), buf,
                    (const u32*)c->ckks_pos, n);
        if (rc) return rc;
        rc = ckks_fft(c, buf, nb, false, true);  // inverse transform: conjugate roots, 1/N applied below
        if (rc) return rc;
        rc = launch(c, k_ckks_encode_finish, dim3((n + 255) / 256, (unsigned)nb), dim3(256), 0, buf, (const cplx_t*)c->ckks_tw,
                    out + (size_t)b0 * level * n, c->limbs_dev, sel, scale_mant, scale_exp2, n);
        if (rc) return rc;
    }
    return TFHE_OK;
}

int tfhe_ckks_decode(tfhe_ctx* c, int level, uint64_t scale_mant, int scale_exp2, const uint64_t* in, double* slots, int64_t batch) {
    int rc = ckks_check(c, level, scale_mant, in, slots, batch);
    if (rc || batch == 0) return rc;
    rc = ckks_tables(c);
    if (rc) return rc;
    const conv_tab_t* T = nullptr;
    rc = ksw_table(c, level, &T);
    if (rc) return rc;
    const u32 n = (u32)c->N;
    const int64_t chunk = chunk_of(c, batch, 4096);
    void* ws = nullptr;
    rc = ensure_ws(c, (size_t)chunk * n * 16, &ws);
    if (rc) return rc;
    cplx_t* buf = (cplx_t*)ws;
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        rc = launch(c, k_ckks_decode_start, dim3((n + 255) / 256, (unsigned)nb), dim3(256), 0, in + (size_t)b0 * level * n, buf,
                    (const cplx_t*)c->ckks_tw, T, level, c->q[0], scale_mant, scale_exp2, n);
        if (rc) return rc;
        rc = ckks_fft(c, buf, nb, true, false);
        if (rc) return rc;
        rc = launch(c, k_ckks_gather, dim3((n / 2 + 255) / 256, (unsigned)nb), dim3(256), 0, buf, (cplx_t*)slots + (size_t)b0 * (n / 2),
                    (const u32*)c->ckks_gpos, n);
        if (rc) return rc;
    }
    return TFHE_OK;
}

// ---- device-side samplers (poly.jl:7-23, crt.jl:277-279; stream definition in sample_kernels.h) --------------------------
int tfhe_sample_uniform(tfhe_ctx* c, int level, uint64_t seed, uint32_t stream, uint64_t first_poly, uint64_t* out, int64_t count) {
    if (!c || !out) return fail(TFHE_E_BADARG, "null argument");
    if (level < 1 || level > c->L) return fail(TFHE_E_LEVEL_MISMATCH, "level=%d outside [1,%d]", level, c->L);
    if (count < 0) return fail(TFHE_E_BADARG, "negative count");
    if (first_poly + (u64)count > (1ull << 32)) return fail(TFHE_E_BADARG, "polynomial counter exceeds 2^32");
    const u32 n = (u32)c->N;
    const int64_t chunk = chunk_of(c, count, 32768);   // polynomials per launch (grid dimension z / y)
    for (int64_t p0 = 0; p0 < count; p0 += chunk) {
        const unsigned np = (unsigned)std::min<int64_t>(chunk, count - p0);
        const int rc = launch(c, k_sample_uniform, dim3((n + 255) / 256, (unsigned)level, np), dim3(256), 0, out + (size_t)p0 * level * n,
                              c->limbs_dev, level, seed, stream, n, first_poly + (u64)p0);
        if (rc) return rc;
    }
    return TFHE_OK;
}
int tfhe_sample_gaussian(tfhe_ctx* c, int level, double sigma, uint64_t multiplier, uint64_t seed, uint32_t stream, uint64_t first_poly,
                         uint64_t* out, int64_t count) {
    if (!c || !out) return fail(TFHE_E_BADARG, "null argument");
    if (level < 1 || level > c->L) return fail(TFHE_E_LEVEL_MISMATCH, "level=%d outside [1,%d]", level, c->L);
    if (!(sigma >= 0) || sigma > 1e15) return fail(TFHE_E_BADARG, "sigma out of range");
    if (count < 0) return fail(TFHE_E_BADARG, "negative count");
    if (first_poly + (u64)count > (1ull << 32)) return fail(TFHE_E_BADARG, "polynomial counter exceeds 2^32");
    const u32 n = (u32)c->N;
    const int64_t chunk = chunk_of(c, count, 32768);   // polynomials per launch (grid dimension z / y)
    for (int64_t p0 = 0; p0 < count; p0 += chunk) {
        const unsigned np = (unsigned)std::min<int64_t>(chunk, count - p0);
        const int rc = launch(c, k_sample_gaussian, dim3((n + 255) / 256, np), dim3(256), 0, out + (size_t)p0 * level * n, c->limbs_dev,
                              level, sigma, multiplier, seed, stream, n, first_poly + (u64)p0);
        if (rc) return rc;
    }
    return TFHE_OK;
}

// ---- profiling / events ---------------------------------------------------------------------------
int tfhe_prof_enable(tfhe_ctx* c, int on) {
    if (!c) return fail(TFHE_E_BADARG, "null context");
    c->prof = on != 0;
    return TFHE_OK;
}
int tfhe_prof_read(tfhe_ctx* c, int64_t* launches, int64_t* limb_polys, double* total_ms) {
    if (!c) return fail(TFHE_E_BADARG, "null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    int64_t nl = 0, np = 0;
    double ms = 0;
    for (auto& p : c->prof_pairs) {
        float t = 0;
        hipEventElapsedTime(&t, p.a, p.b);
        if (p.limb_polys > 0) { nl++; np += p.limb_polys; ms += t; }
        hipEventDestroy(p.a);
        hipEventDestroy(p.b);
    }
    c->prof_pairs.clear();
    if (launches) *launches = nl;
    if (limb_polys) *limb_polys = np;
    if (total_ms) *total_ms = ms;
    return TFHE_OK;
}
int tfhe_event_create(void** ev) {
    if (!ev) return fail(TFHE_E_BADARG, "null out pointer");
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    *ev = (void*)e;
    return TFHE_OK;
}
int tfhe_event_destroy(void* ev) { if (ev) HIP_TRY(hipEventDestroy((hipEvent_t)ev)); return TFHE_OK; }
int tfhe_event_record(tfhe_ctx* c, void* ev) {
    if (!c || !ev) return fail(TFHE_E_BADARG, "null argument");
    HIP_TRY(hipEventRecord((hipEvent_t)ev, c->stream));
    return TFHE_OK;
}
int tfhe_event_elapsed_ms(void* a, void* b, float* ms) {
    if (!a || !b || !ms) return fail(TFHE_E_BADARG, "null argument");
    HIP_TRY(hipEventSynchronize((hipEvent_t)b));
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
    return TFHE_OK;
}

}  // extern "C"

#include "bfv_api.inc"
#include "comm_api.inc"
#include "plain_api.inc"
#include "mul_api.inc"
#include "enc_api.inc"
#include "keygen_api.inc"
#include "dot_api.inc"
