"""The child process of tests/test_gpu_threads.py: `python tests/gpu_threads_child.py SCENARIO` runs ONE scenario of the threading contract
(include/toyfhe_hip.h, "threading") on the device and prints one JSON line; the test asserts on it.  A fresh process per scenario: the
first-use paths are really first uses, the allocator's thresholds come from the environment, and a deadlock ends as a killed child.
At most 8 threads, all daemons, every join with a timeout (a join that times out ends the process at once, exit status 3).

All comparisons are bit-exact: against the same calls made serially in this process, and against oracle.ref_cpu for item 0 of a batch.
N = 2^12 throughout.  ctypes releases the GIL for the length of every call, so the library calls of different threads overlap."""
import ctypes as C
import json
import os
import queue
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import helpers as H
from tests.matmul_oracle import matmul_diag_ref, rotate as ref_rotate

N = 1 << 12
JOIN_S = 150
L = tf.native.lib()
ck = tf.native.check


def malloc(nbytes):
    p = C.c_void_p()
    ck(L.tfhe_malloc(nbytes, C.byref(p)))
    return p.value


def free(p):
    ck(L.tfhe_free(p))


def upload(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    p = malloc(a.nbytes)
    ck(L.tfhe_memcpy_h2d(p, a.ctypes.data, a.nbytes))
    return p


def download(p, shape):
    out = np.empty(shape, dtype=np.uint64)
    ck(L.tfhe_memcpy_d2h(out.ctypes.data, p, out.nbytes))
    return out


def last_error():
    return L.tfhe_last_error().decode("utf-8", "replace")


def join_all(threads):
    for t in threads:
        t.join(JOIN_S)
        if t.is_alive():
            print(json.dumps({"ok": False, "why": "thread %s did not finish in %d s" % (t.name, JOIN_S)}), flush=True)
            os._exit(3)


class CkksRing:
    """tfhe_malloc -> tfhe_nntt -> tfhe_mul -> tfhe_inntt -> tfhe_keyswitch (special prime) -> tfhe_rotate -> tfhe_free, every step into
    a fresh buffer, every input released the moment the call that reads it has returned; no host synchronisation inside a step (the
    input comes from a device-to-device copy on the context's stream).  `diag_product`: also tfhe_matmul_diag with 2 rotations."""

    def __init__(self, name, qs, batch, seed, diag_product=False):
        self.name, self.qs, self.batch = name, [int(q) for q in qs], batch
        self.Lk, self.level = len(qs), len(qs) - 1
        lv = self.level
        rng = np.random.default_rng(seed)
        self.ct = H.rand_residues(rng, qs[:lv], (batch, 2), N)
        self.mult = H.rand_residues(rng, qs[:lv], (batch, 2), N)          # NTT domain
        self.evk = H.uniform_evk(rng, qs, self.Lk, N)
        self.g = pow(3, 5, 2 * N)
        self.shape = (batch, 2, lv, N)
        self.nbytes = batch * 2 * lv * N * 8
        self.md = diag_product
        if self.md:
            self.md_gs = [pow(3, 1, 2 * N), pow(3, 2, 2 * N)]
            self.md_evks = [H.uniform_evk(rng, qs, self.Lk, N) for _ in self.md_gs]
            self.md_diags = H.rand_residues(rng, qs[:lv], (len(self.md_gs) + 1,), N)

    def setup(self):
        """the context and the read-only operands, by the thread that drives the ring"""
        self.ctx = tf.Context(N, self.qs)
        self.d_ct, self.d_mult, self.d_evk = upload(self.ct), upload(self.mult), upload(self.evk)
        if self.md:
            self.d_diags, self.md_keys = upload(self.md_diags), []
            for evk, g in zip(self.md_evks, self.md_gs):
                raw, prep = upload(evk), malloc(evk.nbytes)
                self.ctx.galois_key_prepare(self.Lk, self.Lk, g, raw, prep)
                free(raw)
                self.md_keys.append(prep)

    def step(self, consumed=free):
        c, lv, Lk, b, nb = self.ctx, self.level, self.Lk, self.batch, self.nbytes
        x = malloc(nb)
        ck(L.tfhe_memcpy_d2d(c.h, x, self.d_ct, nb))
        outs = []
        if self.md:
            o = malloc(nb)
            c.matmul_diag(Lk, lv, True, self.md_keys, Lk, self.md_gs, self.d_diags, x, o, b)
            outs.append(o)
        y = malloc(nb); c.nntt(x, y, b * 2, lv); consumed(x)
        x = malloc(nb); c.mul(y, self.d_mult, x, b * 2, lv); consumed(y)
        y = malloc(nb); c.inntt(x, y, b * 2, lv); consumed(x)
        x = malloc(nb); c.keyswitch(Lk, lv, True, self.d_evk, Lk, y, 2, x, b); consumed(y)
        y = malloc(nb); c.rotate(Lk, lv, True, self.d_evk, Lk, self.g, x, y, b); consumed(x)
        return [y] + outs

    def sync(self):
        self.ctx.sync()

    def fetch(self, outs):
        got = [download(p, self.shape) for p in outs]
        for p in outs:
            free(p)
        return got

    def oracle(self):
        """item 0 of the batch"""
        ref, lv = ref_cpu.RefCtx(N, self.qs), self.level
        idx = range(lv)
        a = ref.nntt(self.ct[:1].reshape(-1, lv, N), idx=idx)
        a = ref.pointwise("mul", a, self.mult[:1].reshape(-1, lv, N), idx=idx)
        a = ref.inntt(a, idx=idx).reshape(1, 2, lv, N)
        a = ref.keyswitch(lv, True, self.evk, a)
        want = [ref_rotate(ref, lv, True, self.evk, self.g, a)]
        if self.md:
            want.append(matmul_diag_ref(ref, lv, True, self.md_evks, self.md_gs, self.md_diags, self.ct[:1]))
        return want


class BfvRing:
    """tfhe_bfv_mul_relin through a plan over TWO contexts (the extension-basis work on the big ring's stream)"""
    name, t, ns, batch = "bfv", 65537, 2, 2

    def __init__(self, seed):
        self.ch = H.chain(50, 5, N)
        self.qs = self.ch[:self.ns]
        rng = np.random.default_rng(seed)
        self.c1, self.c2 = H.rand_residues(rng, self.qs, (self.batch, 2), N), H.rand_residues(rng, self.qs, (self.batch, 2), N)
        self.evk = H.uniform_evk(rng, self.qs, self.ns, N)
        self.shape = (self.batch, 2, self.ns, N)
        self.nbytes = self.c1.nbytes

    def setup(self):
        self.small, self.big = tf.Context(N, self.qs), tf.Context(N, self.ch)
        self.plan = tf.BfvPlan(self.small, self.big, self.t)
        self.d_c1, self.d_c2, self.d_evk = upload(self.c1), upload(self.c2), upload(self.evk)

    def step(self, consumed=free):
        nb = self.nbytes
        x1, x2, o = malloc(nb), malloc(nb), malloc(nb)
        ck(L.tfhe_memcpy_d2d(self.small.h, x1, self.d_c1, nb))
        ck(L.tfhe_memcpy_d2d(self.small.h, x2, self.d_c2, nb))
        self.plan.mul_relin(self.d_evk, self.ns, x1, x2, o, self.batch)
        consumed(x1); consumed(x2)
        return [o]

    def sync(self):
        self.small.sync()

    fetch = CkksRing.fetch

    def oracle(self):
        rs, rb = ref_cpu.RefCtx(N, self.qs), ref_cpu.RefCtx(N, self.ch)
        return [rs.keyswitch(self.ns, False, self.evk, ref_cpu.bfv_mul(rs, rb, self.t, self.c1[:1], self.c2[:1]))]


def mixed_chain():
    return H.chain(60, 1, N) + H.chain(40, 3, N) + [H.chain(60, 2, N)[1]]     # tests/test_gpu_lanes.py mixed_chain


def mixed_ring(seed):
    # batch 32: 64 polynomials x 4 limbs x N = 2^20 words, where a mixed ring forks its two lanes (TFHE_MIXED_MIN_WORDS)
    return CkksRing("mixed", mixed_chain(), 32, seed)


# ---- scenarios 1 and 2 ---------------------------------------------------------------------------------------------------------
REJECTED = [   # (call on (ctx handle, two device buffers), status, text): refused on the host, before any device use
    (lambda h, a, b: L.tfhe_nntt(h, None, b, 1, 1, None), tf.native.E_BADARG, "null argument"),
    (lambda h, a, b: L.tfhe_keyswitch(h, 3, 4, 0, a, 3, a, 2, b, 1), tf.native.E_LEVEL, "level=4 outside [1,3]"),
    (lambda h, a, b: L.tfhe_galois(h, a, b, 2, 1, 1, None), tf.native.E_BADARG, "galois element 2 must be odd"),
    (lambda h, a, b: L.tfhe_rescale(h, a, b, 1, 1, None), tf.native.E_LEVEL, "modswitch needs at least 2 limbs"),
]


def scenario_rings():
    """Four threads, four rings, first use at once (nothing has called into the library before the barrier: contexts, tables, the
    raised-LDS table of launch.h and the per-device table of md_api.inc are all first used by racing threads), a fifth thread that
    only makes rejected calls and reads its own error text.  Then the same steps serially, and the oracle."""
    iters = 8
    rings = [CkksRing("fp50", H.chain(50, 4, N), 2, 11, diag_product=True), CkksRing("u60", H.chain(60, 4, N), 2, 12), mixed_ring(13), BfvRing(14)]
    barrier = threading.Barrier(len(rings) + 1)
    results, problems, stop = {}, [], threading.Event()

    def drive(ring):
        try:
            barrier.wait(JOIN_S)
            quiet = last_error()
            ring.setup()
            outs = []
            for _ in range(iters):
                outs.append(ring.step())
                if last_error() != quiet:
                    raise AssertionError("the error text of a working thread changed to %r" % last_error())
            ring.sync()
            results[ring.name] = [ring.fetch(o) for o in outs]
        except BaseException as e:   # noqa: BLE001 -- reported, the main thread fails the scenario
            problems.append("%s: %r" % (ring.name, e))

    rounds = [0]

    def reject():
        try:
            barrier.wait(JOIN_S)
            ctx = tf.Context(N, H.chain(50, 3, N))
            a, b = malloc(3 * N * 8), malloc(3 * N * 8)
            while rounds[0] < 20000 and (rounds[0] < 200 or not stop.is_set()):
                for call, status, text in REJECTED:
                    rc = call(ctx.h, a, b)
                    got = last_error()
                    if rc != status or got != text:
                        raise AssertionError("rejected call: status %d, text %r; expected %d, %r" % (rc, got, status, text))
                rounds[0] += 1
            free(a); free(b)
        except BaseException as e:   # noqa: BLE001
            problems.append("reject: %r" % (e,))

    workers = [threading.Thread(target=drive, args=(r,), name=r.name, daemon=True) for r in rings]
    rejecter = threading.Thread(target=reject, name="reject", daemon=True)
    for t in workers + [rejecter]:
        t.start()
    join_all(workers)
    stop.set()
    join_all([rejecter])
    if problems:
        return {"ok": False, "why": "; ".join(problems)}
    report = {"ok": True, "rejected_rounds": rounds[0], "rings": {}}
    for ring in rings:
        serial = ring.fetch(ring.step())
        want = ring.oracle()
        got = results[ring.name]
        same = all(np.array_equal(g, s) for it in got for g, s in zip(it, serial))
        first = all(np.array_equal(g[:1], w) for g, w in zip(got[0], want))
        report["rings"][ring.name] = {"iterations": len(got), "outputs": len(serial), "equal_serial": bool(same), "equal_oracle": bool(first)}
        report["ok"] = report["ok"] and same and first
    return report


# ---- scenario 3 ----------------------------------------------------------------------------------------------------------------
def scenario_finaliser():
    """A producer thread runs the mixed-ring steps and hands every input buffer to a queue the moment the consuming call has returned; a
    second thread frees them (a garbage collector's finaliser) while the producer keeps enqueuing; a third allocates blocks of the same
    size from another context, fills them with 0xFF and frees them -- a block handed out too early reads as wrong words."""
    iters = 8
    ring = mixed_ring(21)
    ring.setup()
    other = tf.Context(N, H.chain(50, 2, N))
    serial = ring.fetch(ring.step())
    ring.sync(); other.sync()
    s0 = tf.native.alloc_stats()
    q, produced, problems, outs, fills = queue.Queue(), threading.Event(), [], [], [0]

    def producer():
        try:
            for _ in range(iters):
                outs.append(ring.step(consumed=q.put))
        except BaseException as e:   # noqa: BLE001
            problems.append("producer: %r" % (e,))
        finally:
            produced.set()
            q.put(None)

    def finaliser():
        try:
            while True:
                p = q.get(timeout=JOIN_S)
                if p is None:
                    return
                free(p)
        except BaseException as e:   # noqa: BLE001
            problems.append("finaliser: %r" % (e,))

    def filler():
        try:
            while fills[0] < 5000 and (fills[0] < 50 or not produced.is_set()):
                p = malloc(ring.nbytes)
                ck(L.tfhe_memset(other.h, p, 0xFF, ring.nbytes))
                free(p)
                fills[0] += 1
        except BaseException as e:   # noqa: BLE001
            problems.append("filler: %r" % (e,))

    threads = [threading.Thread(target=f, name=f.__name__, daemon=True) for f in (producer, finaliser, filler)]
    for t in threads:
        t.start()
    join_all(threads)
    if problems:
        return {"ok": False, "why": "; ".join(problems)}
    ring.sync(); other.sync()
    got = [ring.fetch(o) for o in outs]
    s1 = tf.native.alloc_stats()
    same = len(got) == iters and all(np.array_equal(g, s) for it in got for g, s in zip(it, serial))
    first = all(np.array_equal(g[:1], w) for g, w in zip(got[0], ring.oracle()))
    return {"ok": bool(same and first), "equal_serial": bool(same), "equal_oracle": bool(first), "fills": fills[0],
            "live_before": s0["live_bytes"], "live_after": s1["live_bytes"], "reuses": s1["reuses"] - s0["reuses"]}


# ---- scenarios 4 and 5 ---------------------------------------------------------------------------------------------------------
class LongQueue:
    """Context A with a queue of in-place transforms over a 128 MiB buffer that lasts tens of milliseconds (its length comes from
    one event-timed call), ending in nntt(X -> Y) on a small X; a live context B; the oracle's transform of X."""
    limbs, count, x_count, target_ms = 4, 1024, 8, 40.0

    def __init__(self, seed, b_qs=None):
        qs = H.chain(50, self.limbs, N)
        self.A, self.B = tf.Context(N, qs), tf.Context(N, b_qs or qs)
        self.t_bytes = self.count * self.limbs * N * 8
        self.T = malloc(self.t_bytes)
        ck(L.tfhe_memset(self.A.h, self.T, 0, self.t_bytes))
        x = H.rand_residues(np.random.default_rng(seed), qs, (self.x_count,), N)
        self.want = ref_cpu.RefCtx(N, qs).nntt(x)
        self.x, self.x_bytes, self.x_shape = x, x.nbytes, x.shape
        self.X, self.Y = upload(x), malloc(x.nbytes)
        self.A.nntt(self.T, self.T, self.count, self.limbs)                    # first use, outside the timing
        e0, e1 = tf.Event(), tf.Event()
        e0.record(self.A)
        self.A.inntt(self.T, self.T, self.count, self.limbs)
        e1.record(self.A)
        self.A.sync(); self.B.sync()
        self.call_ms = e0.elapsed_ms(e1)
        self.k = int(min(4000, max(8, self.target_ms / max(self.call_ms, 1e-3))))

    def enqueue(self):
        h = self.A.h
        for i in range(self.k):
            ck((L.tfhe_nntt if i % 2 == 0 else L.tfhe_inntt)(h, self.T, self.T, self.count, self.limbs, None))
        ck(L.tfhe_nntt(h, self.X, self.Y, self.x_count, self.limbs, None))

    def free_and_overwrite(self):
        """tfhe_free(X), a tfhe_malloc of the same size, the block overwritten through B's stream: (address, milliseconds in malloc)"""
        free(self.X)
        t0 = time.perf_counter()
        p = malloc(self.x_bytes)
        ms = (time.perf_counter() - t0) * 1e3
        ck(L.tfhe_memset(self.B.h, p, 0xFF, self.x_bytes))
        self.B.sync()
        return p, ms


def scenario_handout():
    """TFHE_ALLOC_SOFT_GIB is tiny here, so the allocation waits for the parked X instead of calling hipMalloc: it must not come back
    before A's queue, on another stream than the next user's, has run."""
    Q = LongQueue(31)
    s0 = tf.native.alloc_stats()
    Q.enqueue()
    p, ms = Q.free_and_overwrite()
    Q.A.sync()
    s1 = tf.native.alloc_stats()
    equal = np.array_equal(download(Q.Y, Q.x_shape), Q.want)
    return {"ok": bool(equal and p == Q.X), "same_address": p == Q.X, "reuses": s1["reuses"] - s0["reuses"], "hip_mallocs": s1["hip_mallocs"] - s0["hip_mallocs"],
            "equal_oracle": bool(equal), "queue_calls": Q.k, "call_ms": Q.call_ms, "malloc_ms": ms}


def scenario_handout_ws():
    """The same with a workspace borrower on B: a tfhe_matmul_diag whose workspace is above TFHE_WS_KEEP_GIB (1 GiB here, the least the
    variable can say: 512 ciphertexts of 5 limbs, 88 rows each) takes it from the allocator per call.  X is a block of exactly that size,
    so alloc_ws finds it PARKED and makes B's stream wait for its release events -- the host does not wait."""
    Lk, lv, batch = 6, 5, 512
    qs = H.chain(50, Lk, N)
    rng = np.random.default_rng(51)
    gs = [pow(3, 1, 2 * N), pow(3, 2, 2 * N)]
    evks = [H.uniform_evk(rng, qs, Lk, N) for _ in gs]
    diags = H.rand_residues(rng, qs[:lv], (len(gs) + 1,), N)
    ct = H.rand_residues(rng, qs[:lv], (batch, 2), N)
    Q = LongQueue(52, b_qs=qs)
    B = Q.B
    keys = []
    for evk, g in zip(evks, gs):
        raw, prep = upload(evk), malloc(evk.nbytes)
        B.galois_key_prepare(Lk, Lk, g, raw, prep)
        keys.append(prep)
    d_diags, d_ct, serial, out = upload(diags), upload(ct), malloc(ct.nbytes), malloc(ct.nbytes)
    B.sync()
    c0 = tf.native.alloc_stats()
    B.matmul_diag(Lk, lv, True, keys, Lk, gs, d_diags, d_ct, serial, batch)     # the serial run; its workspace goes back to the cache
    B.sync()
    need = tf.native.alloc_stats()["cached_bytes"] - c0["cached_bytes"]
    if need < Q.x_bytes:
        return {"ok": False, "why": "the matrix product did not borrow its workspace (cached bytes grew by %d)" % need}
    free(Q.X)
    Q.A.sync()
    ck(L.tfhe_alloc_trim())                                                     # nothing cached: the only block alloc_ws can find is X
    Q.X = malloc(need)
    ck(L.tfhe_memcpy_h2d(Q.X, Q.x.ctypes.data, Q.x_bytes))
    s0 = tf.native.alloc_stats()
    Q.enqueue()
    free(Q.X)
    t0 = time.perf_counter()
    B.matmul_diag(Lk, lv, True, keys, Lk, gs, d_diags, d_ct, out, batch)
    t1 = time.perf_counter()
    Q.A.sync()
    pending_ms = (time.perf_counter() - t1) * 1e3                               # A's queue was still running when the call returned
    B.sync()
    s1 = tf.native.alloc_stats()
    equal = np.array_equal(download(Q.Y, Q.x_shape), Q.want)
    got = download(out, ct.shape)
    same = np.array_equal(got, download(serial, ct.shape))
    first = np.array_equal(got[:1], matmul_diag_ref(ref_cpu.RefCtx(N, qs), lv, True, evks, gs, diags, ct[:1]))
    reused = s1["reuses"] - s0["reuses"] >= 1 and s1["hip_mallocs"] == s0["hip_mallocs"] and s1["cached_bytes"] == need
    return {"ok": bool(equal and same and first and reused and pending_ms > 1.0), "workspace_bytes": need, "reuses": s1["reuses"] - s0["reuses"],
            "hip_mallocs": s1["hip_mallocs"] - s0["hip_mallocs"], "cached_after": s1["cached_bytes"], "a_pending_ms": pending_ms,
            "call_ms": (t1 - t0) * 1e3, "equal_oracle": bool(equal), "product_equal_serial": bool(same), "product_equal_oracle": bool(first),
            "queue_calls": Q.k}


def scenario_destroy():
    """tfhe_ctx_destroy(A) on a thread of its own while A's queue is pending; the free of X, which the last queued call reads, falls inside
    the destroy.  The destroy must drain A before the allocator forgets A's stream, or X comes back at once and Y is computed from 0xFF."""
    Q = LongQueue(41)
    s0 = tf.native.alloc_stats()
    returned = threading.Event()
    Q.enqueue()
    hA, Q.A.h = Q.A.h, None                                                    # the handle goes to the destroying thread

    def destroy():
        L.tfhe_ctx_destroy(hA)
        returned.set()

    D = threading.Thread(target=destroy, name="destroy", daemon=True)
    D.start()
    time.sleep(0.002)
    overlap = not returned.is_set()
    p, ms = Q.free_and_overwrite()
    join_all([D])
    s1 = tf.native.alloc_stats()
    equal = np.array_equal(download(Q.Y, Q.x_shape), Q.want)
    return {"ok": bool(equal and overlap and p == Q.X), "overlap": overlap, "same_address": p == Q.X, "reuses": s1["reuses"] - s0["reuses"],
            "equal_oracle": bool(equal), "queue_calls": Q.k, "call_ms": Q.call_ms, "malloc_ms": ms}


SCENARIOS = {"rings": scenario_rings, "finaliser": scenario_finaliser, "handout": scenario_handout, "handout_ws": scenario_handout_ws, "destroy": scenario_destroy}

if __name__ == "__main__":
    report = SCENARIOS[sys.argv[1]]()
    print(json.dumps(report), flush=True)
    sys.exit(0 if report["ok"] else 1)
