#!/usr/bin/env python3
"""Multiply + relinearise + rescale (squaring) per second, three ways in one process, alternated:
  (a) tfhe_mul_relin                                              -- the code under test
  (b) tfhe_nntt -> tfhe_tensor -> tfhe_inntt -> tfhe_keyswitch -> tfhe_rescale on packed buffers   -- baseline: existing entry points
  (c) she.modswitch(she.keyswitch(ek, c * c))                     -- baseline: what a caller of the host mirror pays today
Device events around at least `--min-s` seconds of work per leg and round; the legs take turns round by round so that clock and
thermal drift hit all three alike; the spread over the rounds is reported next to the median.

usage: bench_mul_relin.py [--configs ref13,cfg4,cfg5] [--rounds 5] [--min-s 0.5] [--json profiles/mul_relin_bench.json]
       bench_mul_relin.py --once ref13 --leg a      (one leg of one configuration a few times: for a kernel trace)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import toyfhe_jl_amd as tf  # noqa: E402


def chain(start, n, N):
    out, p = [], tf.nextprime(start, 1, 2 * N)
    for _ in range(n):
        out.append(p)
        p = tf.nextprime(p + 2 * N, 1, 2 * N)
    return out


def reference_ring(N):   # infer.jl:97-112
    q0, ps = chain(2**60 + 1, 2, N)
    return [q0] + chain(2**40 + 1, 5, N) + [ps]


CONFIGS = {
    # name: (log2 N, moduli, batch, product path)
    "ref13": (13, reference_ring, 64, "fused (both cores)"),
    "cfg4": (14, lambda N: chain(2**50 + 1, 7, N), 256, "fused (fp64 core)"),
    "cfg5": (16, reference_ring, 16, "composed"),
}


class Case:
    def __init__(self, name):
        logn, mk, self.batch, self.path = CONFIGS[name]
        self.name, self.N = name, 1 << logn
        qs = mk(self.N)
        self.Lk, self.level = len(qs), len(qs) - 1
        N, batch, level = self.N, self.batch, self.level
        ring = tf.NegacyclicRing(N, qs)
        self.params = tf.ModulusRaised(tf.CKKSParams(ring, 0, 3.2))
        rng = tf.DeviceRng(11)
        kp = tf.keygen(rng, self.params)
        self.ek = tf.keygen_evalmult(rng, kp.priv)
        x = np.tile(np.linspace(-1, 1, N // 2), (batch, 1)).astype(complex)
        self.ct = tf.encrypt(rng, kp, tf.ckks_encode(x, self.params.R_cipher(), 2**40), scale=2**40)
        self.ctx = self.ek.key.key[0].mask.ring.ctx
        # (a), (b): the packed coefficient-domain image of the same ciphertext
        self.packed = tf.she._pack([c.coeffs_primal() for c in self.ct.cs], self.ct.ring(), batch, ctx=self.ctx)
        self.key = self.ek.key.packed()
        self.ndig = len(self.ek.key.key)
        self.out_a = tf.DeviceBuffer(batch * 2 * (level - 1) * N)
        self.out_b = tf.DeviceBuffer(batch * 2 * (level - 1) * N)
        self.f = tf.DeviceBuffer(batch * 2 * level * N)
        self.t = tf.DeviceBuffer(batch * 3 * level * N)
        self.r = tf.DeviceBuffer(batch * 2 * level * N)

    def leg_a(self):
        self.ctx.mul_relin(self.Lk, self.level, True, self.key.ptr, self.ndig, self.packed.ptr, self.packed.ptr, self.out_a.ptr, self.batch, rescale=True)

    def leg_b(self):
        c, b, l = self.ctx, self.batch, self.level
        c.nntt(self.packed.ptr, self.f.ptr, b * 2, l)
        c.tensor(self.f.ptr, self.f.ptr, self.t.ptr, b, l)
        c.inntt(self.t.ptr, self.t.ptr, b * 3, l)
        c.keyswitch(self.Lk, l, True, self.key.ptr, self.ndig, self.t.ptr, 3, self.r.ptr, b)
        c.rescale(self.r.ptr, self.out_b.ptr, b * 2, l)

    def leg_c(self):
        r = tf.modswitch(tf.keyswitch(self.ek, self.ct * self.ct))
        r.cs[0].coeffs_primal()                         # (already there: the rescale leaves coefficients)

    def check(self):
        self.leg_a()
        self.leg_b()
        self.ctx.sync()
        assert np.array_equal(self.out_a.to_numpy(), self.out_b.to_numpy()), "tfhe_mul_relin differs from the composed chain"

    def time_leg(self, f, min_s):
        """products per second from device events around >= min_s seconds of enqueued work"""
        ctx = self.ctx
        e0, e1 = tf.Event(), tf.Event()
        f()
        ctx.sync()
        e0.record(ctx)
        f()
        e1.record(ctx)
        one = max(1e-6, e0.elapsed_ms(e1) * 1e-3)
        reps = max(3, int(min_s / one) + 1)
        e0.record(ctx)
        for _ in range(reps):
            f()
        e1.record(ctx)
        return self.batch * reps / (e0.elapsed_ms(e1) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="ref13,cfg4,cfg5")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--once", default=None, help="run one configuration's leg a few times and exit (kernel traces)")
    ap.add_argument("--leg", default="a", choices=["a", "b", "c"])
    a = ap.parse_args()
    if a.once:
        case = Case(a.once)
        f = {"a": case.leg_a, "b": case.leg_b, "c": case.leg_c}[a.leg]
        for _ in range(4):
            f()
        case.ctx.sync()
        print(f"{a.once} leg {a.leg}: 4 calls of batch {case.batch}")
        return
    results = []
    for name in a.configs.split(","):
        case = Case(name)
        case.check()
        legs = {"a": case.leg_a, "b": case.leg_b, "c": case.leg_c}
        for f in legs.values():                           # warm-up: workspaces, key images, allocator
            for _ in range(2):
                f()
        case.ctx.sync()
        rates = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, f in legs.items():                     # alternated
                rates[k].append(case.time_leg(f, a.min_s))
        row = {"config": name, "N": case.N, "batch": case.batch, "level": case.level, "product_path": case.path, "rounds": a.rounds}
        for k in legs:
            v = rates[k]
            row[k] = {"median_per_s": statistics.median(v), "min_per_s": min(v), "max_per_s": max(v),
                      "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v)}
        row["a_over_b"] = row["a"]["median_per_s"] / row["b"]["median_per_s"]
        row["a_over_c"] = row["a"]["median_per_s"] / row["c"]["median_per_s"]
        results.append(row)
        print(json.dumps(row), flush=True)
        del case
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump({"unit": "ciphertext squarings (multiply + relinearise + rescale) per second", "results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
