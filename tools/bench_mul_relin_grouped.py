#!/usr/bin/env python3
"""The product, relinearised on a grouped-digit key and rescaled, as ONE call (tfhe_mul_relin_grouped) against the chain of public
entry points it replaces -- tfhe_nntt x2 -> tfhe_tensor -> tfhe_inntt -> tfhe_keyswitch_grouped(polys = 3) -> tfhe_rescale -- in the same
process, on the same context, key and operands, and against tfhe_mul_relin on a per-limb key with one special prime; on raw residues
through the C ABI, the legs of a ring alternated round by round:

  infer    N = 2^16, the infer.jl ring 60 + 5 x 40 bits, level 6:  per-limb + one 60-bit special prime | 3 limbs per digit + three 40-bit
  cfg3     N = 2^15, 10 x 40 bits:  per-limb + one 40-bit special prime | 3 per digit + three 41-bit special primes
  cfg4     N = 2^14, 6 x 50 bits:   per-limb + one 50-bit special prime (fused product cores) | 2 per digit + two 50-bit special primes

General products (c1 != c2), coefficient-domain operands, rescale = 1.  Before a ring is timed, the one call and the chain are compared
word for word over the whole batch, and the first and last ciphertext with the oracle (tests/mul_relin_grouped_oracle.py; oracle/ref_cpu.py
for the per-limb leg).  Device events around at least `--min-s` seconds of work per leg and round, after a warm-up; medians and
spreads.  The bytes of one relinearisation key are computed from the shapes, not measured.

usage: bench_mul_relin_grouped.py [--rings infer,cfg3,cfg4] [--batches infer=16,cfg3=64,cfg4=128] [--rounds 3] [--min-s 0.3] [--txt FILE]
                                  [--json FILE] [--no-check]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import toyfhe_jl_amd as tf  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import mul_relin_grouped_oracle as MO  # noqa: E402

RINGS = {
    # name: (log2 N, ciphertext limbs, moduli of the per-limb key ring, (moduli of the grouped key ring, n_special, group))
    "infer": (16, 6, lambda N: H.chain(60, 1, N) + H.chain(40, 5, N) + [H.chain(60, 2, N)[1]], (lambda N: H.chain(60, 1, N) + H.chain(40, 8, N), 3, 3)),
    "cfg3": (15, 10, lambda N: H.chain(40, 11, N), (lambda N: H.chain(40, 10, N) + H.chain(41, 3, N), 3, 3)),
    "cfg4": (14, 6, lambda N: H.chain(50, 7, N), (lambda N: H.chain(50, 8, N), 2, 2)),
}
BATCHES = {"infer": [16], "cfg3": [64], "cfg4": [128]}


class Ring:
    """one key ring with its context, a uniform key and two uniform operand batches"""

    def __init__(self, N, level, qs, k, group, batch):
        self.N, self.level, self.qs, self.k, self.group, self.batch = N, level, qs, k, group, batch
        self.Lk = len(qs)
        assert self.Lk == level + k
        self.ctx = tf.Context(N, qs)
        self.d = level if group == 0 else -(-level // group)
        rng = np.random.default_rng(N % 977 + self.Lk + group)
        self.evk_host = H.uniform_evk(rng, qs, self.d, N)
        self.ends = [H.rand_residues(rng, qs[:level], (2, 2), N) for _ in range(2)]      # the first and last ciphertext of c1 and c2
        self.evk = tf.DeviceBuffer.from_numpy(self.evk_host)
        self.c = []
        for two in self.ends:
            ct = np.empty((batch, 2, level, N), dtype=np.uint64)
            ct[:] = H.rand_residues(rng, qs[:level], (1, 2), N)
            ct[0], ct[-1] = two[0], two[1]
            self.c.append(tf.DeviceBuffer.from_numpy(ct))
        words = batch * 2 * level * N
        self.out = tf.DeviceBuffer(batch * 2 * (level - 1) * N)
        if group:   # the chain's intermediates, allocated once: the chain is charged its launches and its traffic, not its allocations
            self.f = [tf.DeviceBuffer(words), tf.DeviceBuffer(words)]
            self.ten = tf.DeviceBuffer(batch * 3 * level * N)
            self.rel = tf.DeviceBuffer(words)
            self.out_chain = tf.DeviceBuffer(batch * 2 * (level - 1) * N)

    def call(self):
        c, a, b = self.ctx, self.c[0], self.c[1]
        if self.group == 0:
            c.mul_relin(self.Lk, self.level, True, self.evk.ptr, self.d, a.ptr, b.ptr, self.out.ptr, self.batch, rescale=True)
        else:
            c.mul_relin_grouped(self.Lk, self.level, self.k, self.group, self.evk.ptr, self.d, a.ptr, b.ptr, self.out.ptr, self.batch, rescale=True)

    def chain(self):
        c, n, level = self.ctx, self.batch, self.level
        c.nntt(self.c[0].ptr, self.f[0].ptr, n * 2, level)
        c.nntt(self.c[1].ptr, self.f[1].ptr, n * 2, level)
        c.tensor(self.f[0].ptr, self.f[1].ptr, self.ten.ptr, n, level)
        c.inntt(self.ten.ptr, self.ten.ptr, n * 3, level)
        c.keyswitch_grouped(self.Lk, level, self.k, self.group, self.evk.ptr, self.d, self.ten.ptr, 3, self.rel.ptr, n)
        c.rescale(self.rel.ptr, self.out_chain.ptr, n * 2, level)

    def check(self):
        ref = ref_cpu.RefCtx(self.N, self.qs)
        assert self.ctx.psis == ref.psis
        level, shape = self.level, (self.batch, 2, self.level - 1, self.N)
        self.call()
        self.ctx.sync()
        got = self.out.to_numpy(shape)
        if self.group == 0:
            rel = ref.keyswitch(level, True, self.evk_host, ref.enc_mul(self.ends[0], self.ends[1], idx=range(level)))
            want = MO.rescale_ref(ref, level, rel)
        else:
            want = MO.mul_relin_grouped_ref(ref, level, self.k, self.group, self.evk_host, self.ends[0], self.ends[1], rescale=True)
            self.chain()
            self.ctx.sync()
            assert np.array_equal(got, self.out_chain.to_numpy(shape)), "the one call and the chain differ"
        assert np.array_equal(got[[0, self.batch - 1]], want), "the device's words differ from the oracle's"

    def key_bytes(self):
        return self.d * 2 * self.Lk * self.N * 8


def time_leg(ctx, run, min_s):
    """milliseconds per call from device events around >= min_s seconds of enqueued work"""
    e0, e1 = tf.Event(), tf.Event()
    ctx.sync()
    e0.record(ctx)
    run()
    e1.record(ctx)
    one = max(1e-6, e0.elapsed_ms(e1) * 1e-3)
    reps = max(3, int(min_s / one) + 1)
    e0.record(ctx)
    for _ in range(reps):
        run()
    e1.record(ctx)
    return e0.elapsed_ms(e1) / reps


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", default="infer,cfg3,cfg4")
    ap.add_argument("--batches", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-s", type=float, default=0.3)
    ap.add_argument("--txt", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    batches = dict(BATCHES)
    for item in [x for x in a.batches.split(",") if x]:
        name, bs = item.split("=")
        batches[name] = [int(b) for b in bs.split("+")]
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"{'ring':6} {'N':>6} {'batch':>5}  {'leg':58} {'ms/call':>9} {'us/ct':>8} {'spread':>7} {'key MiB':>8} {'vs chain':>9} {'vs per-limb':>11}")
    for ring in [r for r in a.rings.split(",") if r]:
        logn, level, per_limb, (grouped, k, group) = RINGS[ring]
        N = 1 << logn
        for batch in batches[ring]:
            pl, gr = Ring(N, level, per_limb(N), 1, 0, batch), Ring(N, level, grouped(N), k, group, batch)
            checked = not a.no_check and batch == batches[ring][0]
            if checked:
                pl.check()
                gr.check()
            gname = f"{group} per digit, {k} special primes"
            legs = [(f"tfhe_mul_relin, per-limb, one special prime", pl, pl.call), (f"chain of entry points, {gname}", gr, gr.chain),
                    (f"tfhe_mul_relin_grouped, {gname}", gr, gr.call)]
            for _, r, run in legs:                             # warm-up: workspaces, tables, clocks
                for _ in range(3):
                    run()
                r.ctx.sync()
            ms = [[] for _ in legs]
            for _ in range(a.rounds):
                for i, (_, r, run) in enumerate(legs):         # alternated
                    ms[i].append(time_leg(r.ctx, run, a.min_s))
            base, chain = statistics.median(ms[0]), statistics.median(ms[1])
            for (name, r, _), v in zip(legs, ms):
                s = summary(v)
                row = {"ring": ring, "N": N, "level": level, "batch": batch, "leg": name, "n_special": r.k, "group": r.group, "oracle_checked": checked,
                       "ms_per_call": s, "us_per_ciphertext": 1e3 * s["median"] / batch, "time_over_chain": s["median"] / chain,
                       "time_over_per_limb": s["median"] / base, "key_bytes": r.key_bytes()}
                results.append(row)
                say(f"{ring:6} {N:>6} {batch:>5}  {name:58} {s['median']:9.3f} {row['us_per_ciphertext']:8.2f} {s['spread_pct']:6.1f}% "
                    f"{r.key_bytes() / 2**20:8.1f} {row['time_over_chain']:9.3f} {row['time_over_per_limb']:11.3f}")
            del legs, pl, gr
            tf.native.lib().tfhe_alloc_trim()
    for path, dump in ((a.txt, lambda fh: fh.write("\n".join(lines) + "\n")), (a.json, lambda fh: json.dump({"results": results}, fh, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                dump(fh)


if __name__ == "__main__":
    main()
