#!/usr/bin/env python3
"""The key switch with one digit per limb and one special prime (tfhe_keyswitch) against grouped digits and several special primes
(tfhe_keyswitch_grouped), on raw residues through the C ABI, in one process, the legs of a ring alternated round by round:

  infer    N = 2^16, the infer.jl ring 60 + 5 x 40 bits, level 6:  per-limb digits + one 60-bit special prime
                     | 2 limbs per digit + three 40-bit special primes | 3 limbs per digit + three 40-bit special primes
  cfg3     N = 2^15, 10 x 40 bits:  per-limb + one 40-bit special prime | 3 per digit + three 41-bit | 2 per digit + two 41-bit
  cfg4     N = 2^14, 6 x 50 bits:   per-limb + one 50-bit special prime (the fused kernel) | 2 per digit + two 50-bit | 3 per digit + three 50-bit
  fp13     N = 2^13, 6 x 50 bits:   the same three at the other fused size

Every leg has a context of its own (its key ring), a uniform key and a uniform 2-element ciphertext batch; before it is timed its first
and last ciphertext are compared with the oracle (oracle/ref_cpu.py for the per-limb legs, tests/ks_grouped_oracle.py for the grouped
ones).  Device events around at least `--min-s` seconds of work per leg and round, after a warm-up; medians and spreads.  Forward and
inverse transform rows per key switch and the bytes of one key are computed from the shapes, not measured.

usage: bench_keyswitch_grouped.py [--rings infer,cfg3,cfg4,fp13] [--batches infer=16+64,cfg3=512,cfg4=512,fp13=512] [--rounds 3] [--min-s 0.5]
                                  [--txt FILE] [--json FILE] [--no-check]
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
from tests import ks_grouped_oracle as KO  # noqa: E402


def infer_ring(N, specials):
    return H.chain(60, 1, N) + H.chain(40, 5, N) + specials(N)


RINGS = {
    # name: (log2 N, ciphertext limbs, [(leg, moduli of the key ring, n_special, group)]); group 0: tfhe_keyswitch
    "infer": (16, 6, [("per-limb, one 60-bit special prime", lambda N: infer_ring(N, lambda N: [H.chain(60, 2, N)[1]]), 1, 0),
                      ("2 per digit, three 40-bit special primes", lambda N: H.chain(60, 1, N) + H.chain(40, 8, N), 3, 2),
                      ("3 per digit, three 40-bit special primes", lambda N: H.chain(60, 1, N) + H.chain(40, 8, N), 3, 3)]),
    "cfg3": (15, 10, [("per-limb, one 40-bit special prime", lambda N: H.chain(40, 11, N), 1, 0),
                      ("3 per digit, three 41-bit special primes", lambda N: H.chain(40, 10, N) + H.chain(41, 3, N), 3, 3),
                      ("2 per digit, two 41-bit special primes", lambda N: H.chain(40, 10, N) + H.chain(41, 2, N), 2, 2)]),
    "cfg4": (14, 6, [("per-limb, one 50-bit special prime", lambda N: H.chain(50, 7, N), 1, 0),
                     ("2 per digit, two 50-bit special primes", lambda N: H.chain(50, 8, N), 2, 2),
                     ("3 per digit, three 50-bit special primes", lambda N: H.chain(50, 9, N), 3, 3)]),
    "fp13": (13, 6, [("per-limb, one 50-bit special prime", lambda N: H.chain(50, 7, N), 1, 0),
                     ("2 per digit, two 50-bit special primes", lambda N: H.chain(50, 8, N), 2, 2),
                     ("3 per digit, three 50-bit special primes", lambda N: H.chain(50, 9, N), 3, 3)]),
}
BATCHES = {"infer": [16, 64], "cfg3": [512], "cfg4": [512], "fp13": [512]}


class Leg:
    def __init__(self, name, N, level, qs, k, group, batch, check):
        self.name, self.N, self.level, self.qs, self.k, self.group, self.batch = name, N, level, qs, k, group, batch
        Lk = self.Lk = len(qs)
        assert Lk == level + k
        self.ctx = tf.Context(N, qs)
        self.d = level if group == 0 else -(-level // group)
        rng = np.random.default_rng(N % 977 + Lk + group)
        evk = H.uniform_evk(rng, qs, self.d, N)
        two = H.rand_residues(rng, qs[:level], (2, 2), N)              # the first and the last ciphertext: the ones compared
        self.evk = tf.DeviceBuffer.from_numpy(evk)
        ct = np.empty((batch, 2, level, N), dtype=np.uint64)
        ct[:] = H.rand_residues(rng, qs[:level], (1, 2), N)
        ct[0], ct[-1] = two[0], two[1]
        self.ct = tf.DeviceBuffer.from_numpy(ct)
        self.out = tf.DeviceBuffer(batch * 2 * level * N)
        self.worst = None
        if check:
            ref = ref_cpu.RefCtx(N, qs)
            assert self.ctx.psis == ref.psis
            want = ref.keyswitch(level, True, evk, two) if group == 0 else KO.keyswitch_grouped_ref(ref, level, k, group, evk, two)
            self.run()
            self.ctx.sync()
            got = self.out.to_numpy((batch, 2, level, N))[[0, batch - 1]]
            assert np.array_equal(got, want), f"{name}: the device's words differ from the oracle's"
            self.worst = 0

    def run(self):
        if self.group == 0:
            self.ctx.keyswitch(self.Lk, self.level, True, self.evk.ptr, self.d, self.ct.ptr, 2, self.out.ptr, self.batch)
        else:
            self.ctx.keyswitch_grouped(self.Lk, self.level, self.k, self.group, self.evk.ptr, self.d, self.ct.ptr, 2, self.out.ptr, self.batch)

    def shape(self):
        nw = self.level + self.k
        return {"digits": self.d, "forward_rows": self.d * nw, "inverse_rows": 2 * nw, "key_rows": self.d * 2 * self.Lk,
                "key_bytes": self.d * 2 * self.Lk * self.N * 8}

    def time(self, min_s):
        """milliseconds per call from device events around >= min_s seconds of enqueued work"""
        ctx = self.ctx
        e0, e1 = tf.Event(), tf.Event()
        ctx.sync()
        e0.record(ctx)
        self.run()
        e1.record(ctx)
        one = max(1e-6, e0.elapsed_ms(e1) * 1e-3)
        reps = max(3, int(min_s / one) + 1)
        e0.record(ctx)
        for _ in range(reps):
            self.run()
        e1.record(ctx)
        return e0.elapsed_ms(e1) / reps


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", default="infer,cfg3,cfg4,fp13")
    ap.add_argument("--batches", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-s", type=float, default=0.5)
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
    say(f"{'ring':6} {'N':>6} {'batch':>5}  {'leg':44} {'ms/call':>9} {'us/ct':>8} {'spread':>7} {'fwd':>4} {'inv':>4} {'key MiB':>8} {'vs per-limb':>11}")
    for ring in [r for r in a.rings.split(",") if r]:
        logn, level, specs = RINGS[ring]
        N = 1 << logn
        for batch in batches[ring]:
            check = not a.no_check and batch == batches[ring][0]        # (a ring's further batches run the same code on the same shapes)
            legs = [Leg(name, N, level, mk(N), k, group, batch, check) for name, mk, k, group in specs]
            for leg in legs:                                   # warm-up: workspaces, tables, clocks
                for _ in range(3):
                    leg.run()
                leg.ctx.sync()
            ms = [[] for _ in legs]
            for _ in range(a.rounds):
                for i, leg in enumerate(legs):                 # alternated
                    ms[i].append(leg.time(a.min_s))
            base = statistics.median(ms[0])
            for leg, v in zip(legs, ms):
                s, sh = summary(v), leg.shape()
                row = {"ring": ring, "N": N, "level": level, "batch": batch, "leg": leg.name, "n_special": leg.k, "group": leg.group,
                       "oracle_checked": leg.worst == 0, "ms_per_call": s, "us_per_ciphertext": 1e3 * s["median"] / batch,
                       "time_over_per_limb": s["median"] / base, **sh}
                results.append(row)
                say(f"{ring:6} {N:>6} {batch:>5}  {leg.name:44} {s['median']:9.3f} {row['us_per_ciphertext']:8.2f} {s['spread_pct']:6.1f}% "
                    f"{sh['forward_rows']:>4} {sh['inverse_rows']:>4} {sh['key_bytes'] / 2**20:8.1f} {row['time_over_per_limb']:11.3f}")
            del legs
            tf.native.lib().tfhe_alloc_trim()
    for path, dump in ((a.txt, lambda fh: fh.write("\n".join(lines) + "\n")), (a.json, lambda fh: json.dump({"results": results}, fh, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                dump(fh)


if __name__ == "__main__":
    main()
