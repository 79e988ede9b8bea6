#!/usr/bin/env python3
"""The product by baby and giant steps on grouped-digit keys (tfhe_matmul_bsgs_grouped) against what the library offers without it, on
raw residues through the C ABI, in one process, the legs of a shape alternated round by round: a 64 x 64 layer by n1 baby steps on the
infer.jl ring (N = 2^16, 60 + 5 x 40 bits, level 6), one input, no bias.

  infer3 / infer2   3 / 2 limbs per digit, three 40-bit special primes (the key rings of tools/bench_rotate_many_grouped.py)

  grouped       tfhe_matmul_bsgs_grouped on the prepared grouped keys
  chain     (a) the composition it states, entry point by entry point on the same keys: tfhe_rotate_many_grouped -> tfhe_nntt -> one
                tfhe_dot per giant step -> tfhe_inntt -> tfhe_rotate_grouped (the plain keys) -> tfhe_add
  per-limb  (b) tfhe_matmul_bsgs on per-limb keys with one 60-bit special prime

Oracle-free word check first: before a shape's first batch size is timed, the output of `grouped` is compared with that of `chain`,
word for word over the whole batch (tests/test_gpu_matmul_bsgs_grouped.py holds the comparison with the oracle).  Device events around
at least `--min-s` seconds of work per leg and round, after a warm-up; medians and spreads over `--rounds` rounds.  Key bytes are
computed from the shapes; the workspace is read from the context after the warm-up.

usage: bench_matmul_bsgs_grouped.py [--shapes infer3,infer2] [--batches 16+64] [--n1 8] [--legs grouped,chain,per-limb] [--rounds 3]
                                    [--min-s 0.3] [--txt FILE] [--json FILE] [--no-check]
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
from tests import helpers as H  # noqa: E402

SHAPES = {
    # name: (log2 N, level, grouped key ring, n_special, group, per-limb key ring)
    "infer3": (16, 6, lambda N: H.chain(60, 1, N) + H.chain(40, 8, N), 3, 3, lambda N: H.chain(60, 1, N) + H.chain(40, 5, N) + [H.chain(60, 2, N)[1]]),
    "infer2": (16, 6, lambda N: H.chain(60, 1, N) + H.chain(40, 8, N), 3, 2, lambda N: H.chain(60, 1, N) + H.chain(40, 5, N) + [H.chain(60, 2, N)[1]]),
    "small": (12, 4, lambda N: H.chain(60, 1, N) + H.chain(40, 5, N), 2, 2, lambda N: H.chain(60, 1, N) + H.chain(40, 3, N) + [H.chain(60, 2, N)[1]]),
}
LEGS = ("grouped", "chain", "per-limb")


class Side:
    """one key ring: a context, plain and prepared copies of one uniform key per Galois element, a ciphertext batch, the diagonals"""

    def __init__(self, N, level, qs, k, group, bgs, ggs, batch, want_plain):
        self.N, self.level, self.qs, self.k, self.group, self.bgs, self.ggs, self.batch = N, level, qs, k, group, bgs, ggs, batch
        self.Lk = len(qs)
        self.ctx = tf.Context(N, qs)
        self.d = level if group == 0 else -(-level // group)
        rng = np.random.default_rng(N % 977 + self.Lk + group)
        self.evk = H.uniform_evk(rng, qs, self.d, N)
        src = tf.DeviceBuffer.from_numpy(self.evk)
        self.plain, self.prepared = [], []
        for g in bgs + ggs:
            dst = tf.DeviceBuffer(self.evk.size)
            self.ctx.galois_key_prepare(self.Lk, self.d, g, src.ptr, dst.ptr)
            self.prepared.append(dst)
            if want_plain:
                cp = tf.DeviceBuffer(self.evk.size)
                tf.native.check(tf.native.lib().tfhe_memcpy_d2d(self.ctx.h, cp.ptr, src.ptr, self.evk.size * 8))
                self.plain.append(cp)
        self.ct = tf.DeviceBuffer.from_numpy(H.rand_residues(rng, qs[:level], (batch, 2), N))
        self.nb1, self.ng1 = len(bgs) + 1, len(ggs) + 1
        self.diags = tf.DeviceBuffer.from_numpy(H.rand_residues(rng, qs[:level], (self.ng1, self.nb1), N))
        self.sz = 2 * level * N
        self.out = tf.DeviceBuffer(batch * self.sz)
        self.bptrs, self.gptrs = [p.ptr for p in self.prepared[:len(bgs)]], [p.ptr for p in self.prepared[len(bgs):]]
        if want_plain:      # the chain's intermediates: the terms [nb1][batch][2][level][N], the diagonals broadcast over the batch, the sums
            self.terms = tf.DeviceBuffer(self.nb1 * batch * self.sz)
            self.bd = tf.DeviceBuffer(self.ng1 * self.nb1 * batch * self.sz)
            for t in range(self.ng1 * self.nb1):
                tf.native.check(tf.native.lib().tfhe_broadcast_poly(self.ctx.h, self.bd.ptr + t * batch * self.sz * 8, self.diags.ptr + t * level * N * 8,
                                                                    level * N, batch * 2))
            self.inner = tf.DeviceBuffer(self.ng1 * batch * self.sz)
            self.rot = tf.DeviceBuffer(batch * self.sz)
            self.chain_out = tf.DeviceBuffer(batch * self.sz)

    def key_bytes(self):
        return len(self.bgs + self.ggs) * self.d * 2 * self.Lk * self.N * 8

    def run(self, leg):
        c, L, lv, b, sz = self.ctx, self.Lk, self.level, self.batch, self.sz
        if leg == "grouped":
            c.matmul_bsgs_grouped(L, lv, self.k, self.group, self.bptrs, self.bgs, self.gptrs, self.ggs, self.d, [self.diags.ptr], [self.ct.ptr], None,
                                  self.out.ptr, b)
        elif leg == "per-limb":
            c.matmul_bsgs(L, lv, True, self.bptrs, self.bgs, self.gptrs, self.ggs, self.d, self.diags.ptr, self.ct.ptr, self.out.ptr, b)
        else:
            tf.native.check(tf.native.lib().tfhe_memcpy_d2d(c.h, self.terms.ptr, self.ct.ptr, b * sz * 8))
            c.rotate_many_grouped(L, lv, self.k, self.group, self.bptrs, self.d, self.bgs, self.ct.ptr, self.terms.ptr + b * sz * 8, b)
            c.nntt(self.terms.ptr, self.terms.ptr, self.nb1 * b * 2, lv)
            a = [self.terms.ptr + i * b * sz * 8 for i in range(self.nb1)]
            for j in range(self.ng1):
                c.dot(None, a, [self.bd.ptr + (j * self.nb1 + i) * b * sz * 8 for i in range(self.nb1)], self.inner.ptr + j * b * sz * 8, b * 2, lv)
            c.inntt(self.inner.ptr, self.inner.ptr, self.ng1 * b * 2, lv)
            tf.native.check(tf.native.lib().tfhe_memcpy_d2d(c.h, self.chain_out.ptr, self.inner.ptr, b * sz * 8))
            for j, g in enumerate(self.ggs):
                c.rotate_grouped(L, lv, self.k, self.group, self.plain[len(self.bgs) + j].ptr, self.d, g, self.inner.ptr + (j + 1) * b * sz * 8,
                                 self.rot.ptr, b)
                c.add(self.chain_out.ptr, self.rot.ptr, self.chain_out.ptr, b * 2, lv)

    def check(self):
        """`grouped` against `chain`, every word of the batch"""
        for buf in (self.out, self.chain_out):
            tf.native.check(tf.native.lib().tfhe_memset(self.ctx.h, buf.ptr, 0xA5, buf.n * 8))
        self.run("grouped")
        self.run("chain")
        assert np.array_equal(self.out.to_numpy(), self.chain_out.to_numpy()), "tfhe_matmul_bsgs_grouped differs from the composition chain"

    def time(self, leg, min_s):
        """milliseconds per call from device events around >= min_s seconds of enqueued work"""
        ctx = self.ctx
        e0, e1 = tf.Event(), tf.Event()
        ctx.sync()
        e0.record(ctx)
        self.run(leg)
        e1.record(ctx)
        one = max(1e-6, e0.elapsed_ms(e1) * 1e-3)
        reps = max(3, int(min_s / one) + 1)
        e0.record(ctx)
        for _ in range(reps):
            self.run(leg)
        e1.record(ctx)
        return e0.elapsed_ms(e1) / reps


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="infer3,infer2")
    ap.add_argument("--batches", default="16+64")
    ap.add_argument("--n1", type=int, default=8)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-s", type=float, default=0.3)
    ap.add_argument("--txt", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split("+")]
    legs = [x for x in a.legs.split(",") if x]
    assert all(x in LEGS for x in legs), legs
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"{'shape':7} {'N':>6} {'batch':>5} {'baby+giant':>10}  {'leg':9} {'ms/call':>9} {'spread':>7} {'keys GiB':>8} {'ws GiB':>7} {'vs grouped':>10}")
    for shape in [s for s in a.shapes.split(",") if s]:
        logn, level, gring, k, group, pring = SHAPES[shape]
        N = 1 << logn
        B = N // 128
        _, bsteps, gsteps = tf.bsgs_diagonals(np.zeros((64, 1)), a.n1, block=B)
        bgs, ggs = [pow(5, s, 2 * N) for s in bsteps], [pow(5, s, 2 * N) for s in gsteps]
        for batch in batches:
            sides = {}
            glegs = [x for x in legs if x in ("grouped", "chain")]
            plegs = [x for x in legs if x == "per-limb"]
            if glegs:
                sides["g"] = (Side(N, level, gring(N), k, group, bgs, ggs, batch, "chain" in glegs), glegs)
            if plegs:
                sides["p"] = (Side(N, level, pring(N), 1, 0, bgs, ggs, batch, False), plegs)
            checked = False
            if "g" in sides and "chain" in glegs and "grouped" in glegs and not a.no_check and batch == batches[0]:
                sides["g"][0].check()
                checked = True
            ws = {}
            for side, its in sides.values():
                for leg in its:                                        # warm-up: workspaces, tables, clocks
                    for _ in range(2):
                        side.run(leg)
                    side.ctx.sync()
                    ws[leg] = side.ctx.workspace()[1]
            ms = {leg: [] for leg in legs}
            for _ in range(a.rounds):
                for side, its in sides.values():                       # alternated
                    for leg in its:
                        ms[leg].append(side.time(leg, a.min_s))
            base = statistics.median(ms["grouped"]) if "grouped" in ms else None
            for leg in legs:
                side = sides["g" if leg in glegs else "p"][0]
                s = summary(ms[leg])
                results.append({"shape": shape, "N": N, "level": level, "batch": batch, "n_baby": len(bgs), "n_giant": len(ggs), "leg": leg,
                                "n_special": side.k, "group": side.group, "words_checked_against_the_chain": checked, "ms_per_call": s,
                                "key_bytes": side.key_bytes(), "workspace_bytes": ws[leg], "time_over_grouped": s["median"] / base if base else None})
                say(f"{shape:7} {N:>6} {batch:>5} {len(bgs):>5}+{len(ggs):<4}  {leg:9} {s['median']:9.3f} {s['spread_pct']:6.1f}% "
                    f"{side.key_bytes() / 2**30:8.2f} {ws[leg] / 2**30:7.2f} {(s['median'] / base if base else 0):10.3f}")
            del sides, side
            tf.native.lib().tfhe_alloc_trim()
    for path, dump in ((a.txt, lambda fh: fh.write("\n".join(lines) + "\n")), (a.json, lambda fh: json.dump({"results": results}, fh, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                dump(fh)


if __name__ == "__main__":
    main()
