#!/usr/bin/env python3
"""Hoisted rotations and the diagonal product on grouped-digit keys (tfhe_rotate_many_grouped, tfhe_matmul_diag_grouped) against what
the library had before them, on raw residues through the C ABI, in one process, the legs of a shape alternated round by round:

  infer2 / infer3   N = 2^16, the infer.jl ring 60 + 5 x 40 bits, level 6, 63 rotations; 2 / 3 limbs per digit, three 40-bit special primes
  cfg3              N = 2^15, 10 x 40 bits, 8 rotations; 3 limbs per digit, three 41-bit special primes

  hoisted       tfhe_rotate_many_grouped on the prepared grouped keys
  unhoisted (a) n_rot calls of tfhe_rotate_grouped on the same keys, unprepared
  per-limb  (b) tfhe_rotate_many(prepared = 1) on per-limb keys with one special prime
  product       tfhe_matmul_diag_grouped
  product   (c) tfhe_matmul_diag on the per-limb keys

Every rotation has a key buffer of its own (one uniform key, copied and prepared per Galois element).  A spot check, not the test
suite's word-for-word comparison (tests/test_gpu_rotate_many_grouped.py holds the words): before a shape's first batch size is timed, the
first and the last rotation of the first ciphertext are compared with the oracle (tests/rotate_many_grouped_oracle.py for the grouped
legs, tests/matmul_oracle.py for the per-limb ones) -- the rotations between them are not --, and the two products with the oracle's
transform and an exact integer sum over the rotations the DEVICE returned, at the first and last 256 positions of every row.  Device
events around at least `--min-s` seconds of work per leg and round, after a warm-up; medians and spreads over `--rounds` rounds (3 by
default: raise it for a figure that has to carry weight).  Key bytes and the bytes the tail kernel moves are computed from the shapes;
the workspace is read from the context after the warm-up.

usage: bench_rotate_many_grouped.py [--shapes infer2,infer3,cfg3] [--batches infer2=16+64,infer3=16+64,cfg3=512] [--legs hoisted,unhoisted,...]
                                    [--rounds 3] [--min-s 0.3] [--txt FILE] [--json FILE] [--no-check]
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
from tests import matmul_oracle as MO  # noqa: E402
from tests import rotate_many_grouped_oracle as RO  # noqa: E402

SHAPES = {
    # name: (log2 N, level, rotations, grouped key ring, n_special, group, per-limb key ring)
    "infer2": (16, 6, 63, lambda N: H.chain(60, 1, N) + H.chain(40, 8, N), 3, 2, lambda N: H.chain(60, 1, N) + H.chain(40, 5, N) + [H.chain(60, 2, N)[1]]),
    "infer3": (16, 6, 63, lambda N: H.chain(60, 1, N) + H.chain(40, 8, N), 3, 3, lambda N: H.chain(60, 1, N) + H.chain(40, 5, N) + [H.chain(60, 2, N)[1]]),
    "cfg3": (15, 10, 8, lambda N: H.chain(40, 10, N) + H.chain(41, 3, N), 3, 3, lambda N: H.chain(40, 11, N)),
}
BATCHES = {"infer2": [16, 64], "infer3": [16, 64], "cfg3": [512]}
LEGS = ("hoisted", "unhoisted", "per-limb", "product", "product-per-limb")


class Side:
    """one key ring: a context, n_rot plain and prepared copies of one uniform key, a ciphertext batch, the diagonals"""

    def __init__(self, N, level, qs, k, group, gs, batch, want_plain):
        self.N, self.level, self.qs, self.k, self.group, self.gs, self.batch = N, level, qs, k, group, gs, batch
        self.Lk = len(qs)
        self.ctx = tf.Context(N, qs)
        self.d = level if group == 0 else -(-level // group)
        rng = np.random.default_rng(N % 977 + self.Lk + group)
        self.evk = H.uniform_evk(rng, qs, self.d, N)
        src = tf.DeviceBuffer.from_numpy(self.evk)
        self.plain, self.prepared = [], []
        for g in gs:
            dst = tf.DeviceBuffer(self.evk.size)
            self.ctx.galois_key_prepare(self.Lk, self.d, g, src.ptr, dst.ptr)
            self.prepared.append(dst)
            if want_plain:
                cp = tf.DeviceBuffer(self.evk.size)
                tf.native.check(tf.native.lib().tfhe_memcpy_d2d(self.ctx.h, cp.ptr, src.ptr, self.evk.size * 8))
                self.plain.append(cp)
        self.first = H.rand_residues(rng, qs[:level], (1, 2), N)
        ct = np.empty((batch, 2, level, N), dtype=np.uint64)
        ct[:] = H.rand_residues(rng, qs[:level], (1, 2), N)
        ct[0] = self.first[0]
        self.ct = tf.DeviceBuffer.from_numpy(ct)
        self.diags_np = H.rand_residues(rng, qs[:level], (len(gs) + 1,), N)
        self.diags = tf.DeviceBuffer.from_numpy(self.diags_np)
        self.sz = 2 * level * N
        self.rots = tf.DeviceBuffer(len(gs) * batch * self.sz)
        self.prod = tf.DeviceBuffer(batch * self.sz)
        self.ptrs = [p.ptr for p in self.prepared]

    def key_bytes(self):
        return len(self.gs) * self.d * 2 * self.Lk * self.N * 8

    def tail_bytes(self):
        """what k_ks_group_rot_tail moves per call: per row group nw rows in (+ level addend rows for component 0), level rows out"""
        nw = self.level + self.k
        return len(self.gs) * self.batch * (2 * nw + self.level + 2 * self.level) * self.N * 8

    def run(self, leg):
        c, L, lv = self.ctx, self.Lk, self.level
        if leg == "hoisted":
            c.rotate_many_grouped(L, lv, self.k, self.group, self.ptrs, self.d, self.gs, self.ct.ptr, self.rots.ptr, self.batch)
        elif leg == "unhoisted":
            for r, g in enumerate(self.gs):
                c.rotate_grouped(L, lv, self.k, self.group, self.plain[r].ptr, self.d, g, self.ct.ptr, self.rots.ptr + r * self.batch * self.sz * 8, self.batch)
        elif leg == "per-limb":
            c.rotate_many(L, lv, True, self.ptrs, self.d, self.gs, self.ct.ptr, self.rots.ptr, self.batch, prepared=True)
        elif leg == "product":
            c.matmul_diag_grouped(L, lv, self.k, self.group, self.ptrs, self.d, self.gs, self.diags.ptr, self.ct.ptr, self.prod.ptr, self.batch)
        else:
            c.matmul_diag(L, lv, True, self.ptrs, self.d, self.gs, self.diags.ptr, self.ct.ptr, self.prod.ptr, self.batch)

    def check(self, legs):
        """the first and the last rotation of the first ciphertext, and the product of the first ciphertext built on ALL rotations the
        device returned (themselves compared above at both ends), against the oracle"""
        ref = ref_cpu.RefCtx(self.N, self.qs)
        assert self.ctx.psis == ref.psis
        ends = [0, len(self.gs) - 1]
        if self.group:
            want = [RO.rotate_many_grouped_ref(ref, self.level, self.k, self.group, [self.evk], [self.gs[r]], self.first)[0, 0] for r in ends]
        else:
            want = [MO.rotate(ref, self.level, True, self.evk, self.gs[r], self.first)[0] for r in ends]
        rots = None
        for leg in [x for x in legs if not x.startswith("product")]:
            tf.native.check(tf.native.lib().tfhe_memset(self.ctx.h, self.rots.ptr, 0xA5, self.rots.n * 8))
            self.run(leg)
            rots = self.rots.to_numpy((len(self.gs), self.batch, 2, self.level, self.N))[:, 0]
            for r, w in zip(ends, want):
                assert np.array_equal(rots[r], w), f"{leg}: rotation {r} differs from the oracle's words"
        for leg in [x for x in legs if x.startswith("product")]:
            if rots is None:
                self.run("hoisted" if self.group else "per-limb")
                rots = self.rots.to_numpy((len(self.gs), self.batch, 2, self.level, self.N))[:, 0]
            terms = np.concatenate([self.first, rots])
            img = ref.nntt(terms.reshape(-1, self.level, self.N), idx=range(self.level)).reshape(terms.shape)
            sel = np.r_[0:256, self.N - 256:self.N]            # the sum is pointwise in the NTT domain: exact integers at 512 positions of every row
            q = np.array([int(x) for x in self.qs[:self.level]], dtype=object).reshape(1, self.level, 1)
            tot = sum(img[t][..., sel].astype(object) * self.diags_np[t][:, sel].astype(object)[None] for t in range(terms.shape[0])) % q
            self.run(leg)
            got = self.prod.to_numpy((self.batch, 2, self.level, self.N))[0][..., sel]
            assert np.array_equal(got, tot.astype(np.uint64)), f"{leg}: the product differs from the oracle's words"

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
    ap.add_argument("--shapes", default="infer2,infer3,cfg3")
    ap.add_argument("--batches", default="")
    ap.add_argument("--legs", default=",".join(LEGS))
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
    legs = [x for x in a.legs.split(",") if x]
    assert all(x in LEGS for x in legs), legs
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"{'shape':7} {'N':>6} {'batch':>5} {'rot':>3}  {'leg':17} {'ms/call':>9} {'us/rot/ct':>9} {'spread':>7} {'keys GiB':>8} {'ws GiB':>7} {'vs hoisted':>10}")
    for shape in [s for s in a.shapes.split(",") if s]:
        logn, level, n_rot, gring, k, group, pring = SHAPES[shape]
        N = 1 << logn
        gs = [pow(5, r + 1, 2 * N) for r in range(n_rot)]
        for batch in batches[shape]:
            sides = {}
            glegs = [x for x in legs if x in ("hoisted", "unhoisted", "product")]
            plegs = [x for x in legs if x in ("per-limb", "product-per-limb")]
            if glegs:
                sides["g"] = (Side(N, level, gring(N), k, group, gs, batch, "unhoisted" in glegs), glegs)
            if plegs:
                sides["p"] = (Side(N, level, pring(N), 1, 0, gs, batch, False), plegs)
            ws = {}
            for side, its in sides.values():
                if not a.no_check and batch == batches[shape][0]:      # (a shape's further batches run the same code on the same shapes)
                    side.check(its)
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
            base = statistics.median(ms["hoisted"]) if "hoisted" in ms else None
            for leg in legs:
                side = sides["g" if leg in glegs else "p"][0]
                s = summary(ms[leg])
                row = {"shape": shape, "N": N, "level": level, "batch": batch, "n_rot": n_rot, "leg": leg, "n_special": side.k, "group": side.group,
                       "oracle_checked": not a.no_check and batch == batches[shape][0], "ms_per_call": s,
                       "us_per_rotation_and_ciphertext": 1e3 * s["median"] / (n_rot * batch), "key_bytes": side.key_bytes(), "workspace_bytes": ws[leg],
                       "time_over_hoisted": s["median"] / base if base else None}
                if leg == "hoisted":
                    row["tail_kernel_bytes_per_call"] = side.tail_bytes()
                results.append(row)
                say(f"{shape:7} {N:>6} {batch:>5} {n_rot:>3}  {leg:17} {s['median']:9.3f} {row['us_per_rotation_and_ciphertext']:9.3f} {s['spread_pct']:6.1f}% "
                    f"{side.key_bytes() / 2**30:8.2f} {ws[leg] / 2**30:7.2f} {(row['time_over_hoisted'] or 0):10.3f}")
            if "g" in sides:
                say(f"        k_ks_group_rot_tail moves {sides['g'][0].tail_bytes() / 2**30:.3f} GiB per hoisted call at this shape")
            del sides, side
            tf.native.lib().tfhe_alloc_trim()
    for path, dump in ((a.txt, lambda fh: fh.write("\n".join(lines) + "\n")), (a.json, lambda fh: json.dump({"results": results}, fh, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                dump(fh)


if __name__ == "__main__":
    main()
