#!/usr/bin/env python3
"""The rectangular product and the fold on grouped-digit keys (tfhe_matmul_bsgs_fold_grouped, tfhe_rotate_sum_grouped) against what the
library offers without them, on raw residues through the C ABI: a 10 x 64 layer by 16 extended diagonals at n1 = 4 and a fold of radix
4 (one step of three keys) or radix 2 (two steps of one key), one input, with bias.

  infer3 / infer2   N = 2^16, 60 + 5 x 40 bits, level 6; 3 / 2 limbs per digit, three 40-bit special primes
  cfg3              N = 2^15, 10 x 40 bits, level 10; 3 limbs per digit, three 40-bit special primes

  new       tfhe_matmul_bsgs_fold_grouped, the fold on the route the process runs (see below)
  sum       tfhe_rotate_sum_grouped alone, on the same fold keys
  chain     (a) the parent commit's entry points on the same keys: tfhe_matmul_bsgs_grouped -> per step tfhe_rotate_many_grouped -> tfhe_add
            (sum-chain: the fold's part of it alone)
  per-limb  (c) tfhe_matmul_bsgs_fold (sum-per-limb: tfhe_rotate_sum) on per-limb keys with one 60-bit special prime
  padded    (d) tfhe_matmul_bsgs_grouped on the matrix padded to 64 x 64 (16 x 4: 15 baby and 3 giant keys)

The routes are read once per process, so the parent starts one child per route and round, alternated: a child without any switch times
every leg (the library's default: the fold on the coefficient route, the baby phase in the evaluation domain); `(eval)` children run with
TFHE_MDG_FOLD_EVAL=1 -- the fold in the evaluation domain -- and `(md-coeff)` children (b) with TFHE_MD_COEFF=1 -- the baby phase AND the
fold on the coefficient route --, both timing `new` and `sum` only.  Oracle-free word check first in every child of the first round:
`new` against `chain` and `sum` against `sum-chain`, word for word.  Device events around at least --min-s seconds of work per leg; medians
and spreads over the rounds.

usage: bench_matmul_rect_grouped.py [--shapes infer3,infer2,cfg3] [--batches 16+64] [--radices 4,2] [--rounds 3] [--min-s 0.2] [--txt FILE] [--json FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, DIM, N1 = 10, 64, 4


def shapes():
    from tests import helpers as H
    wide = lambda N: H.chain(60, 1, N) + H.chain(40, 8, N)
    wide1 = lambda N: H.chain(60, 1, N) + H.chain(40, 5, N) + [H.chain(60, 2, N)[1]]
    return {  # name: (log2 N, level, grouped key ring, n_special, group, per-limb key ring)
        "infer3": (16, 6, wide, 3, 3, wide1), "infer2": (16, 6, wide, 3, 2, wide1),
        "cfg3": (15, 10, lambda N: H.chain(40, 13, N), 3, 3, lambda N: H.chain(40, 10, N) + H.chain(60, 1, N)),
        "small": (12, 4, lambda N: H.chain(60, 1, N) + H.chain(40, 5, N), 2, 2, lambda N: H.chain(60, 1, N) + H.chain(40, 3, N) + [H.chain(60, 2, N)[1]]),
    }


class Side:
    """one key ring: a context, one uniform key prepared per Galois element, a ciphertext batch, diagonals, a bias"""

    def __init__(self, N, level, qs, k, group, batch, radix):
        import numpy as np

        import toyfhe_jl_amd as tf
        from tests import helpers as H
        self.tf, self.N, self.level, self.k, self.group, self.batch, self.Lk = tf, N, level, k, group, batch, len(qs)
        self.ctx = tf.Context(N, qs)
        self.d = level if group == 0 else -(-level // group)
        B = N // 2 // DIM
        _, rb, rg, rf = tf.rect_diagonals(np.zeros((ROWS, DIM)), N1, block=B, fold_radix=radix)
        _, pb, pg = tf.bsgs_diagonals(np.zeros((DIM, 1)), 16, block=B)
        el = lambda s: pow(5, s, 2 * N)
        rng = np.random.default_rng(N % 977 + self.Lk + group)
        evk = H.uniform_evk(rng, qs, self.d, N)
        src = tf.DeviceBuffer.from_numpy(evk)
        self.keys = {}
        for s in sorted(set(rb + rg + pb + pg + [s for st in rf for s in st])):
            dst = tf.DeviceBuffer(evk.size)
            self.ctx.galois_key_prepare(self.Lk, self.d, el(s), src.ptr, dst.ptr)
            self.keys[s] = dst
        ptr = lambda steps: [self.keys[s].ptr for s in steps]
        self.rb, self.rg, self.pb, self.pg = (ptr(rb), [el(s) for s in rb]), (ptr(rg), [el(s) for s in rg]), (ptr(pb), [el(s) for s in pb]), (ptr(pg), [el(s) for s in pg])
        self.rf = ([ptr(st) for st in rf], [[el(s) for s in st] for st in rf])
        self.n_keys = {"rect": len(rb) + len(rg) + sum(map(len, rf)), "padded": len(pb) + len(pg)}
        self.key_bytes = evk.size * 8
        ql = qs[:level]
        self.ct = tf.DeviceBuffer.from_numpy(np.tile(H.rand_residues(rng, ql, (1, 2), N), (batch, 1, 1, 1)))   # (one ciphertext repeated: the time does not depend on the words)
        self.diags = tf.DeviceBuffer.from_numpy(H.rand_residues(rng, ql, (len(rg) + 1, len(rb) + 1), N))
        self.pdiags = tf.DeviceBuffer.from_numpy(H.rand_residues(rng, ql, (len(pg) + 1, len(pb) + 1), N)) if group else None
        self.bias = tf.DeviceBuffer.from_numpy(H.rand_residues(rng, ql, (), N))
        self.sz = 2 * level * N
        self.out, self.f = tf.DeviceBuffer(batch * self.sz), tf.DeviceBuffer(batch * self.sz)
        self.rots = tf.DeviceBuffer(max(map(len, rf)) * batch * self.sz) if group else None
        full = np.zeros((batch, 2, level, N), dtype=np.uint64)
        full[:, 0] = self.bias.to_numpy((level, N))
        self.bias_full = tf.DeviceBuffer.from_numpy(full)

    def fold_chain(self, f):
        c, L, lv, b = self.ctx, self.Lk, self.level, self.batch
        for ptrs, gs in zip(*self.rf):
            c.rotate_many_grouped(L, lv, self.k, self.group, ptrs, self.d, gs, f.ptr, self.rots.ptr, b)
            for u in range(len(ptrs)):
                c.add(f.ptr, self.rots.ptr + u * b * self.sz * 8, f.ptr, b * 2, lv)

    def run(self, leg):
        c, L, lv, b, k, g, d = self.ctx, self.Lk, self.level, self.batch, self.k, self.group, self.d
        if leg == "new":
            c.matmul_bsgs_fold_grouped(L, lv, k, g, *self.rb, *self.rg, d, [self.diags.ptr], [self.ct.ptr], *self.rf, self.bias.ptr, self.out.ptr, b)
        elif leg == "sum":
            c.rotate_sum_grouped(L, lv, k, g, *self.rf, d, self.ct.ptr, self.out.ptr, b)
        elif leg == "chain":
            c.matmul_bsgs_grouped(L, lv, k, g, *self.rb, *self.rg, d, [self.diags.ptr], [self.ct.ptr], None, self.f.ptr, b)
            self.fold_chain(self.f)
            c.add(self.f.ptr, self.bias_full.ptr, self.f.ptr, b * 2, lv)
        elif leg == "sum-chain":
            self.tf.native.check(self.tf.native.lib().tfhe_memcpy_d2d(c.h, self.f.ptr, self.ct.ptr, b * self.sz * 8))
            self.fold_chain(self.f)
        elif leg == "padded":
            c.matmul_bsgs_grouped(L, lv, k, g, *self.pb, *self.pg, d, [self.pdiags.ptr], [self.ct.ptr], self.bias.ptr, self.out.ptr, b)
        elif leg == "per-limb":
            c.matmul_bsgs_fold(L, lv, True, *self.rb, *self.rg, d, [self.diags.ptr], [self.ct.ptr], *self.rf, self.bias.ptr, self.out.ptr, b)
        elif leg == "sum-per-limb":
            c.rotate_sum(L, lv, True, *self.rf, d, self.ct.ptr, self.out.ptr, b)
        else:
            raise AssertionError(leg)

    def check(self):
        import numpy as np
        for leg, ref, a, bbuf in (("new", "chain", self.out, self.f), ("sum", "sum-chain", self.out, self.f)):
            for buf in (a, bbuf):
                self.tf.native.check(self.tf.native.lib().tfhe_memset(self.ctx.h, buf.ptr, 0xA5, buf.n * 8))
            self.run(leg)
            self.run(ref)
            assert np.array_equal(a.to_numpy(), bbuf.to_numpy()), f"{leg} differs from {ref}"

    def time(self, leg, min_s):
        tf, ctx = self.tf, self.ctx
        e0, e1 = tf.Event(), tf.Event()
        for _ in range(2):
            self.run(leg)
        ctx.sync()
        e0.record(ctx)
        self.run(leg)
        e1.record(ctx)
        reps = max(3, int(min_s / max(1e-6, e0.elapsed_ms(e1) * 1e-3)) + 1)
        e0.record(ctx)
        for _ in range(reps):
            self.run(leg)
        e1.record(ctx)
        return e0.elapsed_ms(e1) / reps


GROUPED_LEGS = ("new", "sum", "chain", "sum-chain", "padded")
PERLIMB_LEGS = ("per-limb", "sum-per-limb")


def child(a):
    """one timing per (shape, batch, radix, leg), one JSON line each"""
    import toyfhe_jl_amd as tf
    legs = a.child.split(",")
    for shape in a.shapes.split(","):
        logn, level, gring, k, group, pring = shapes()[shape]
        N = 1 << logn
        for batch in [int(b) for b in a.batches.split("+")]:
            for radix in [int(r) for r in a.radices.split(',')]:
                for ring, kk, gg, mine in ((gring, k, group, GROUPED_LEGS), (pring, 1, 0, PERLIMB_LEGS)):
                    todo = [x for x in legs if x in mine and not (radix == 2 and x == "padded")]
                    if not todo:
                        continue
                    side = Side(N, level, ring(N), kk, gg, batch, radix)
                    if gg and not a.no_check:
                        side.check()
                    for leg in todo:
                        ms = side.time(leg, a.min_s)
                        print("ROW " + json.dumps({"shape": shape, "N": N, "level": level, "n_special": kk, "group": gg, "batch": batch, "radix": radix,
                                                   "leg": leg, "ms": ms, "keys": side.n_keys["padded" if leg == "padded" else "rect"],
                                                   "key_bytes_each": side.key_bytes, "workspace_bytes": side.ctx.workspace()[1]}), flush=True)
                    del side
                    tf.native.lib().tfhe_alloc_trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="infer3,infer2,cfg3")
    ap.add_argument("--batches", default="16+64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-s", type=float, default=0.2)
    ap.add_argument("--txt", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--radices", default="4,2", help="fold radices, of 4 and 2")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    routes = {"": ({}, GROUPED_LEGS + PERLIMB_LEGS), "(eval)": ({"TFHE_MDG_FOLD_EVAL": "1"}, ("new", "sum")),
              "(md-coeff)": ({"TFHE_MD_COEFF": "1"}, ("new", "sum"))}
    rows = {}
    for rnd in range(a.rounds):
        for route, (env, legs) in routes.items():                    # alternated: one fresh process per route and round
            cmd = [sys.executable, os.path.abspath(__file__), "--child", ",".join(legs), "--shapes", a.shapes, "--batches", a.batches, "--min-s", str(a.min_s), "--radices", a.radices]
            if a.no_check or rnd:
                cmd.append("--no-check")
            base_env = {k: v for k, v in os.environ.items() if k not in ("TFHE_MDG_FOLD_EVAL", "TFHE_MD_COEFF")}
            r = subprocess.run(cmd, env=dict(base_env, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, r.stderr[-3000:]
            for line in r.stdout.splitlines():
                if line.startswith("ROW "):
                    row = json.loads(line[4:])
                    leg = row["leg"] + route
                    key = (row["shape"], row["batch"], row["radix"], leg)
                    rows.setdefault(key, dict(row, leg=leg, ms=[]))["ms"].append(row["ms"])
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"{'shape':7} {'N':>6} {'batch':>5} {'radix':>5}  {'leg':16} {'keys':>4} {'ms/call':>9} {'min':>9} {'max':>9} {'spread':>7} {'ws GiB':>7} {'vs new':>7}")
    for (shape, batch, radix, leg), row in rows.items():
        v = row["ms"]
        med = statistics.median(v)
        base_leg = "sum" if leg.startswith("sum") else "new"
        base = statistics.median(rows[(shape, batch, radix, base_leg)]["ms"]) if (shape, batch, radix, base_leg) in rows else None
        row.update(median=med, min=min(v), max=max(v), spread_pct=100.0 * (max(v) - min(v)) / med, time_over_default_route=med / base if base else None)
        results.append(row)
        say(f"{shape:7} {row['N']:>6} {batch:>5} {radix:>5}  {leg:16} {row['keys']:>4} {med:9.3f} {min(v):9.3f} {max(v):9.3f} {row['spread_pct']:6.1f}% "
            f"{row['workspace_bytes'] / 2**30:7.2f} {(med / base if base else 0):7.3f}")
    for path, dump in ((a.txt, lambda fh: fh.write("\n".join(lines) + "\n")), (a.json, lambda fh: json.dump({"results": results}, fh, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                dump(fh)


if __name__ == "__main__":
    main()
