#!/usr/bin/env python3
"""One 10 x 64 matrix product on encrypted slots (the last layer of examples/encrypted_mnist.py), in one process, alternated:
  padded_a, padded_b   the matrix padded to 64 x 64, tfhe_matmul_bsgs at (16, 4) -- 18 key switches -- timed TWICE per round: the two
                       against each other are the noise band, and this is the path without the rectangular product
  fold_r2              tfhe_matmul_bsgs_fold: 16 extended diagonals at (4, 4) + fold steps (1, 1) -- 3 + 3 + 2 = 8 key switches
  fold_r4              the same with the fold as one step of three keys, (3,) -- 3 + 3 + 3 = 9 key switches
through the mirror (packing included on every leg).  Before timing, the words of both fold legs are compared with the composition they
replace (matmul_bsgs_blocks -> rotate_many + per fold step) and their decryption with the padded product's first 10 rows.  Device
events around at least `--min-s` seconds of work per leg and round; the legs take turns round by round; medians and spreads.

usage: bench_matmul_rect.py [--configs ref13,ref16,fp14] [--batch 16] [--rounds 5] [--min-s 0.3] [--json FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import toyfhe_jl_amd as tf  # noqa: E402
from bench_matmul_bsgs import CONFIGS, Case as SquareCase, summary  # noqa: E402
from toyfhe_jl_amd import she  # noqa: E402

ROWS, DIM = 10, 64


class Case:
    def __init__(self, name, batch):
        logn, mk = CONFIGS[name]
        self.name, self.N, self.batch = name, 1 << logn, batch
        N = self.N
        params = tf.ModulusRaised(tf.CKKSParams(tf.NegacyclicRing(N, mk(N)), 0, 3.2))
        self.params, self.R = params, params.R_cipher()
        rng = tf.DeviceRng(5)
        self.kp = tf.keygen(rng, params)
        nrng = np.random.default_rng(5)
        self.scale = 2**30
        B = self.block = N // 2 // DIM
        x = nrng.normal(0, 1, (batch, N // 2)).astype(complex)
        self.c = tf.encrypt(rng, self.kp, tf.ckks_encode(x, self.R, self.scale), scale=self.scale)
        self.W = nrng.normal(0, 1, (ROWS, DIM))
        enc = lambda D: tf.ckks_encode(D.reshape(-1, N // 2).astype(complex), self.R, self.scale)
        # the padded product: 64 diagonals of [W; 0], regrouped at (16, 4)
        Wp = np.vstack([self.W, np.zeros((DIM - ROWS, DIM))])
        dv = np.stack([np.repeat(np.array([Wp[i, (i - k) % DIM] for i in range(DIM)]), B) for k in range(DIM)])
        D, bs, gs = tf.bsgs_diagonals(dv, 16, block=B)
        steps = set(bs + gs)
        self.rect = {}
        for radix in (2, 4):
            Dr, rb, rg, rf = tf.rect_diagonals(self.W, 4, block=B, fold_radix=radix)
            self.rect[radix] = (Dr, rb, rg, rf)
            steps |= set(rb + rg + [s for g in rf for s in g])
        steps = sorted(steps)
        by_step = dict(zip(steps, tf.keygen_galois_many(rng, self.kp.priv, steps=steps)))
        self.padded = ([by_step[s] for s in bs], [by_step[s] for s in gs], enc(D))
        self.folds = {radix: ([by_step[s] for s in rb], [by_step[s] for s in rg], [[by_step[s] for s in g] for g in rf], enc(Dr))
                      for radix, (Dr, rb, rg, rf) in self.rect.items()}
        self.keys = {"padded": len(bs) + len(gs), **{f"fold_r{r}": len(b) + len(g) + sum(map(len, f)) for r, (b, g, f, _) in self.folds.items()}}

    def legs(self):
        pb, pg, pd = self.padded
        out = {"padded_a": lambda: tf.matmul_bsgs(pb, pg, pd, self.c), "padded_b": lambda: tf.matmul_bsgs(pb, pg, pd, self.c)}
        for radix, (b, g, f, d) in self.folds.items():
            out[f"fold_r{radix}"] = (lambda b=b, g=g, f=f, d=d: tf.matmul_bsgs_fold(b, g, [d], [self.c], f))
        return out

    def check(self):
        """words against the composition; decryption of the first 10 rows against the padded product's"""
        pb, pg, pd = self.padded
        md = tf.matmul_bsgs(pb, pg, pd, self.c)
        ref = tf.ckks_decode(tf.decrypt(self.kp, md), md.scale).reshape(self.batch, DIM, self.block)[:, :ROWS]
        worst = {}
        for radix, (b, g, f, d) in self.folds.items():
            got = tf.matmul_bsgs_fold(b, g, [d], [self.c], f)
            want = tf.matmul_bsgs_blocks(b, g, [d], [self.c])
            for grp in f:
                acc = want
                for r in tf.rotate_many(grp, want):
                    acc = acc + r
                want = acc
            for x, y in zip(got.cs, want.cs):
                assert np.array_equal(x.to_numpy(), y.to_numpy()), f"tfhe_matmul_bsgs_fold (radix {radix}) differs from the composition"
            dec = tf.ckks_decode(tf.decrypt(self.kp, got), got.scale).reshape(self.batch, DIM, self.block)[:, :ROWS]
            worst[f"fold_r{radix}"] = float(np.abs(dec - ref).max())
        return worst

    time_leg = SquareCase.time_leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="ref13,ref16,fp14")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    results = []
    for name in [c for c in a.configs.split(",") if c]:
        case = Case(name, a.batch)
        diff = case.check()
        legs = case.legs()
        for f in legs.values():                               # warm-up: workspaces, prepared keys, allocator
            for _ in range(2):
                f()
        case.R.ctx.sync()
        ms = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, f in legs.items():                         # alternated
                ms[k].append(case.time_leg(f, a.min_s))
        row = {"config": name, "N": case.N, "batch": a.batch, "limbs": case.R.L, "shape": [ROWS, DIM], "rounds": a.rounds,
               "unit": "ms per 10 x 64 product over the batch", "keys": case.keys, "max_slot_difference_to_padded": diff}
        row.update({k: summary(v) for k, v in ms.items()})
        fast = min(row["padded_a"]["median"], row["padded_b"]["median"])
        row["noise_band"] = abs(row["padded_b"]["median"] / row["padded_a"]["median"] - 1.0)
        for k in ("fold_r2", "fold_r4"):
            row[f"{k}_over_padded"] = row[k]["median"] / fast
        row["fold_r4_over_fold_r2"] = row["fold_r4"]["median"] / row["fold_r2"]["median"]
        results.append(row)
        print(json.dumps(row), flush=True)
        she.release_staging(case.R.ctx)
        del case, legs
        tf.native.lib().tfhe_alloc_trim()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump({"results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
