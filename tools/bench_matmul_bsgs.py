#!/usr/bin/env python3
"""A 64 x 64 diagonal matrix product on encrypted slots, in one process, alternated:
  diag_a, diag_b   tfhe_matmul_diag with 63 Galois keys, timed TWICE per round: the two against each other are the noise band
  bsgs_N1xN2       tfhe_matmul_bsgs with N1 - 1 baby and N2 - 1 giant keys, (N1, N2) in {(8, 8), (16, 4), (4, 16)}
through the mirror (she.matmul_diag / she.matmul_bsgs: packing included on every leg).  The diagonals of the BSGS legs are the
63-key leg's, regrouped by she.bsgs_diagonals.  Before timing, the words of every BSGS leg are compared with the composition it
replaces (rotate_many -> dot_plain -> rotate -> +) and its decryption with the 63-key product's.  Device events around at least
`--min-s` seconds of work per leg and round; the legs take turns round by round; medians and spreads are reported, with the key bytes
each leg keeps on the device (plain + prepared copies count twice).

usage: bench_matmul_bsgs.py [--configs ref13,ref16,fp14] [--batch 16] [--rounds 5] [--min-s 0.3] [--json FILE]
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
from toyfhe_jl_amd import she  # noqa: E402


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
    # name: (log2 N, moduli with the special prime last)
    "ref13": (13, reference_ring),
    "ref16": (16, reference_ring),
    "fp14": (14, lambda N: chain(2**50 + 1, 4, N)),
}
SPLITS = ((8, 8), (16, 4), (4, 16))
DIM = 64


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
        self.block = N // 2 // DIM
        x = nrng.normal(0, 1, (batch, N // 2)).astype(complex)
        self.c = tf.encrypt(rng, self.kp, tf.ckks_encode(x, self.R, self.scale), scale=self.scale)
        self.dv = nrng.normal(0, 1, (DIM, N // 2))
        self.gks = tf.keygen_galois_many(rng, self.kp.priv, steps=[k * self.block for k in range(1, DIM)])
        self.diags = tf.ckks_encode(self.dv.astype(complex), self.R, self.scale)
        self.key_bytes = len(self.gks[0].key.key) * 2 * self.gks[0].key.key[0].mask.ring.L * N * 8
        self.bsgs = {}
        for n1, n2 in SPLITS:
            D, bs, gs = tf.bsgs_diagonals(self.dv, n1, block=self.block)
            assert len(bs) == n1 - 1 and len(gs) == n2 - 1
            by_step = {k * self.block: g for k, g in zip(range(1, DIM), self.gks)}           # the 63-key set holds every step
            self.bsgs[(n1, n2)] = ([by_step[s] for s in bs], [by_step[s] for s in gs],
                                   tf.ckks_encode(D.reshape(-1, N // 2).astype(complex), self.R, self.scale), D)

    def legs(self):
        out = {"diag_a": lambda: tf.matmul_diag(self.gks, self.diags, self.c), "diag_b": lambda: tf.matmul_diag(self.gks, self.diags, self.c)}
        for (n1, n2), (baby, giant, stacked, _) in self.bsgs.items():
            out[f"bsgs_{n1}x{n2}"] = (lambda b=baby, g=giant, s=stacked: tf.matmul_bsgs(b, g, s, self.c))
        return out

    def check(self):
        """words against the composition; decryption against the 63-key product (both approximate the same slots)"""
        md = tf.matmul_diag(self.gks, self.diags, self.c)
        ref = tf.ckks_decode(tf.decrypt(self.kp, md), md.scale)
        worst = {}
        for (n1, n2), (baby, giant, stacked, D) in self.bsgs.items():
            got = tf.matmul_bsgs(baby, giant, stacked, self.c)
            rots = [self.c] + list(tf.rotate_many(baby, self.c))
            flat = D.reshape(-1, self.N // 2).astype(complex)
            rows = [tf.ckks_encode(flat[r], self.R, self.scale) for r in range(flat.shape[0])]      # single elements, to broadcast
            want = None
            for j in range(n2):
                inner = tf.CipherText.dot_plain(rots, [d.broadcast_to(self.batch) for d in rows[j * n1:(j + 1) * n1]])
                want = inner if j == 0 else want + tf.rotate(giant[j - 1], inner)
            for a, b in zip(got.cs, want.cs):
                assert np.array_equal(a.to_numpy(), b.to_numpy()), f"tfhe_matmul_bsgs ({n1}, {n2}) differs from the composition"
            worst[f"{n1}x{n2}"] = float(np.abs(tf.ckks_decode(tf.decrypt(self.kp, got), got.scale) - ref).max())
        return worst

    def time_leg(self, f, min_s):
        """milliseconds per product from device events around >= min_s seconds of enqueued work"""
        ctx = self.R.ctx
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
        return e0.elapsed_ms(e1) / reps


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v)}


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
        row = {"config": name, "N": case.N, "batch": a.batch, "limbs": case.R.L, "dim": DIM, "rounds": a.rounds,
               "unit": "ms per 64 x 64 product over the batch", "key_bytes_each": case.key_bytes,
               "keys": {"diag": DIM - 1, **{f"bsgs_{n1}x{n2}": n1 + n2 - 2 for n1, n2 in SPLITS}},
               "max_slot_difference_to_diag": diff}
        row.update({k: summary(v) for k, v in ms.items()})
        row["noise_band"] = abs(row["diag_b"]["median"] / row["diag_a"]["median"] - 1.0)
        for n1, n2 in SPLITS:
            row[f"bsgs_{n1}x{n2}_over_diag"] = row[f"bsgs_{n1}x{n2}"]["median"] / row["diag_a"]["median"]
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
