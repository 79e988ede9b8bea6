#!/usr/bin/env python3
"""A 64 x 256 dense layer (infer.jl:158-163: W[:, block m] over four ciphertext batches, .+ b) on encrypted slots, in one process,
alternated, per baby/giant split (N1, N2) in {(8, 8), (16, 4)}:
  A_a, A_b   four tfhe_matmul_bsgs calls, three ciphertext additions and the bias addition -- what the layer costs without the
             block-row call -- timed TWICE per round: the two against each other are the noise band
  B          one tfhe_matmul_bsgs_blocks call with the bias
through the mirror (she.matmul_bsgs / she.matmul_bsgs_blocks: packing included on every leg).  Before timing, the words of B are
compared with the composition it replaces (rotate_many per input -> ONE dot_plain per giant step over all terms -> rotate -> + ->
+ bias), and the decryptions of A and B with the plaintext product W @ x + b.  Device events around at least `--min-s` seconds of work
per leg and round; the legs take turns round by round; medians and spreads are reported.

usage: bench_matmul_bsgs_blocks.py [--configs ref13,fp14,ref16] [--batch 16] [--rounds 5] [--min-s 0.3] [--json FILE]
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
    "fp14": (14, lambda N: chain(2**50 + 1, 4, N)),
    "ref16": (16, reference_ring),
}
SPLITS = ((8, 8), (16, 4))
DIM, N_IN = 64, 4


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
        self.block = B = N // 2 // DIM
        # slot = row * B + image: W @ x acts on the 64 rows of every image
        self.x = nrng.normal(0, 1, (N_IN, batch, DIM, B))
        self.W = nrng.normal(0, 1, (DIM, DIM * N_IN)) / 16
        self.b = nrng.normal(0, 1, DIM)
        self.cs = [tf.encrypt(rng, self.kp, tf.ckks_encode(self.x[m].reshape(batch, -1).astype(complex), self.R, self.scale), scale=self.scale)
                   for m in range(N_IN)]
        self.bias = tf.ckks_encode(np.repeat(self.b, B).astype(complex), self.R, self.scale ** 2)
        self.bias_b = self.bias.broadcast_to(batch)
        self.want = sum(np.einsum("ij,bjk->bik", self.W[:, DIM * m:DIM * (m + 1)], self.x[m]) for m in range(N_IN)) + self.b[None, :, None]
        steps = sorted({s for n1, _ in SPLITS for part in tf.bsgs_diagonals(np.zeros((DIM, 1)), n1, block=B)[1:] for s in part})
        by_step = dict(zip(steps, tf.keygen_galois_many(rng, self.kp.priv, steps=steps)))
        self.splits = {}
        for n1, n2 in SPLITS:
            Ds, enc = [], []
            for m in range(N_IN):
                Wm = self.W[:, DIM * m:DIM * (m + 1)]
                dv = np.stack([np.repeat(np.array([Wm[i, (i - k) % DIM] for i in range(DIM)]), B) for k in range(DIM)])
                D, bs, gs = tf.bsgs_diagonals(dv, n1, block=B)
                assert len(bs) == n1 - 1 and len(gs) == n2 - 1
                Ds.append(D)
                e = tf.ckks_encode(D.reshape(-1, N // 2).astype(complex), self.R, self.scale)
                e.coeffs_dual()
                enc.append(e)
            self.splits[(n1, n2)] = ([by_step[s] for s in bs], [by_step[s] for s in gs], enc, Ds)

    def leg_a(self, baby, giant, enc):
        """four calls, three +, the bias onto component 0"""
        res = tf.matmul_bsgs(baby, giant, enc[0], self.cs[0])
        for m in range(1, N_IN):
            res = res + tf.matmul_bsgs(baby, giant, enc[m], self.cs[m])
        return tf.CipherText(res.params, (res.cs[0] + self.bias_b,) + tuple(res.cs[1:]), res.scale)

    def leg_b(self, baby, giant, enc):
        return tf.matmul_bsgs_blocks(baby, giant, enc, self.cs, self.bias)

    def legs(self):
        out = {}
        for (n1, n2), (baby, giant, enc, _) in self.splits.items():
            out[f"A_a_{n1}x{n2}"] = (lambda b=baby, g=giant, e=enc: self.leg_a(b, g, e))
            out[f"A_b_{n1}x{n2}"] = (lambda b=baby, g=giant, e=enc: self.leg_a(b, g, e))
            out[f"B_{n1}x{n2}"] = (lambda b=baby, g=giant, e=enc: self.leg_b(b, g, e))
        return out

    def slots(self, ct):
        return tf.ckks_decode(tf.decrypt(self.kp, ct), ct.scale).real.reshape(self.batch, DIM, self.block)

    def check(self):
        """the words of B against the composition; the decryptions of A and B against W @ x + b"""
        worst = {}
        for (n1, n2), (baby, giant, enc, Ds) in self.splits.items():
            got = self.leg_b(baby, giant, enc)
            rots = [r for c in self.cs for r in [c] + list(tf.rotate_many(baby, c))]
            rows = []                                          # [n_in][n2 n1] single elements, to broadcast
            for D in Ds:
                flat = D.reshape(-1, self.N // 2).astype(complex)
                rows.append([tf.ckks_encode(flat[r], self.R, self.scale) for r in range(flat.shape[0])])
            want = None
            for j in range(n2):
                inner = tf.CipherText.dot_plain(rots, [d.broadcast_to(self.batch) for rm in rows for d in rm[j * n1:(j + 1) * n1]])
                want = inner if j == 0 else want + tf.rotate(giant[j - 1], inner)
            want = tf.CipherText(want.params, (want.cs[0] + self.bias_b,) + tuple(want.cs[1:]), want.scale)
            for a, b in zip(got.cs, want.cs):
                assert np.array_equal(a.to_numpy(), b.to_numpy()), f"tfhe_matmul_bsgs_blocks ({n1}, {n2}) differs from the composition"
            worst[f"{n1}x{n2}"] = {"A": float(np.abs(self.slots(self.leg_a(baby, giant, enc)) - self.want).max()),
                                   "B": float(np.abs(self.slots(got) - self.want).max())}
        return worst

    def time_leg(self, f, min_s):
        """milliseconds per layer from device events around >= min_s seconds of enqueued work"""
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
    ap.add_argument("--configs", default="ref13,fp14,ref16")
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
        row = {"config": name, "N": case.N, "batch": a.batch, "limbs": case.R.L, "layer": f"{DIM} x {DIM * N_IN}", "inputs": N_IN, "rounds": a.rounds,
               "unit": "ms per layer over the batch", "max_slot_difference_to_plain": diff}
        row.update({k: summary(v) for k, v in ms.items()})
        for n1, n2 in SPLITS:
            s = f"{n1}x{n2}"
            row[f"noise_band_{s}"] = abs(row[f"A_b_{s}"]["median"] / row[f"A_a_{s}"]["median"] - 1.0)
            row[f"B_over_A_{s}"] = row[f"B_{s}"]["median"] / row[f"A_a_{s}"]["median"]
            row[f"B_faster_beyond_noise_{s}"] = bool(1.0 - row[f"B_over_A_{s}"] > row[f"noise_band_{s}"])
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
