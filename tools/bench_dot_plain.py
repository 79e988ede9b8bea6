#!/usr/bin/env python3
"""The accumulation of the diagonal matrix product (infer.jl:140-149: 63 rotated ciphertexts times 63 plaintext diagonals, both
components), in one process, alternated:
  call       CipherText.dot_plain through tfhe_dot_plain (the default): one call per component on view operands -- under test
  parent_a   the same with the switch off (TFHE_DOT_PLAIN_CALL=0): the mirror's staging copies, one tfhe_nntt per chunk and
  parent_b   tfhe_dot, which is what the parent commit ran -- the baseline, timed TWICE per round: parent_b against parent_a is the
             noise band of the comparison
The operands are unsplit key-switch results (packed [batch][2][limbs][N] buffers in the coefficient domain, as chained rotations leave
them); the plaintexts are transformed already.  Before timing, the words of `call` and `parent` are compared.  Device events around
at least `--min-s` seconds of work per leg and round; the legs take turns round by round; medians and spreads are reported.
`--mnist` adds the reference-shaped pass of examples/encrypted_mnist.py (N = 2^16, 16 ciphertext sets, one Galois key, chained
rotations) with the call and, twice, without (the same noise band), alternated, device span of the last of three passes.

usage: bench_dot_plain.py [--configs fp13,fp14,mix13,mix14,ref16] [--terms 63] [--batch 16] [--rounds 5] [--min-s 0.3] [--mnist 2]
                          [--json profiles/dot_plain_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np  # noqa: E402

import toyfhe_jl_amd as tf  # noqa: E402
from toyfhe_jl_amd import native, she  # noqa: E402


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
    # name: (log2 N, moduli, special prime, path)
    "fp13": (13, lambda N: chain(2**50 + 1, 3, N), False, "fused (fp64 policy)"),
    "fp14": (14, lambda N: chain(2**50 + 1, 3, N), False, "fused (fp64 policy)"),
    "mix13": (13, lambda N: chain(2**60 + 1, 1, N) + chain(2**40 + 1, 1, N), False, "fused (two lanes)"),
    "mix14": (14, lambda N: chain(2**60 + 1, 1, N) + chain(2**40 + 1, 1, N), False, "fused (two lanes)"),
    "ref16": (16, reference_ring, True, "composed"),
}


class switch:
    """the mirror with the call on / off (she reads the module flags at every call; the environment sets them at import)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = (she._DOT_PLAIN_CALL, she._DOT_PLAIN_CALL_MAX_LOG2)
        she._DOT_PLAIN_CALL, she._DOT_PLAIN_CALL_MAX_LOG2 = self.on, 17     # the call at every size: this tool is what sets the mirror's bound

    def __exit__(self, *a):
        she._DOT_PLAIN_CALL, she._DOT_PLAIN_CALL_MAX_LOG2 = self.old


def copies(ctx, host, n):
    """n device buffers with the words of `host` (one upload, device copies: distinct addresses, so nothing stays in a cache)"""
    first = tf.DeviceBuffer.from_numpy(host)
    out = [first]
    for _ in range(n - 1):
        b = tf.DeviceBuffer(first.n)
        native.check(native.lib().tfhe_memcpy_d2d(ctx.h, b.ptr, first.ptr, first.n * 8))
        out.append(b)
    return out


class Case:
    def __init__(self, name, terms, batch):
        logn, mk, special, self.path = CONFIGS[name]
        self.name, self.N, self.batch, self.terms = name, 1 << logn, batch, terms
        ring = tf.NegacyclicRing(self.N, mk(self.N))
        inner = tf.CKKSParams(ring, 0, 3.2)
        params = tf.ModulusRaised(inner) if special else inner
        rc = params.R_cipher()
        self.ctx, self.level = rc.ctx, rc.L
        rng = np.random.default_rng(3)
        res = lambda prefix: np.stack([rng.integers(0, q, size=prefix + (self.N,), dtype=np.uint64) for q in rc.moduli], axis=len(prefix))
        images = copies(self.ctx, res((batch, 2)), terms)
        self.cts = [she._PackedResult(params, 2**40, im, self.ctx, rc, batch, batch) for im in images]
        self.pts = [tf.RingElement(rc, None, b, batch) for b in copies(self.ctx, res((batch,)), terms)]

    def run(self, on):
        with switch(on):
            return tf.CipherText.dot_plain(self.cts, self.pts)

    def legs(self):
        return {"call": lambda: self.run(True), "parent_a": lambda: self.run(False), "parent_b": lambda: self.run(False)}

    def check(self):
        on, off = self.run(True), self.run(False)
        for x, y in zip(on.cs, off.cs):
            assert np.array_equal(x.to_numpy("dual"), y.to_numpy("dual")), "tfhe_dot_plain differs from the staging route"
        assert all(c._cs is None for c in self.cts)

    def time_leg(self, f, min_s):
        """milliseconds per dot_plain (both components) from device events around >= min_s seconds of enqueued work"""
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
        return e0.elapsed_ms(e1) / reps


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v)}


def mnist(rounds):
    """the reference-shaped pass (tools/bench_configs.py mnist_case, reference_shape): device span of the last of three passes, ms"""
    import encrypted_mnist as em
    spans = {"call": [], "parent_a": [], "parent_b": []}
    for _ in range(rounds):
        for leg, on in (("call", True), ("parent_a", False), ("parent_b", False)):   # the parent twice: its noise band
            st = {}
            with switch(on):
                em.run(16, 0, verbose=False, batches=16, hoisted=False, repeat=3, fused=False, stats=st)
            spans[leg].append(st["device_span_s"] * 1e3)
    row = {"config": "mnist16 reference-shaped pass", "unit": "ms (device span of the last of three passes)", "rounds": rounds}
    row.update({k: summary(v) for k, v in spans.items()})
    row["call_over_parent"] = row["call"]["median"] / row["parent_a"]["median"]
    row["noise_band"] = abs(row["parent_b"]["median"] / row["parent_a"]["median"] - 1.0)
    row["call_not_slower"] = row["call_over_parent"] <= 1.0 + row["noise_band"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="fp13,fp14,mix13,mix14,ref16")
    ap.add_argument("--terms", type=int, default=63)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.3)
    ap.add_argument("--mnist", type=int, default=0, help="rounds of the reference-shaped MNIST pass per leg (0: skip)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    results = []
    for name in [c for c in a.configs.split(",") if c]:
        case = Case(name, a.terms, a.batch)
        case.check()
        legs = case.legs()
        for f in legs.values():                               # warm-up: workspaces, staging buffers, allocator
            for _ in range(2):
                f()
        case.ctx.sync()
        ms = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, f in legs.items():                         # alternated
                ms[k].append(case.time_leg(f, a.min_s))
        row = {"config": name, "N": case.N, "batch": a.batch, "terms": a.terms, "limbs": case.level, "path": case.path, "rounds": a.rounds,
               "unit": "ms per dot_plain (both components)"}
        row.update({k: summary(v) for k, v in ms.items()})
        row["call_over_parent"] = row["call"]["median"] / row["parent_a"]["median"]
        row["noise_band"] = abs(row["parent_b"]["median"] / row["parent_a"]["median"] - 1.0)
        row["call_not_slower"] = row["call_over_parent"] <= 1.0 + row["noise_band"]
        results.append(row)
        print(json.dumps(row), flush=True)
        she.release_staging(case.ctx)
        del case, legs
    if a.mnist:
        row = mnist(a.mnist)
        results.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump({"results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
