#!/usr/bin/env python3
"""Key generation -- the relinearisation key plus `--galois` Galois keys of one parameter set -- in one process, alternated:
  call       she.keygen_evalmult + she.keygen_galois_many through tfhe_evalkey_gen (the default)          -- the call under test
  composed   the kept composition on ring elements (she._keygen_evalmult_composed, _keygen_galois_composed): what the parent
             commit's keygen_evalmult / keygen_galois loop ran                                             -- baseline
Before timing, the packed words of every key of both legs (same generator seed) are compared word for word, and the generator
states afterwards.  Key generation is host-driven (the composition reads an element back per key), so a leg is timed on the host's
clock between two stream synchronisations; the legs take turns round by round so that clock and thermal drift hit both alike; the
spread over the rounds is reported next to the median; a leg shorter than half a second is repeated within its round until it has
run that long.  One counting pass per leg reports the C-ABI calls made (each is at least
one launch or copy) and the bytes moved between host and device.

usage: bench_keygen.py [--configs n14,ref16] [--galois 63] [--rounds 5] [--json profiles/keygen_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    "n14": (14, lambda N: chain(2**50 + 1, 8, N), False, "fused (fp64 policy)"),
    "ref16": (16, reference_ring, True, "composed"),
}


class counting:
    """count the C-ABI calls and the host <-> device bytes while the block runs (not used while timing)"""

    def __enter__(self):
        self.calls, self.h2d, self.d2h = {}, 0, 0
        self.lib = native.lib()
        self.saved = {}
        for name in native.EXPORTED_SYMBOLS:
            if name in ("tfhe_last_error", "tfhe_malloc", "tfhe_free", "tfhe_ctx_sync"):
                continue
            f = getattr(self.lib, name)
            self.saved[name] = f
            setattr(self.lib, name, self.wrap(name, f))
        return self

    def wrap(self, name, f):
        def g(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            if name == "tfhe_memcpy_h2d":
                self.h2d += int(a[2])
            elif name == "tfhe_memcpy_d2h":
                self.d2h += int(a[2])
            return f(*a)
        return g

    def __exit__(self, *a):
        for name, f in self.saved.items():
            setattr(self.lib, name, f)

    def summary(self):
        return {"abi_calls": sum(self.calls.values()), "h2d_bytes": self.h2d, "d2h_bytes": self.d2h,
                "by_symbol": dict(sorted(self.calls.items(), key=lambda kv: -kv[1])[:6])}


class Case:
    def __init__(self, name, n_galois):
        logn, mk, special, self.path = CONFIGS[name]
        self.name, self.N = name, 1 << logn
        qs = mk(self.N)
        ring = tf.NegacyclicRing(self.N, qs)
        inner = tf.CKKSParams(ring, 0, 3.2)
        self.params = tf.ModulusRaised(inner) if special else inner
        self.ctx, self.Lk = ring.ctx, len(qs)
        self.kp = tf.keygen(tf.DeviceRng(11), self.params)
        self.steps = list(range(1, n_galois + 1))

    def call(self, seed=5):
        rng = tf.DeviceRng(seed)
        keys = [tf.keygen_evalmult(rng, self.kp.priv).key] + [g.key for g in tf.keygen_galois_many(rng, self.kp.priv, steps=self.steps)]
        return keys, rng.next_poly

    def composed(self, seed=5):
        rng = tf.DeviceRng(seed)
        keys = [she._keygen_evalmult_composed(rng, self.kp.priv).key]
        keys += [she._keygen_galois_composed(rng, self.kp.priv, steps=st).key for st in self.steps]
        for k in keys:
            k.packed()                                       # the composition's keys are not usable before they are packed
        return keys, rng.next_poly

    def check(self):
        (a, sa), (b, sb) = self.call(), self.composed()
        assert sa == sb, "the generator states differ"
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x.packed().to_numpy(), y.packed().to_numpy()), f"key {i}: the call differs from the composition"

    def time_leg(self, f, min_seconds=0.5):
        """seconds per pass: passes are repeated until the leg has run for min_seconds, so that a short leg is not one host-clock
        reading (a pass's keys are dropped before the next one starts, as a caller's would be)"""
        self.ctx.sync()
        passes, t0 = 0, time.perf_counter()
        while True:
            keys, _ = f()
            self.ctx.sync()
            del keys
            passes += 1
            dt = time.perf_counter() - t0
            if dt >= min_seconds:
                return dt / passes

    def count_leg(self, f):
        with counting() as c:
            keys, _ = f()
            self.ctx.sync()
        del keys
        return c.summary()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="n14,ref16")
    ap.add_argument("--galois", type=int, default=63)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert she._FUSED_KEYGEN, "TFHE_FUSED_KEYGEN=0 turns the leg under test into the baseline"
    she._FUSED_KEYGEN_MAX_LOG2 = 17                           # the call at every size: this is what decides the mirror's routing
    results = []
    for name in a.configs.split(","):
        case = Case(name, a.galois)
        case.check()
        legs = {"call": case.call, "composed": case.composed}
        for f in legs.values():                               # warm-up: workspaces, allocator
            case.time_leg(f)
        secs = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, f in legs.items():                         # alternated
                secs[k].append(case.time_leg(f))
        row = {"config": name, "N": case.N, "key_limbs": case.Lk, "keys": 1 + a.galois, "path": case.path, "rounds": a.rounds}
        for k, v in secs.items():
            row[k] = {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v),
                      "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v), **case.count_leg(legs[k])}
        row["composed_over_call"] = row["composed"]["median_s"] / row["call"]["median_s"]
        results.append(row)
        print(json.dumps(row), flush=True)
        del case
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump({"unit": "seconds per key set (relinearisation key + Galois keys), host clock", "results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
