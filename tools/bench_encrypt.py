#!/usr/bin/env python3
"""Encryptions and decryption phases per second, in one process, alternated:
  enc_call / dec_call   tfhe_encrypt / tfhe_decrypt_phase on packed device buffers        -- the calls under test
  enc_on   / dec_on     she.encrypt / she._decryption through the calls (the default)     -- what a caller of the mirror pays now
  enc_off  / dec_off    the same with the switch off (TFHE_FUSED_ENCRYPT=0): the term-by-term composition on ring elements the
                        parent commit ran                                                 -- baseline
Before timing, the residues of enc_on and enc_off (same generator seed) and of dec_on and dec_off are compared word for word.
Device events around at least `--min-s` seconds of work per leg and round; the legs take turns round by round so that clock and
thermal drift hit all alike; the spread over the rounds is reported next to the median.

usage: bench_encrypt.py [--configs n14,ref16] [--batches 16,256] [--rounds 5] [--min-s 0.5] [--json profiles/encrypt_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    # name: (log2 N, moduli, special prime, path)
    "n14": (14, lambda N: chain(2**50 + 1, 8, N), False, "fused (fp64 policy)"),
    "ref16": (16, reference_ring, True, "composed"),
}


class switch:
    """the mirror with the device calls on / off (she reads the module flag at every call; the environment sets it at import)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old, she._FUSED_ENCRYPT = she._FUSED_ENCRYPT, self.on

    def __exit__(self, *a):
        she._FUSED_ENCRYPT = self.old


class Case:
    def __init__(self, name, batch):
        logn, mk, special, self.path = CONFIGS[name]
        self.name, self.N, self.batch = name, 1 << logn, batch
        qs = mk(self.N)
        ring = tf.NegacyclicRing(self.N, qs)
        inner = tf.CKKSParams(ring, 0, 3.2)
        self.params = tf.ModulusRaised(inner) if special else inner
        self.kp = tf.keygen(tf.DeviceRng(11), self.params)
        rc = self.params.R_cipher()
        self.Lk, self.level, self.ctx = len(qs), rc.L, ring.ctx
        x = np.tile(np.linspace(-1, 1, self.N // 2), (batch, 1)).astype(complex)
        self.msg = tf.ckks_encode(x, rc, 2**40)
        self.pk = she._packed_pubkey(self.kp.pub, ring)
        self.secret = self.kp.priv.secret.coeffs_dual()
        self.out = tf.DeviceBuffer(batch * 2 * self.level * self.N)
        self.b = tf.DeviceBuffer(batch * self.level * self.N)
        self.ct = self.mirror_encrypt(True)

    def mirror_encrypt(self, on, seed=5):
        with switch(on):
            return tf.encrypt(tf.DeviceRng(seed), self.kp, self.msg, scale=2**40)

    def mirror_decrypt(self, on):
        with switch(on):
            return she._decryption(self.kp, tf.CipherText(self.params, self.ct.cs, self.ct.scale))[1]

    def enc_call(self):
        self.ctx.encrypt(self.Lk, self.level, self.pk.ptr, self.out.ptr, self.batch, msg=self.msg.coeffs_primal().ptr, sigma_u=3.2, sigma_e=3.2,
                         seed=5, first_poly=0)

    def dec_call(self):
        self.ctx.decrypt_phase(self.Lk, self.level, self.secret.ptr, self.out.ptr, 2, self.b.ptr, self.batch)

    def legs(self):
        return {"enc_call": self.enc_call, "enc_on": lambda: self.mirror_encrypt(True), "enc_off": lambda: self.mirror_encrypt(False),
                "dec_call": self.dec_call, "dec_on": lambda: self.mirror_decrypt(True).coeffs_primal(),
                "dec_off": lambda: self.mirror_decrypt(False).coeffs_primal()}

    def check(self):
        on, off = self.mirror_encrypt(True), self.mirror_encrypt(False)
        for x, y in zip(on.cs, off.cs):
            assert np.array_equal(x.to_numpy(), y.to_numpy()), "the fused encryption differs from the composition"
        self.enc_call()
        got = self.out.to_numpy((self.batch, 2, self.level, self.N))
        assert all(np.array_equal(got[:, p], on.cs[p].to_numpy()) for p in range(2)), "tfhe_encrypt differs from the mirror"
        assert np.array_equal(self.mirror_decrypt(True).to_numpy(), self.mirror_decrypt(False).to_numpy()), "the decryption phases differ"
        self.dec_call()
        assert np.array_equal(self.b.to_numpy((self.batch, self.level, self.N)), self.mirror_decrypt(True).to_numpy())

    def time_leg(self, f, min_s):
        """ciphertexts per second from device events around >= min_s seconds of enqueued work"""
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
        return self.batch * reps / (e0.elapsed_ms(e1) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="n14,ref16")
    ap.add_argument("--batches", default="16,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    results = []
    for name in a.configs.split(","):
        for batch in (int(b) for b in a.batches.split(",")):
            case = Case(name, batch)
            case.check()
            legs = case.legs()
            for f in legs.values():                           # warm-up: workspaces, key images, allocator
                for _ in range(2):
                    f()
            case.ctx.sync()
            rates = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, f in legs.items():                     # alternated
                    rates[k].append(case.time_leg(f, a.min_s))
            row = {"config": name, "N": case.N, "batch": batch, "level": case.level, "key_limbs": case.Lk, "path": case.path, "rounds": a.rounds}
            for k, v in rates.items():
                row[k] = {"median_per_s": statistics.median(v), "min_per_s": min(v), "max_per_s": max(v),
                          "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v)}
            for kind in ("enc", "dec"):
                row[kind + "_on_over_off"] = row[kind + "_on"]["median_per_s"] / row[kind + "_off"]["median_per_s"]
                row[kind + "_call_over_off"] = row[kind + "_call"]["median_per_s"] / row[kind + "_off"]["median_per_s"]
            results.append(row)
            print(json.dumps(row), flush=True)
            del case
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump({"unit": "ciphertexts per second (encryptions; decryption phases)", "results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
