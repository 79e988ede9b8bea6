"""Device plaintext codecs (tfhe_plain_decode / tfhe_plain_encode / tfhe_bfv_noise_max) on the headline ring -- N = 2^14,
L = 8 primes of 50 bits, t = 65537, a batch of 1024 -- against the host code they replace (the Python big-integer loops of
she.BFVParams._host_decode, the per-coefficient encode and the host noise maximum), timed at batch 2 and extrapolated.
Writes one JSON line (default profiles/plain_codec_bench.json) and prints it.

    python tools/plain_codec_bench.py [--batch 1024] [--reps 5] [--host-batch 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toyfhe_jl_amd as tf  # noqa: E402
from toyfhe_jl_amd.she import _map_plain  # noqa: E402


def chain(bits, n, N):
    out, p = [], tf.nextprime(2**bits + 1, 1, 2 * N)
    for _ in range(n):
        out.append(p)
        p = tf.nextprime(p + 2 * N, 1, 2 * N)
    return out


def device_ms(ctx, fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = tf.Event(), tf.Event()
        a.record(ctx)
        fn()
        b.record(ctx)
        times.append(a.elapsed_ms(b))
    return statistics.median(times), min(times)


def host_s(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=14)
    ap.add_argument("--limbs", type=int, default=8)
    ap.add_argument("--t", type=int, default=65537)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-batch", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plain_codec_bench.json"))
    a = ap.parse_args()
    N, L, t, B = 1 << a.logn, a.limbs, a.t, a.batch
    R = tf.NegacyclicRing(N, chain(50, L, N))
    params = tf.BFVParams(R, R, t)
    ctx = R.ctx
    plan = tf.PlainPlan(ctx, t)
    src = tf.DeviceBuffer(B * L * N)
    ctx.sample_uniform(L, 2024, 0, 0, src.ptr, B)
    dec = tf.DeviceBuffer(B * N)
    m = np.random.default_rng(1).integers(0, t, size=(B, N), dtype=np.uint64)
    dm = tf.DeviceBuffer.from_numpy(m)
    enc = tf.DeviceBuffer(B * L * N)
    words = tf.DeviceBuffer(B * plan.delta_words)
    d_dec = device_ms(ctx, lambda: plan.decode(tf.native.PLAIN_BFV, src.ptr, dec.ptr, B), a.reps)
    d_bgv = device_ms(ctx, lambda: plan.decode(tf.native.PLAIN_BGV, src.ptr, dec.ptr, B), a.reps)
    d_enc = device_ms(ctx, lambda: plan.encode(tf.native.PLAIN_BFV, dm.ptr, enc.ptr, B), a.reps)
    d_noise = device_ms(ctx, lambda: plan.noise_max(src.ptr, words.ptr, B), a.reps)
    ctx.sync()

    # the host paths these replace, on the first host-batch elements
    hb = a.host_batch
    res = np.empty((hb, L, N), dtype=np.uint64)
    tf.native.check(tf.native.lib().tfhe_memcpy_d2h(res.ctypes.data, src.ptr, res.nbytes))
    el = R.from_residues(res)
    h_dec = host_s(lambda: params._host_decode(el))
    delta = params.delta
    plain = m[:hb].tolist()
    h_enc = host_s(lambda: R(_map_plain(plain, lambda x: delta * (int(x) % t))))

    def host_noise():
        for row in el.to_ints():
            max((delta - x % delta) if x % delta > delta // 2 else x % delta for x in row)
    h_noise = host_s(host_noise)
    # the device result agrees with the host on those elements
    assert params.decode(el) == params._host_decode(el)

    gib_in = B * L * N * 8 / 2**30
    line = {
        "workload": "bfv plaintext codec", "N": N, "limbs": L, "q_bits": 50, "t": t, "batch": B,
        "device_decode_ms": round(d_dec[0], 3), "device_decode_min_ms": round(d_dec[1], 3),
        "device_bgv_decode_ms": round(d_bgv[0], 3),
        "device_encode_ms": round(d_enc[0], 3), "device_noise_max_ms": round(d_noise[0], 3),
        "device_decode_GBps": round(gib_in * 2**30 / 1e9 / (d_dec[0] / 1e3), 1),
        "host_batch": hb,
        "host_decode_s_per_elem": round(h_dec / hb, 4), "host_encode_s_per_elem": round(h_enc / hb, 4),
        "host_noise_s_per_elem": round(h_noise / hb, 4),
        "host_decode_s_extrapolated": round(h_dec / hb * B, 1), "host_encode_s_extrapolated": round(h_enc / hb * B, 1),
        "host_noise_s_extrapolated": round(h_noise / hb * B, 1),
        "decode_speedup": round(h_dec / hb * B / (d_dec[0] / 1e3)),
    }
    s = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(s + "\n")
    print(s)


if __name__ == "__main__":
    main()
