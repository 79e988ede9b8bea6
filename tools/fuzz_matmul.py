#!/usr/bin/env python3
"""Random rings for tfhe_matmul_diag at N = 2^10 .. 2^16 (one to six ciphertext limbs of 30 / 40 / 50 / 60 bits in any mix, special
prime of 40 / 50 / 60 bits or none, one to eight rotations, batch 1-4): the product against rotate_many + dot_plain, word for word
(the evaluation-domain form against the coefficient-domain path: fused and unfused lifts, both masked walks, every policy split).
With --oracle every fourth shape up to N = 2^14 is also run through the raw C ABI on uniform residues and keys -- tfhe_matmul_diag and,
with the rotations split into baby and giant steps and the ciphertext given twice, tfhe_matmul_bsgs_blocks -- against the host reference
tests/matmul_oracle.py (the C oracle's key switch and transforms, exact integer sums), so that the run is not device against device only.
About five minutes on the GPU box.  usage: python tools/fuzz_matmul.py [--oracle] [first-seed] [seconds]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toyfhe_jl_amd as tf

ORACLE = "--oracle" in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a != "--oracle"]
S0 = int(argv[0]) if len(argv) > 0 else 0
budget = float(argv[1]) if len(argv) > 1 else 300.0
ORACLE_EVERY, ORACLE_MAX_LOGN = 4, 14


def oracle_check(seed, N, qs, raised, level, n_rot, batch):
    """the shape of this seed through the raw ABI against tests/matmul_oracle.py: matmul_diag over n_rot rotations, and the block-row
    product with the same keys split into baby and giant steps over two inputs and a bias"""
    from oracle import ref_cpu
    from tests import helpers as H
    from tests import matmul_oracle as MO
    rs = np.random.default_rng(10**6 + seed)
    Lk, batch = len(qs), batch or 1
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    cq = qs[:level]
    gs = [pow(3, int(k), 2 * N) for k in rs.choice(np.arange(1, N // 2), n_rot, replace=False)]
    keys = [H.uniform_evk(rs, qs, Lk, N) for _ in gs]
    prep = []
    for k, g in zip(keys, gs):
        d, p = tf.DeviceBuffer.from_numpy(k), tf.DeviceBuffer(k.size)
        ctx.galois_key_prepare(Lk, Lk, g, d.ptr, p.ptr)
        prep.append(p)
    cts = [H.rand_residues(rs, cq, (batch, 2), N) for _ in range(2)]
    dcts = [tf.DeviceBuffer.from_numpy(c) for c in cts]
    out = tf.DeviceBuffer(batch * 2 * level * N)
    diags = H.rand_residues(rs, cq, (n_rot + 1,), N)
    ddiag = tf.DeviceBuffer.from_numpy(diags)
    ctx.matmul_diag(Lk, level, raised, [p.ptr for p in prep], Lk, gs, ddiag.ptr, dcts[0].ptr, out.ptr, batch)
    ok = np.array_equal(out.to_numpy((batch, 2, level, N)), MO.matmul_diag_ref(ref, level, raised, keys, gs, diags, cts[0]))
    nb = n_rot // 2
    ng = n_rot - nb
    bd = H.rand_residues(rs, cq, (2, ng + 1, nb + 1), N)
    bias = H.rand_residues(rs, cq, (), N)
    dbd, dbias = [tf.DeviceBuffer.from_numpy(d) for d in bd], tf.DeviceBuffer.from_numpy(bias)
    ctx.matmul_bsgs_blocks(Lk, level, raised, [p.ptr for p in prep[:nb]], gs[:nb], [p.ptr for p in prep[nb:]], gs[nb:], Lk,
                           [d.ptr for d in dbd], [c.ptr for c in dcts], dbias.ptr, out.ptr, batch)
    want = MO.matmul_bsgs_blocks_ref(ref, level, raised, keys[:nb], gs[:nb], keys[nb:], gs[nb:], bd, cts, bias)
    return ok and np.array_equal(out.to_numpy((batch, 2, level, N)), want)


t0, bad, n, n_oracle = time.time(), [], 0, 0
for seed in range(S0, S0 + 100000):
    if time.time() - t0 > budget:
        break
    rs = np.random.default_rng(seed)
    logn = int(rs.choice([10, 12, 13, 14, 15, 16, 16])); N = 1 << logn
    L = int(rs.integers(1, 7)); raised = bool(rs.integers(0, 5))
    qs, used = [], set()
    for k in range(L + (1 if raised else 0)):
        bits = int(rs.choice([40, 50, 60])) if (raised and k == L) else int(rs.choice([30, 40, 50, 60]))
        q = tf.nextprime(2 ** bits + 1, 1, 2 * N)
        while q in used:
            q = tf.nextprime(q + 2 * N, 1, 2 * N)
        used.add(q); qs.append(q)
    desc = (seed, logn, [q.bit_length() for q in qs], raised)
    try:
        params = tf.CKKSParams(tf.NegacyclicRing(N, qs), 0, 3.2)
        if raised:
            params = tf.ModulusRaised(params)
        rng = tf.DeviceRng(seed)
        kp = tf.keygen(rng, params)
        n_rot = int(rs.integers(1, 9)); batch = [None, 2, 3, 4][int(rs.integers(0, 4))]
        shape = (N // 2,) if batch is None else (batch, N // 2)
        scale = 2 ** 20
        c = tf.encrypt(rng, kp, tf.ckks_encode(rs.normal(0, 1, shape).astype(complex), params.R_cipher(), scale), scale=scale)
        if L > 1 and rs.integers(0, 2):
            c = tf.modswitch(c)                           # a lower level of the same keys
        gks = tf.keygen_galois_many(rng, kp.priv, steps=[int(k) for k in rs.choice(np.arange(1, N // 2), n_rot, replace=False)])
        dv = rs.normal(0, 1, (n_rot + 1, N // 2)).astype(complex)
        singles = [tf.ckks_encode(dv[k], c.ring(), scale) for k in range(n_rot + 1)]
        want = tf.CipherText.dot_plain([c] + list(tf.rotate_many(gks, c)), [d if batch is None else d.broadcast_to(batch) for d in singles])
        got = tf.matmul_diag(gks, singles, c)
        ok = all(np.array_equal(a.to_numpy("dual"), b.to_numpy("dual")) for a, b in zip(got.cs, want.cs))
        if ok and ORACLE and seed % ORACLE_EVERY == 0 and logn <= ORACLE_MAX_LOGN:
            n_oracle += 1
            if not oracle_check(seed, N, qs, raised, c.ring().L, n_rot, batch):
                ok = False; desc = desc + ("oracle",)
    except Exception as e:  # noqa: BLE001
        ok = False; desc = desc + (repr(e)[:200],)
    n += 1
    if not ok:
        bad.append(desc); print("FAIL", desc, flush=True)
print(f"{n} cases from seed {S0}" + (f" ({n_oracle} of them also against tests/matmul_oracle.py)" if ORACLE else "") + f"; failures: {bad}")
