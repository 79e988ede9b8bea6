"""The BFV / BGV plaintext codecs and the BFV noise maximum on the MI355X (tfhe_plain_*, tfhe_bfv_noise_max) against the
oracle (spec.bfv_decode / bgv_decode / bfv_encode) and the host mirror they replace (she.BFVParams._host_decode ...)."""
import math
import random

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import spec
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _fetch_rows(buf, row_words, rows):
    out = np.empty((len(rows), row_words), dtype=np.uint64)
    for k, b in enumerate(rows):
        tf.native.check(tf.native.lib().tfhe_memcpy_d2h(out[k].ctypes.data, buf.ptr + b * row_words * 8, row_words * 8))
    return out


def _oracle_sample(res, qs, t, picks):
    """spec decodes of coefficients `picks` of residues [L][N]"""
    ring = spec.Ring(len(picks), qs, [1] * len(qs))
    poly = [[int(res[l, k]) for k in picks] for l in range(len(qs))]
    return spec.bfv_decode(poly, ring, t), spec.bgv_decode(poly, ring, t)


def _host_budget(ints, params):
    """she.invariant_noise_budget's host formula (bfv.jl:137-166) over the coefficients of b"""
    delta = params.delta
    worst = max((delta - x % delta) if x % delta > delta // 2 else x % delta for x in ints)
    return math.log2(params.ring.modulus()) - math.log2(params.t) - 1 - (math.log2(worst) if worst else 0.0)


@pytest.mark.parametrize("logn", range(10, 17))
def test_decode_encode_match_oracle_over_degrees(logn):
    N, t = 1 << logn, 65537
    qs = H.chain(50, 3, N)
    R = tf.NegacyclicRing(N, qs)
    bfv, bgv = tf.BFVParams(R, R, t), tf.BGVParams(R, t)
    rng = np.random.default_rng(logn)
    res = H.rand_residues(rng, qs, (2,), N)
    el = R.from_residues(res)
    picks = sorted(set(rng.integers(0, N, size=48).tolist()) | {0, N - 1})
    got_bfv, got_bgv = bfv.decode_array(el), bgv.decode_array(el)
    assert got_bfv.shape == (2, N) and got_bfv.dtype == np.uint64
    for b in range(2):
        wb, wg = _oracle_sample(res[b], qs, t, picks)
        assert got_bfv[b, picks].tolist() == wb and got_bgv[b, picks].tolist() == wg
    if logn <= 12:                                                  # the whole host mirror
        assert bfv.decode(el) == bfv._host_decode(el) and bgv.decode(el) == bgv._host_decode(el)
    m = rng.integers(-3 * t, 3 * t, size=(2, N), dtype=np.int64)
    for params, want in ((bfv, lambda row: spec.bfv_encode(row, spec.Ring(N, qs, [1] * 3), t)),
                         (bgv, lambda row: [[x % t % q for x in row] for q in qs])):
        enc = params.encode(m.tolist())
        assert enc.batch == 2
        got = enc.to_numpy()
        for b in range(2):
            assert got[b].tolist() == want([int(x) for x in m[b]])


def test_non_prefix_limbs_and_mixed_ring():
    N, t = 1 << 12, 65537
    q0, ps = H.chain(60, 2, N)
    qs = [q0] + H.chain(40, 3, N) + [ps]                              # the mixed 60 / 40-bit ring (infer.jl:97-112)
    R = tf.NegacyclicRing(N, qs)
    rng = np.random.default_rng(5)
    for which in ([4, 0, 2], [1, 2, 3], list(range(5))):
        Rs = R.crtselect(which)
        sq = Rs.moduli
        res = H.rand_residues(rng, sq, (3,), N)
        el = Rs.from_residues(res)
        picks = list(range(0, N, 97))
        for tt in (t, 2, 256):
            bfv, bgv = tf.BFVParams(Rs, Rs, tt), tf.BGVParams(Rs, tt)
            gb, gg = bfv.decode_array(el), bgv.decode_array(el)
            for b in range(3):
                wb, wg = _oracle_sample(res[b], sq, tt, picks)
                assert gb[b, picks].tolist() == wb and gg[b, picks].tolist() == wg
        plan = tf.PlainPlan(R.ctx, t, which)
        m = rng.integers(0, 2**63, size=(3, N), dtype=np.uint64)
        dm, out = tf.DeviceBuffer.from_numpy(m), tf.DeviceBuffer(3 * len(which) * N)
        plan.encode(tf.native.PLAIN_BFV, dm.ptr, out.ptr, 3)
        R.ctx.sync()
        got = out.to_numpy((3, len(which), N))
        Q = 1
        for q in sq:
            Q *= q
        delta = Q // t
        for b in range(3):
            for k in picks:
                assert [int(v) for v in got[b, :, k]] == [delta * (int(m[b, k]) % t) % q for q in sq]
        plan.close()


def test_headline_batches_and_user_stream():
    torch = pytest.importorskip("torch")
    N, L, t = 1 << 14, 8, 65537
    qs = H.chain(50, L, N)
    R = tf.NegacyclicRing(N, qs)
    plan = tf.PlainPlan(R.ctx, t)
    bfv = tf.BFVParams(R, R, t)
    src = tf.DeviceBuffer(1024 * L * N)
    R.ctx.sample_uniform(L, 77, 0, 0, src.ptr, 1024)
    out = tf.DeviceBuffer(1024 * N)
    plan.decode(tf.native.PLAIN_BFV, src.ptr, out.ptr, 0)             # an empty batch does nothing
    rng = random.Random(9)
    for batch in (1, 7, 1024):
        plan.decode(tf.native.PLAIN_BFV, src.ptr, out.ptr, batch)
        R.ctx.sync()
        rows = sorted({0, batch - 1} | {rng.randrange(batch) for _ in range(3)})
        got, res = _fetch_rows(out, N, rows), _fetch_rows(src, L * N, rows).reshape(len(rows), L, N)
        picks = sorted(rng.sample(range(N), 24))
        for i in range(len(rows)):
            assert got[i, picks].tolist() == _oracle_sample(res[i], qs, t, picks)[0]
    # the full host mirror at batch 2
    res2 = _fetch_rows(src, L * N, [0, 1]).reshape(2, L, N)
    el = R.from_residues(res2)
    assert bfv.decode(el) == bfv._host_decode(el)
    # a caller's non-blocking stream: the same results
    full = out.to_numpy((1024, N))
    side = torch.cuda.Stream()
    R.ctx.set_stream(side.cuda_stream)
    try:
        out2 = tf.DeviceBuffer(1024 * N)
        plan.decode(tf.native.PLAIN_BFV, src.ptr, out2.ptr, 1024)
        R.ctx.sync()
        assert np.array_equal(out2.to_numpy((1024, N)), full)
    finally:
        R.ctx.set_stream(None)
    plan.close()


def test_bfv_round_trip_mul_relin_batch():
    N, t, batch = 1 << 14, 65537, 64
    ch = H.chain(50, 7, N)
    Rbig = tf.NegacyclicRing(N, ch)
    R = Rbig.crtselect(range(3))
    params = tf.BFVParams(R, Rbig, t)
    rng = tf.DeviceRng(404)
    kp = tf.keygen(rng, params)
    nrng = np.random.default_rng(4)
    m1 = nrng.integers(0, t, size=(batch, N), dtype=np.int64)
    m2 = nrng.integers(-8, 9, size=(batch, N), dtype=np.int64)
    c1, c2 = tf.encrypt(rng, kp, m1.tolist()), tf.encrypt(rng, kp, m2)
    prod = tf.keyswitch(tf.keygen_evalmult(rng, kp.priv), c1 * c2)
    P = params.plaintext_space()
    want = (P(m1.tolist()) * P(np.mod(m2, t).tolist())).to_ints()
    arr = tf.decrypt_array(kp, prod)
    assert arr.dtype == np.uint64 and arr.shape == (batch, N)
    assert arr.tolist() == want
    assert tf.decrypt(kp, prod) == arr.tolist()
    # the batched noise budget is the per-ciphertext one, and each is the host formula over the same b
    budgets = tf.invariant_noise_budget(kp.priv, prod)
    assert isinstance(budgets, list) and len(budgets) == batch
    parts = prod.split([1] * batch)
    for i in (0, 17, batch - 1):
        single = tf.invariant_noise_budget(kp.priv, parts[i])          # a batch of one: a list of one
        assert single == [budgets[i]]
        _, b = tf.she._decryption(kp, parts[i])
        assert budgets[i] == _host_budget(b.to_ints()[0], params)
    # one ciphertext (no batch dimension) still gives one float, the same formula
    c0 = tf.encrypt(rng, kp, [5] + [0] * (N - 1))
    v = tf.invariant_noise_budget(kp.priv, c0)
    _, b0 = tf.she._decryption(kp, c0)
    assert isinstance(v, float) and v == _host_budget(b0.to_ints(), params)


def test_bgv_modulus_raised_ring():
    """the ModulusRaised shape of test_gpu_configs.py:201 (N = 2^14, 6 + 1 limbs of 50 bits, t = 257): the ciphertext ring
    drops the special prime; BGV centres by the element's own modulus, so the device codec of that ring is exact"""
    N, L, t = 1 << 14, 6, 257
    qs = H.chain(50, L + 1, N)
    R = tf.NegacyclicRing(N, qs)
    params = tf.ModulusRaised(tf.BGVParams(R, t))
    rng = tf.DeviceRng(46)
    kp = tf.keygen(rng, params)
    ms = np.random.default_rng(6).integers(0, t, size=(3, N), dtype=np.int64)
    c = tf.she.encrypt_zero(rng, kp.pub, batch=3) + params.R_cipher()(ms.tolist())
    arr = tf.decrypt_array(kp, c)
    assert arr.tolist() == ms.tolist()
    y = c * c
    dec = tf.decrypt_array(kp, y)
    priv, b = tf.she._decryption(kp, y)
    assert dec.tolist() == params.params._host_decode(b) == tf.decrypt(kp, y)


def test_modulus_raised_bfv_keeps_the_host_path():
    """ModulusRaised(BFV) centres by params.ring's modulus, not by the ciphertext ring's: decode stays on the host, unchanged"""
    N, t = 1 << 12, 65537
    ch = H.chain(50, 8, N)
    Rbig = tf.NegacyclicRing(N, ch)
    R = Rbig.crtselect(range(4))
    params = tf.ModulusRaised(tf.BFVParams(R, Rbig, t))
    rng = tf.DeviceRng(12)
    kp = tf.keygen(rng, params)
    ms = np.random.default_rng(13).integers(0, 2**40, size=(2, N), dtype=np.int64)
    c = tf.she.encrypt_zero(rng, kp.pub, batch=2) + params.R_cipher()(ms.tolist())
    priv, b = tf.she._decryption(kp, c)
    assert not params.params._device_ring(b)
    host = params.params._host_decode(b)
    assert tf.decrypt(kp, c) == host
    assert tf.decrypt_array(kp, c).tolist() == host


def test_plan_destroy_returns_allocator_bytes():
    N, t = 1 << 12, 65537
    R = tf.NegacyclicRing(N, H.chain(50, 4, N))
    R.ctx.sync()
    start = tf.native.alloc_stats()["live_bytes"]
    plan = tf.PlainPlan(R.ctx, t)
    src = tf.DeviceBuffer(5 * 4 * N)
    R.ctx.sample_uniform(4, 3, 0, 0, src.ptr, 5)
    out = tf.DeviceBuffer(5 * N)
    words = tf.DeviceBuffer(5 * plan.delta_words)
    plan.decode(tf.native.PLAIN_BGV, src.ptr, out.ptr, 5)
    plan.noise_max(src.ptr, words.ptr, 5)
    R.ctx.sync()
    plan.close()
    for b in (src, out, words):
        b.free()
    assert tf.native.alloc_stats()["live_bytes"] == start
