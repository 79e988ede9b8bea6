"""tfhe_encrypt / tfhe_decrypt_phase on the device, through the C ABI: the counter convention against tfhe_sample_gaussian word
for word, given randomness against the oracle (tests/enc_oracle.py over oracle/ref_cpu) on every size class and code path, the
decryption phase against the oracle, and the host mirror: the same residues and the same generator state with the calls on
(default) and off (TFHE_FUSED_ENCRYPT=0, the composition on ring elements), compared across two fresh child processes."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import enc_oracle as EO
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_BOUND = 2**31 - 1


def dev(a):
    return tf.DeviceBuffer.from_numpy(a)


def dev_i32(a):
    """int32 [..] -> device (the buffer type moves 64-bit words: an even number of int32)"""
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    assert a.size % 2 == 0
    return tf.DeviceBuffer.from_numpy(a.view(np.uint64))


def ring(N, bits):
    """one NTT-friendly prime per entry of `bits`, distinct, just above 2^bits"""
    qs = []
    for b in bits:
        qs.append(next(q for q in H.primes_above(1 << b, len(bits) + 1, N) if q not in qs))
    return qs


_CTX = {}


def context(N, bits):
    key = (N, tuple(bits))
    if key not in _CTX:
        qs = ring(N, bits)
        ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
        assert ctx.psis == ref.psis
        _CTX[key] = (qs, ctx, ref)
    return _CTX[key]


# ---- 1. the counter convention ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("logn", [12, 11])          # the fused kernel and the composed path: one sample_gauss_int
@pytest.mark.parametrize("mult", [1, 65537])
def test_counter_convention_is_three_sample_gaussian_calls(logn, mult):
    N, batch, first, seed, su, se = 1 << logn, 3, 17, 0xC0FFEE, 3.2, 19.5
    qs, ctx, ref = context(N, (50, 50))
    L = len(qs)

    def gauss(first_poly, sigma, m):
        o = tf.DeviceBuffer(batch * L * N)
        ctx.sample_gaussian(L, sigma, m, seed, 1, first_poly, o.ptr, batch)
        return o.to_numpy((batch, L, N))
    u, e1, e2 = gauss(first, su, 1), gauss(first + batch, se, mult), gauss(first + 2 * batch, se, mult)
    assert len(np.unique(u[0, 0])) > 8 and not np.array_equal(e1, e2)
    out = tf.DeviceBuffer(batch * 2 * L * N)
    zero = dev(np.zeros((2, L, N), dtype=np.uint64))
    ctx.encrypt(L, L, zero.ptr, out.ptr, batch, sigma_u=su, sigma_e=se, mult_e=mult, seed=seed, stream=1, first_poly=first)
    got = out.to_numpy((batch, 2, L, N))
    assert np.array_equal(got[:, 0], e1), "component 0 with a zero key is the Gaussian draw at first_poly + batch"
    assert np.array_equal(got[:, 1], e2), "component 1 with a zero key is the Gaussian draw at first_poly + 2 batch"
    one = np.zeros((2, L, N), dtype=np.uint64)
    one[1] = 1                                       # masked = the NTT image of the constant 1
    ctx.encrypt(L, L, dev(one).ptr, out.ptr, batch, sigma_u=su, sigma_e=se, mult_e=mult, seed=seed, stream=1, first_poly=first)
    got = out.to_numpy((batch, 2, L, N))
    assert np.array_equal(ref.pointwise("sub", got[:, 0], e1), u), "component 0 - e1 with masked = 1 is the draw at first_poly"
    assert np.array_equal(got[:, 1], e2)


# ---- 2. given randomness against the oracle ----------------------------------------------------------------------------------------

def rand_ints(rng, batch, N, extreme=False):
    if extreme:
        r = np.where(rng.integers(0, 2, size=(batch, 3, N)) == 1, I32_BOUND, -I32_BOUND - 1).astype(np.int64)
    else:
        r = np.rint(rng.normal(0.0, 3.2, size=(batch, 3, N))).astype(np.int64)
    r[:, :, :5] = np.array([I32_BOUND, -I32_BOUND - 1, 0, 1, -1])
    return r


def check_encrypt(N, bits, level, batch, seed, with_msg=True, mult=1, variant=0, extreme=False):
    qs, ctx, ref_all = context(N, bits)
    Lk = len(qs)
    ref = ref_all if level == Lk else ref_cpu.RefCtx(N, qs[:level], ref_all.psis[:level])
    rng = np.random.default_rng(seed)
    pk = H.rand_residues(rng, qs, (2,), N)
    if extreme:
        pk[:] = np.array(qs, dtype=np.uint64)[None, :, None] - 1
    rand = rand_ints(rng, batch, N, extreme)
    msg = H.rand_residues(rng, qs[:level], (batch,), N) if with_msg else None
    if extreme and with_msg:
        msg[:] = np.array(qs[:level], dtype=np.uint64)[None, :, None] - 1
    out = tf.DeviceBuffer(batch * 2 * level * N)
    dm = None if msg is None else dev(msg)
    ctx.set_ntt_variant(variant)
    try:
        # seed, stream, first_poly and the sigmas are ignored with given randomness: pass values that would be rejected otherwise
        ctx.encrypt(Lk, level, dev(pk).ptr, out.ptr, batch, msg=None if dm is None else dm.ptr, rand=dev_i32(rand).ptr, mult_e=mult,
                    sigma_u=-1.0, first_poly=2**40)
        got = out.to_numpy((batch, 2, level, N))
    finally:
        ctx.set_ntt_variant(0)
    want = EO.encrypt_ref(ref, pk[:, :level], rand, mult, msg)
    assert np.array_equal(got, want), (N, bits, level, batch, with_msg, mult, variant)
    for j in range(level):
        assert int(got[:, :, j].max()) < qs[j]


ENC_CASES = [
    # (logn, modulus bits, level, batch, message, multiplier, variant, extreme)
    (12, (50, 50, 50), 3, 2, True, 1, 0, False),        # fp64-size ring
    (12, (50, 50, 50), 2, 2, True, 65537, 0, False),    # level < key_limbs (ModulusRaised)
    (12, (50, 50, 50), 3, 1, False, 1, 0, True),        # msg = NULL, batch = 1, growth-maximising words
    (12, (60, 60), 2, 2, True, 1, 0, True),             # u64 policy
    (12, (60, 40, 60), 3, 3, True, 65537, 0, False),    # mixed: two lanes
    (12, (60, 40, 60), 2, 2, False, 1, 0, False),
    (13, (60, 40), 2, 2, True, 1, 0, False),
    (14, (60, 50), 2, 2, True, 65537, 0, True),         # the 512-thread register map, both policies; NTT(u) parked
    (11, (50, 60), 2, 2, True, 65537, 0, False),        # composed path below the fused sizes
    (15, (50, 60), 2, 2, True, 1, 0, False),            # ... and above
    (16, (60, 40), 2, 1, True, 1, 0, False),            # mixed ring at 2^16
    (12, (50, 60), 2, 2, True, 1, 1, False),            # set_ntt_variant(1): composed at a fused size
]


@pytest.mark.parametrize("logn,bits,level,batch,with_msg,mult,variant,extreme", ENC_CASES)
def test_encrypt_with_given_randomness_matches_the_oracle(logn, bits, level, batch, with_msg, mult, variant, extreme):
    check_encrypt(1 << logn, bits, level, batch, 7000 + logn * 31 + level + batch, with_msg, mult, variant, extreme)


def test_encrypt_item_walk_wraps():
    """more (ciphertext, limb) items than the persistent grid has workgroups (at most 8 per CU): every workgroup takes several"""
    check_encrypt(1 << 12, (50, 60), 2, 1400, 99, with_msg=True, mult=1)


# ---- 4. the decryption phase -------------------------------------------------------------------------------------------------------

def check_decrypt(N, bits, level, polys, ntt_in, batch, seed, variant=0, extreme=False):
    qs, ctx, ref_all = context(N, bits)
    Lk = len(qs)
    ref = ref_all if level == Lk else ref_cpu.RefCtx(N, qs[:level], ref_all.psis[:level])
    rng = np.random.default_rng(seed)
    s = H.rand_residues(rng, qs, (), N)                                  # [Lk][N], NTT domain
    ct = H.rand_residues(rng, qs[:level], (batch, polys), N)
    if extreme:
        s[:] = np.array(qs, dtype=np.uint64)[:, None] - 1
        ct[:] = np.array(qs[:level], dtype=np.uint64)[None, None, :, None] - 1
        ct[:, :, :, :3] = np.array([0, 1, 2], dtype=np.uint64)
    out = tf.DeviceBuffer(batch * level * N)
    ctx.set_ntt_variant(variant)
    try:
        ctx.decrypt_phase(Lk, level, dev(s).ptr, dev(ct).ptr, polys, out.ptr, batch, ntt_in=ntt_in)
        got = out.to_numpy((batch, level, N))
    finally:
        ctx.set_ntt_variant(0)
    want = EO.decrypt_ref(ref, s[:level], ct, ntt_in)
    assert np.array_equal(got, want), (N, bits, level, polys, ntt_in, batch, variant)
    for j in range(level):
        assert int(got[:, j].max()) < qs[j]


DEC_SIZES = [
    # (logn, modulus bits, level, batch, variant, extreme)
    (12, (50, 50, 50), 3, 2, 0, False),
    (12, (50, 50, 50), 2, 1, 0, True),                  # level < key_limbs
    (12, (60, 60), 2, 2, 0, True),
    (12, (60, 40, 60), 3, 3, 0, False),
    (13, (60, 40), 2, 2, 0, False),
    (14, (60, 50), 2, 2, 0, False),
    (11, (50, 60), 2, 2, 0, False),
    (15, (50, 60), 2, 2, 0, False),
    (16, (60, 40), 2, 1, 0, False),
    (12, (50, 60), 2, 2, 1, False),
]


@pytest.mark.parametrize("ntt_in", [False, True])
@pytest.mark.parametrize("polys", [2, 3])
@pytest.mark.parametrize("logn,bits,level,batch,variant,extreme", DEC_SIZES)
def test_decrypt_phase_matches_the_oracle(logn, bits, level, batch, variant, extreme, polys, ntt_in):
    check_decrypt(1 << logn, bits, level, polys, ntt_in, batch, 9000 + logn * 17 + polys * 4 + ntt_in, variant, extreme)


def test_decrypt_item_walk_wraps():
    check_decrypt(1 << 12, (50, 60), 2, 2, False, 1400, 98)


def test_four_components_are_unsupported_by_the_call():
    qs, ctx, _ = context(1 << 12, (50, 50, 50))
    N = 1 << 12
    s, ct, out = tf.DeviceBuffer(3 * N), tf.DeviceBuffer(4 * 3 * N), tf.DeviceBuffer(3 * N)
    with pytest.raises(NotImplementedError):
        ctx.decrypt_phase(3, 3, s.ptr, ct.ptr, 4, out.ptr, 1)
    with pytest.raises(AssertionError):                                  # the full range test, now that the ring's N is known
        ctx.decrypt_phase(3, 3, s.ptr, ct.ptr, 2, ct.ptr + 8 * N, 1)
    with pytest.raises(AssertionError):
        ctx.encrypt(3, 3, ct.ptr, ct.ptr + 8 * N, 1, sigma_u=3.2, sigma_e=3.2)
    ctx.encrypt(3, 3, ct.ptr, out.ptr, 0, sigma_u=3.2, sigma_e=3.2)      # batch == 0 does nothing
    ctx.decrypt_phase(3, 3, s.ptr, ct.ptr, 2, out.ptr, 0)


# ---- 3. + 5. the mirror, with the calls on and off ----------------------------------------------------------------------------------

CHILD = r"""
import hashlib, json, sys
import numpy as np
import toyfhe_jl_amd as tf

def digest(el):
    return hashlib.sha256(np.ascontiguousarray(el.to_numpy("primal")).tobytes()).hexdigest()

def residues(c):
    return [digest(x) for x in c.cs]

N, B = 4096, 3
out = {"fused": tf.she._FUSED_ENCRYPT}
R = tf.NegacyclicRing.from_logqs(N, (50, 50, 50))
Rmix = tf.NegacyclicRing.from_logqs(N, (60, 40, 60))
Rbig = tf.NegacyclicRing.from_logqs(N, (50, 50, 50, 50, 50, 50, 50))
t = 65537
plain = np.zeros((B, N), dtype=np.int64); plain[0, :] = 0; plain[1, :] = 1; plain[2, :] = t - 1; plain[:, 5] = np.array([7, t - 1, 0])
slots = np.cos(np.arange(N // 2) / 50.0).astype(complex)[None].repeat(B, axis=0)
schemes = {
    "bfv": (tf.BFVParams(R, Rbig, t), lambda p: plain),
    "bgv": (tf.BGVParams(R, t), lambda p: plain),
    "ckks": (tf.CKKSParams(Rmix, 0, 3.2), lambda p: tf.ckks_encode(slots, p.R_cipher(), 2**30)),
    "raised_ckks": (tf.ModulusRaised(tf.CKKSParams(Rmix, 0, 3.2)), lambda p: tf.ckks_encode(slots, p.R_cipher(), 2**30)),
}
for name, (params, make) in schemes.items():
    for kind in ("device", "numpy"):
        rng = tf.DeviceRng(1234) if kind == "device" else np.random.default_rng(1234)
        kp = tf.keygen(rng, params)
        c = tf.encrypt(rng, kp, make(params), scale=2**30 if "ckks" in name else None)
        z = tf.she.encrypt_zero(rng, kp.pub, B)
        rec = {"c": residues(c), "z": residues(z), "len": len(c),
               "state": rng.next_poly if kind == "device" else int(rng.integers(0, 2**62))}
        _, b = tf.she._decryption(kp, c)
        rec["b"] = digest(b)
        c3 = c * c                                           # three components, NTT images only
        rec["b3_ntt"] = digest(tf.she._decryption(kp, c3)[1])
        for x in c3.cs:
            x.coeffs_primal()                                # ... and with coefficient forms present
        rec["b3"] = digest(tf.she._decryption(kp, c3)[1])
        if name == "bfv" and kind == "device":
            c4 = tf.CipherText(params, list(c.cs) + list(z.cs))          # four components: the mirror's loop
            rec["b4"] = digest(tf.she._decryption(kp, c4)[1])
        if name in ("bfv", "bgv"):
            rec["roundtrip"] = bool(np.array_equal(tf.decrypt_array(kp, c), np.mod(plain, t).astype(np.uint64)))
            rec["single"] = bool(tf.decrypt(kp, tf.encrypt(rng, kp, plain[2].tolist())) == np.mod(plain[2], t).tolist())
        if name == "bfv":
            rec["budget"] = tf.invariant_noise_budget(kp, c)
        out[name + "/" + kind] = rec
print("RESULT " + json.dumps(out))
"""


def _child(fused):
    env = dict(os.environ)
    env.pop("TFHE_FUSED_ENCRYPT", None)
    if not fused:
        env["TFHE_FUSED_ENCRYPT"] = "0"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def mirror_runs():
    return _child(True), _child(False)


def test_switch_selects_the_path(mirror_runs):
    on, off = mirror_runs
    assert on["fused"] is True and off["fused"] is False


@pytest.mark.parametrize("scheme", ["bfv", "bgv", "ckks", "raised_ckks"])
@pytest.mark.parametrize("kind", ["device", "numpy"])
def test_mirror_residues_and_generator_state_do_not_depend_on_the_switch(mirror_runs, scheme, kind):
    on, off = (r[scheme + "/" + kind] for r in mirror_runs)
    assert on["len"] == off["len"] == 2
    assert on["c"] == off["c"], "tf.encrypt: the ciphertext residues differ"
    assert on["z"] == off["z"], "tf.encrypt_zero: the ciphertext residues differ"
    assert on["state"] == off["state"], "the generator does not end in the same state"
    assert on["b"] == off["b"], "decryption phase of a fresh ciphertext"
    assert on["b3"] == off["b3"] and on["b3_ntt"] == off["b3_ntt"], "decryption phase of a 3-component product"
    assert on["b3"] == on["b3_ntt"]


def test_round_trips_and_noise_budget(mirror_runs):
    on, off = mirror_runs
    for r in (on, off):
        for key in ("bfv/device", "bfv/numpy", "bgv/device", "bgv/numpy"):
            assert r[key]["roundtrip"] is True and r[key]["single"] is True, key
    for kind in ("device", "numpy"):
        assert on["bfv/" + kind]["budget"] == off["bfv/" + kind]["budget"]          # the same b: the same floats
        assert all(b > 0 for b in on["bfv/" + kind]["budget"])
    assert on["bfv/device"]["b4"] == off["bfv/device"]["b4"], "a 4-component ciphertext decrypts through the mirror's loop"
