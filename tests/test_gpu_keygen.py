"""tfhe_evalkey_gen on the device, through the C ABI and through the host mirror: the counter convention against tfhe_sample_uniform /
tfhe_sample_gaussian word for word, given randomness against the oracle (tests/keygen_oracle.py over oracle/ref_cpu) on every size
class, code path, gadget and source of `old`, the chunk seams, 32 / 33 limbs, the mirror against the kept composition in one
process (words, generator state, views), the switch in a fresh child process, keys that work (multiply, rotate, encrypt), and the
host-side refusals."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import helpers as H
from tests import keygen_oracle as KO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_BOUND = 2**31 - 1
POISON = 0xDEADBEEFDEADBEEF


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


def secret_ntt(ref, rng):
    """the NTT image [L][N] of a small secret"""
    ints = np.rint(rng.normal(0.0, 3.2, size=(1, ref.N))).astype(np.int64)
    return ref.nntt(KO.small_residues(ints, 1, ref.qs))[0]


def poisoned(n_keys, words):
    return [dev(np.full(words, POISON, dtype=np.uint64)) for _ in range(n_keys)]


def read(bufs, nd, L, N):
    return np.stack([b.to_numpy((nd, 2, L, N)) for b in bufs])


# ---- 1. the counter convention ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [2, 5])
@pytest.mark.parametrize("mult", [1, 65537])
@pytest.mark.parametrize("logn", [12, 11])          # the fused kernel and the composed path
def test_counter_convention_is_the_two_samplers(logn, mult, stride):
    N, K, D, seed, sigma, mask_poly, noise_poly = 1 << logn, 2, 3, 0xC0FFEE, 3.2, 17, 1000
    qs, ctx, ref = context(N, (50, 50, 50))
    L = len(qs)
    rng = np.random.default_rng(5)
    s = secret_ntt(ref, rng)
    one = tf.DeviceBuffer(L * N)
    mask, noise = np.empty((K, D, L, N), dtype=np.uint64), np.empty((K, D, N), dtype=np.int64)
    for m in range(K * D):
        ctx.sample_uniform(L, seed, 4, mask_poly + m * stride, one.ptr, 1)
        mask[m // D, m % D] = one.to_numpy((L, N))
        ctx.sample_gaussian(L, sigma, 1, seed, 9, noise_poly + m * stride, one.ptr, 1)
        e = one.to_numpy((L, N))[0].astype(np.int64)
        noise[m // D, m % D] = np.where(e > qs[0] // 2, e - qs[0], e)
    assert len(np.unique(mask[0, 0, 0])) > 8 and not np.array_equal(noise[0, 0], noise[1, 2])
    bufs, ds = poisoned(K, D * 2 * L * N), dev(s)    # (named: a buffer lives as long as its object)
    ctx.evalkey_gen(L, ds.ptr, [b.ptr for b in bufs], D, gadget=KO.rns_gadget(qs), galois_elements=[0, 3], sigma_e=sigma, mult_e=mult,
                    seed=seed, stream_mask=4, stream_noise=9, mask_poly=mask_poly, noise_poly=noise_poly, poly_stride=stride)
    got = read(bufs, D, L, N)
    # row 0 is tfhe_nntt of the uniform draw
    dm = dev(mask)
    ctx.nntt(dm.ptr, dm.ptr, K * D, L)
    assert np.array_equal(got[:, :, 0], dm.to_numpy((K, D, L, N))), "row 0 is the transform of tfhe_sample_uniform's polynomial"
    # the whole key is the oracle fed with the two samplers' outputs
    want = KO.evalkey_ref(ref, s, mask, noise, mult, gadget=KO.rns_gadget(qs), galois=[0, 3])
    assert np.array_equal(got, want)
    # one polynomial of each stream against the stream definition itself
    m, ks = 4, list(range(0, N, 97))
    assert np.array_equal(mask[m // D, m % D][:, ks], KO.stream_uniform(qs, N, seed, 4, mask_poly + m * stride, ks))
    assert (noise[m // D, m % D] != KO.stream_gauss(N, seed, 9, noise_poly + m * stride, sigma)).mean() < 0.01   # (libm against the device's)


# ---- 2. given randomness against the oracle ----------------------------------------------------------------------------------------

def gadget_of(kind, qs):
    return {"rns": lambda: KO.rns_gadget(qs), "raised": lambda: KO.rns_gadget(qs, special=True), "window": lambda: KO.window_gadget(qs, 16),
            "raised_window": lambda: KO.window_gadget(qs, 16, special=True), "none": lambda: None}[kind]()


def check_evalkey(N, bits, key_limbs, gadget_kind, source, seed, mult=1, variant=0, extreme=False, n_keys=None, chunk=0):
    qs_all, ctx, ref_all = context(N, bits)
    qs = qs_all[:key_limbs]
    ref = ref_all if key_limbs == len(qs_all) else ref_cpu.RefCtx(N, qs, ref_all.psis[:key_limbs])
    rng = np.random.default_rng(seed)
    s = secret_ntt(ref, rng)
    gadget = gadget_of(gadget_kind, qs)
    D = 1 if gadget is None else len(gadget)
    g1 = tf.she.galois_element_for_steps(1, N)
    galois = {"explicit": None, "mixed": [0, 3, 2 * N - 1, g1]}[source]
    K = n_keys or (2 if galois is None else len(galois))
    galois = None if galois is None else galois[:K]
    old = H.rand_residues(rng, qs, (K,), N) if source == "explicit" else None
    mask = H.rand_residues(rng, qs, (K, D), N)
    noise = np.rint(rng.normal(0.0, 3.2, size=(K, D, N))).astype(np.int64)
    if extreme:                                       # the growth-maximising rows: all q - 1, alternating 0 / q - 1; noise at the int32 bound
        top = np.array(qs, dtype=np.uint64)[:, None] - 1
        mask[0, :] = top
        mask[-1, :] = 0
        mask[-1, :, :, 1::2] = np.broadcast_to(top, (key_limbs, N))[:, 1::2]
        noise = np.where(rng.integers(0, 2, size=(K, D, N)) == 1, I32_BOUND, -I32_BOUND - 1).astype(np.int64)
    noise[:, :, :5] = np.array([I32_BOUND, -I32_BOUND - 1, 0, 1, -1])
    bufs = poisoned(K, D * 2 * key_limbs * N)
    ds, dmask, dnoise, dold = dev(s), dev(mask), dev_i32(noise), None if old is None else dev(old)
    ctx.set_ntt_variant(variant)
    ctx.set_chunk(chunk)
    try:
        # the seed, the streams, the counters and sigma are ignored with given randomness: pass values that would be rejected otherwise
        ctx.evalkey_gen(key_limbs, ds.ptr, [b.ptr for b in bufs], D, gadget=gadget, old=None if dold is None else dold.ptr,
                        galois_elements=galois, mask_rand=dmask.ptr, noise_rand=dnoise.ptr, mult_e=mult, sigma_e=-1.0, mask_poly=2**40, noise_poly=2**40)
        got = read(bufs, D, key_limbs, N)
    finally:
        ctx.set_ntt_variant(0)
        ctx.set_chunk(0)
    want = KO.evalkey_ref(ref, s, mask, noise, mult, gadget=gadget, old=old, galois=galois)
    assert np.array_equal(got, want), (N, bits, key_limbs, gadget_kind, source, variant, chunk)
    for j in range(key_limbs):
        assert int(got[:, :, :, j].max()) < qs[j]
    return got


KEY_CASES = [
    # (logn, modulus bits, key_limbs, gadget, old source, multiplier, variant, extreme)
    (12, (50, 50, 50), 3, "rns", "mixed", 1, 0, False),           # fp64-size ring; s s, g = 3, g = 2N - 1, g of one rotation step
    (12, (50, 50, 50), 3, "raised", "explicit", 65537, 0, False), # zero special row and column; explicit old
    (12, (50, 50, 50), 3, "window", "mixed", 1, 0, True),         # every gadget residue non-zero; growth-maximising rows
    (12, (50, 50, 50), 1, "rns", "mixed", 1, 0, False),           # key_limbs < the context's limbs
    (12, (50, 50, 50), 3, "none", "explicit", 65537, 0, True),    # the public-key form: old ignored
    (12, (60, 60, 60), 3, "rns", "mixed", 1, 0, True),            # u64 policy
    (12, (60, 50, 50), 3, "raised_window", "mixed", 65537, 0, False),   # mixed: two lanes
    (12, (60, 50, 50), 1, "window", "explicit", 1, 0, False),
    (13, (60, 50, 50), 3, "rns", "mixed", 1, 0, False),
    (14, (60, 50, 50), 3, "raised", "mixed", 65537, 0, True),     # the 512-thread register map, both policies; row 0 read back
    (11, (50, 60, 50), 3, "rns", "mixed", 65537, 0, False),       # composed path below the fused sizes
    (11, (50, 60, 50), 3, "none", "mixed", 1, 0, False),
    (15, (60, 50, 50), 3, "raised", "mixed", 1, 0, False),        # ... and above
    (15, (60, 50, 50), 1, "window", "explicit", 1, 0, True),
    (12, (50, 60, 50), 3, "rns", "mixed", 1, 1, False),           # set_ntt_variant(1): composed at a fused size
    (12, (50, 60, 50), 3, "window", "explicit", 65537, 2, True),  # set_ntt_variant(2)
]


@pytest.mark.parametrize("logn,bits,key_limbs,gadget,source,mult,variant,extreme", KEY_CASES)
def test_evalkey_with_given_randomness_matches_the_oracle(logn, bits, key_limbs, gadget, source, mult, variant, extreme):
    check_evalkey(1 << logn, bits, key_limbs, gadget, source, 7000 + logn * 31 + key_limbs + variant, mult, variant, extreme)


# ---- 3. chunk seams ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("logn,bits", [(12, (60, 50, 50)), (11, (60, 50, 50))])     # the fused and the composed path, mixed ring
def test_words_do_not_depend_on_the_chunk(logn, bits):
    """2 keys x 3 digits x 3 limbs with the chunk capped at 1, 2 and 5 components: seams inside a key and across the two"""
    whole = check_evalkey(1 << logn, bits, 3, "rns", "mixed", 31, n_keys=2)
    for cap in (1, 2, 5):
        assert np.array_equal(check_evalkey(1 << logn, bits, 3, "rns", "mixed", 31, n_keys=2, chunk=cap), whole), cap
    # device randomness across the seams: the counters are those of the whole call
    qs, ctx, ref = context(1 << logn, bits)
    N, L = 1 << logn, 3
    s = dev(secret_ntt(ref, np.random.default_rng(3)))

    def run(cap):
        bufs = poisoned(2, 3 * 2 * L * N)
        ctx.set_chunk(cap)
        try:
            ctx.evalkey_gen(L, s.ptr, [b.ptr for b in bufs], 3, gadget=KO.rns_gadget(qs), galois_elements=[0, 3], sigma_e=3.2, seed=11,
                            mask_poly=5, noise_poly=6, poly_stride=2)
            return read(bufs, 3, L, N)
        finally:
            ctx.set_chunk(0)
    base = run(0)
    assert not (base == POISON).any()
    for cap in (1, 2, 5):
        assert np.array_equal(run(cap), base), cap


# ---- 4. many limbs ---------------------------------------------------------------------------------------------------------------------

def test_33_limbs_and_33_digits_on_the_composed_path():
    N, L = 1 << 5, 33
    qs = H.primes_above(1 << 50, L, N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(33)
    s, mask = secret_ntt(ref, rng), H.rand_residues(rng, qs, (2, L), N)
    noise = np.rint(rng.normal(0.0, 3.2, size=(2, L, N))).astype(np.int64)
    bufs = poisoned(2, L * 2 * L * N)
    ds, dmask, dnoise = dev(s), dev(mask), dev_i32(noise)    # (named: a buffer lives as long as its object)
    ctx.evalkey_gen(L, ds.ptr, [b.ptr for b in bufs], L, gadget=KO.rns_gadget(qs), galois_elements=[0, 2 * N - 1], mask_rand=dmask.ptr,
                    noise_rand=dnoise.ptr)
    assert np.array_equal(read(bufs, L, L, N), KO.evalkey_ref(ref, s, mask, noise, 1, gadget=KO.rns_gadget(qs), galois=[0, 2 * N - 1]))
    # the stream's limb counter at 33 limbs: device randomness, limb 32 against the definition
    ctx.evalkey_gen(L, ds.ptr, [bufs[0].ptr], 1, gadget=None, sigma_e=3.2, seed=77, mask_poly=9, noise_poly=10)
    row0 = ref.inntt(bufs[0].to_numpy((L, 2, L, N))[0, 0][None])[0]
    assert np.array_equal(row0, KO.stream_uniform(qs, N, 77, 0, 9))


def test_32_limbs_on_the_fused_path():
    N, L, D = 1 << 12, 32, 2
    qs = H.primes_above(1 << 50, L, N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(32)
    s, mask = secret_ntt(ref, rng), H.rand_residues(rng, qs, (1, D), N)
    noise = np.rint(rng.normal(0.0, 3.2, size=(1, D, N))).astype(np.int64)
    gadget = KO.rns_gadget(qs)[:D]
    bufs = poisoned(1, D * 2 * L * N)
    ds, dmask, dnoise = dev(s), dev(mask), dev_i32(noise)
    ctx.evalkey_gen(L, ds.ptr, [bufs[0].ptr], D, gadget=gadget, galois_elements=[3], mask_rand=dmask.ptr, noise_rand=dnoise.ptr)
    assert np.array_equal(read(bufs, D, L, N), KO.evalkey_ref(ref, s, mask, noise, 1, gadget=gadget, galois=[3]))


# ---- 5. the mirror against the kept composition -----------------------------------------------------------------------------------------

def _schemes(N):
    R = tf.NegacyclicRing.from_logqs(N, (50, 50, 50))
    Rmix = tf.NegacyclicRing.from_logqs(N, (60, 40, 60))
    Rbig = tf.NegacyclicRing.from_logqs(N, (50, 50, 50, 50, 50, 50, 50))
    t = 65537
    return {"bfv": tf.BFVParams(R, Rbig, t), "bgv": tf.BGVParams(R, t), "ckks": tf.CKKSParams(Rmix, 0, 3.2),
            "raised_ckks": tf.ModulusRaised(tf.CKKSParams(Rmix, 0, 3.2)), "bfv_window": tf.BFVParams(R, Rbig, t, relin_window=16)}


_SCHEMES = {}


def _words(ksk):
    return ksk.packed().to_numpy()


def _all_keys(params, kind, composed):
    """keygen, keygen_evalmult, keygen_galois and three more Galois keys from one generator; -> (packed words, generator state)"""
    N = params.R_key().N
    gs = [3, 2 * N - 1, tf.she.galois_element_for_steps(2, N)]
    rng = tf.DeviceRng(4321) if kind == "device" else np.random.default_rng(4321)
    S = tf.she
    if composed:
        kp = S._keygen_composed(rng, params)
        ek = S._keygen_evalmult_composed(rng, kp.priv)
        gk = S._keygen_galois_composed(rng, kp.priv, steps=1)
        many = [S._keygen_galois_composed(rng, kp.priv, galois_element=g) for g in gs]
    else:
        kp = tf.keygen(rng, params)
        ek = tf.keygen_evalmult(rng, kp.priv)
        gk = tf.keygen_galois(rng, kp.priv, steps=1)
        many = tf.keygen_galois_many(rng, kp.priv, galois_elements=gs)
    assert [g.galois_element for g in many] == gs
    state = rng.next_poly if kind == "device" else rng.bit_generator.state
    pub = S._packed_pubkey(kp.pub, params.R_key()).to_numpy()
    return kp, {"pub": pub, "ek": _words(ek.key), "gk": _words(gk.key), **{f"many{i}": _words(g.key) for i, g in enumerate(many)}}, state, (ek, gk, many)


@pytest.mark.parametrize("kind", ["device", "numpy"])
@pytest.mark.parametrize("scheme", ["bfv", "bgv", "ckks", "raised_ckks", "bfv_window"])
@pytest.mark.parametrize("logn", [12, 11])
def test_mirror_keys_are_the_compositions_words(logn, scheme, kind):
    assert tf.she._FUSED_KEYGEN
    N = 1 << logn
    if N not in _SCHEMES:
        _SCHEMES[N] = _schemes(N)
    params = _SCHEMES[N][scheme]
    kp, new, state_new, (ek, gk, many) = _all_keys(params, kind, composed=False)
    _, old, state_old, _ = _all_keys(params, kind, composed=True)
    for name in old:
        assert np.array_equal(new[name], old[name]), f"{name}: the call's words differ from the composition's"
    assert state_new == state_old, "the generator does not end in the same state"
    if kind == "device":
        nd = len(ek.key.key)
        assert state_new == 3 + 2 * nd * 5                                       # 3 for keygen, 2 per digit of five keys
    # the key's components are views into the buffer the call wrote: packed() copies nothing
    ring_, sz = params.R_key(), params.R_key().L * N
    assert kp.pub._packed is not None and kp.pub.key.mask.dual.parent is kp.pub._packed
    for ksk in [ek.key, gk.key] + [g.key for g in many]:
        buf = ksk._packed
        assert buf is not None and ksk.packed() is buf
        words = buf.to_numpy((len(ksk.key), 2, ring_.L, N))
        for i, kc in enumerate(ksk.key):
            assert kc.mask.dual.parent is buf and kc.mask.dual.ptr == buf.ptr + (2 * i) * sz * 8
            assert np.array_equal(kc.mask.to_numpy("dual"), words[i, 0]) and np.array_equal(kc.masked.to_numpy("dual"), words[i, 1])


CHILD = r"""
import hashlib
import numpy as np
import toyfhe_jl_amd as tf
R = tf.NegacyclicRing.from_logqs(4096, (50, 50, 50))
rng = tf.DeviceRng(99)
kp = tf.keygen(rng, tf.BGVParams(R, 65537))
gk = tf.keygen_galois_many(rng, kp.priv, steps=[1, 2])[1]
print("RESULT", tf.she._FUSED_KEYGEN, isinstance(gk.key.key[0].mask.dual, tf.she._KeyView), rng.next_poly,
      hashlib.sha256(gk.key.packed().to_numpy().tobytes()).hexdigest())
"""


def test_switch_selects_the_composition():
    """TFHE_FUSED_KEYGEN=0 in a fresh child process: the composition runs (no views into a packed buffer), the same words come out"""
    env = dict(os.environ)
    env["TFHE_FUSED_KEYGEN"] = "0"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    fused, views, state, digest = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1].split()[1:]
    assert fused == "False" and views == "False"
    R = tf.NegacyclicRing.from_logqs(4096, (50, 50, 50))
    rng = tf.DeviceRng(99)
    kp = tf.keygen(rng, tf.BGVParams(R, 65537))
    gk = tf.keygen_galois_many(rng, kp.priv, steps=[1, 2])[1]
    assert isinstance(gk.key.key[0].mask.dual, tf.she._KeyView)
    assert int(state) == rng.next_poly
    assert digest == hashlib.sha256(gk.key.packed().to_numpy().tobytes()).hexdigest()


# ---- 6. keys that work (no oracle) ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["device", "numpy"])
def test_keys_from_the_call_multiply_rotate_and_encrypt(kind):
    N = 1 << 12
    rng = tf.DeviceRng(21) if kind == "device" else np.random.default_rng(21)
    R = tf.NegacyclicRing(N, H.chain(40, 3, N))                    # rescaling by a 40-bit prime keeps the scale at 2^40
    params = tf.ModulusRaised(tf.CKKSParams(R, 0, 3.2))
    kp = tf.keygen(rng, params)
    ek = tf.keygen_evalmult(rng, kp.priv)
    gk, gk2 = tf.keygen_galois_many(rng, kp.priv, steps=[1, 2])
    assert isinstance(ek.key._packed, tf.DeviceBuffer) and isinstance(kp.pub._packed, tf.DeviceBuffer)     # the call made them
    vals = (np.arange(1, N // 2 + 1) / N).astype(complex)
    scale = 2**40
    c = tf.encrypt(rng, kp, tf.ckks_encode(vals, params.R_cipher(), scale), scale=scale)
    assert np.abs(tf.ckks_decode(tf.decrypt(kp, c), c.scale) - vals).max() < 1e-6
    sq = tf.mul_relin(ek, c, c, rescale=True)
    assert np.abs(tf.ckks_decode(tf.decrypt(kp, sq), sq.scale) - vals * vals).max() < 1e-5
    r1, r2 = tf.rotate(gk, c), tf.rotate(gk2, c)
    assert np.abs(tf.ckks_decode(tf.decrypt(kp, r1), r1.scale) - np.roll(vals, 1)).max() < 1e-6
    assert np.abs(tf.ckks_decode(tf.decrypt(kp, r2), r2.scale) - np.roll(vals, 2)).max() < 1e-6
    # BFV: encrypt under the call's public key, decrypt, and a positive noise budget; relinearise with a windowed key of the call
    Rq = tf.NegacyclicRing.from_logqs(N, (50, 50, 50))
    Rbig = tf.NegacyclicRing.from_logqs(N, (50, 50, 50, 50, 50, 50, 50))
    t = 65537
    bfv = tf.BFVParams(Rq, Rbig, t, relin_window=16)
    kb = tf.keygen(rng, bfv)
    ekb = tf.keygen_evalmult(rng, kb.priv)
    m = np.zeros(N, dtype=np.int64)
    m[:3] = [7, 3, t - 1]
    cb = tf.encrypt(rng, kb.pub, m)
    assert np.array_equal(tf.decrypt_array(kb, cb), m.astype(np.uint64))
    assert tf.invariant_noise_budget(kb, cb) > 0
    prod = tf.keyswitch(ekb, cb * cb)
    want = np.zeros(N, dtype=np.int64)                               # (7 + 3x - x^2)^2 = 49 + 42x - 5x^2 - 6x^3 + x^4
    want[:5] = [49, 42, t - 5, t - 6, 1]
    assert np.array_equal(tf.decrypt_array(kb, prod), want.astype(np.uint64))
    assert tf.invariant_noise_budget(kb, prod) > 0


# ---- 7. refusals (host side; the outputs stay untouched) -----------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched():
    N, L, D = 1 << 12, 3, 3
    qs, ctx, ref = context(N, (50, 50, 50))
    s = dev(secret_ntt(ref, np.random.default_rng(1)))
    words = D * 2 * L * N
    big = dev(np.full(2 * words, POISON, dtype=np.uint64))
    o0, o1 = big.ptr, big.ptr + words * 8
    rnd = tf.DeviceBuffer(2 * D * L * N)
    kw = dict(gadget=KO.rns_gadget(qs), sigma_e=3.2, seed=1)

    def refused(exc, outs, **more):
        with pytest.raises(exc):
            ctx.evalkey_gen(L, s.ptr, outs, D, **{**kw, "galois_elements": [0, 3][:len(outs)], **more})
    refused(AssertionError, [o0, o1 - 8])                                        # the second output starts inside the first
    refused(AssertionError, [o0, o0 + 8 * N])
    refused(AssertionError, [o0, o1], galois_elements=[0, 4])                    # an even g
    refused(AssertionError, [o0, o1], galois_elements=[2 * N + 1, 3])            # g >= 2N
    refused(AssertionError, [o0, o1], galois_elements=[2 * N, 3])
    refused(AssertionError, [o0, o1], mask_rand=rnd.ptr)                         # exactly one of the two
    refused(AssertionError, [o0, o1], noise_rand=rnd.ptr)
    refused(AssertionError, [o0, o1], mask_rand=o1 + 8 * N, noise_rand=rnd.ptr)  # an output reaching into an operand
    refused(AssertionError, [o0], old=o0 + 8)
    bad = KO.rns_gadget(qs)
    bad[1][1] = qs[1]
    refused(AssertionError, [o0, o1], gadget=bad)                                # a gadget residue that is not a residue
    with pytest.raises(tf.UsageError):
        ctx.evalkey_gen(L + 1, s.ptr, [o0], 1, sigma_e=3.2)                      # key_limbs above the context's limbs
    with pytest.raises(AssertionError):
        ctx.evalkey_gen(L, s.ptr, [o0, o1], D, **kw, galois_elements=[0, 3], mask_poly=2**32 - 10)   # the last counter reaches 2^32
    ctx.sync()
    assert (big.to_numpy() == POISON).all(), "a refused call wrote to its outputs"
    ctx.evalkey_gen(L, s.ptr, [], D, **kw, galois_elements=[])                   # n_keys == 0 does nothing
    ctx.sync()
    assert (big.to_numpy() == POISON).all()
    ctx.evalkey_gen(L, s.ptr, [o0, o1], D, **kw, galois_elements=[0, 3])         # and the accepted call writes every word
    ctx.sync()
    got = big.to_numpy((2, D, 2, L, N))
    assert not (got == POISON).any() and all(int(got[:, :, :, j].max()) < qs[j] for j in range(L))
