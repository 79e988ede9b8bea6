"""tfhe_keyswitch_grouped / tfhe_rotate_grouped on the device against tests/ks_grouped_oracle.py, word for word, every word read back
below its modulus: the two degenerate cases against tfhe_keyswitch / tfhe_rotate themselves; the shape matrix (group sizes 1 .. 4 in
registers and the run-time loop, ragged groups, levels below the key's, 34 working limbs, the row kernels, a mixed ring on both
lanes, N = 2^15); special primes below and above every ciphertext limb; batches and chunks; the five planted group integers and
every word q - 1; every host check with a context; a dirty workspace; the mirror end to end; and the key-switch step itself against
its derived noise bound."""
import math

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import helpers as H
from tests import keygen_oracle as KG
from tests import ks_grouped_oracle as KO
from tests.dirty_ws import on_dirty_workspace
from tests.test_gpu_chunk_seams import cap

pytestmark = pytest.mark.gpu


def dev(a):
    return tf.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.uint64))


def dev_i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    assert a.size % 2 == 0
    return tf.DeviceBuffer.from_numpy(a.view(np.uint64))


def poisoned(words):
    return dev(np.full(words, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))


_CTX = {}


def pair(N, qs):
    key = (N, tuple(qs))
    if key not in _CTX:
        ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
        assert ctx.psis == ref.psis
        _CTX[key] = (ctx, ref)
    return _CTX[key]


def qcol(qs):
    return np.array([int(q) for q in qs], dtype=np.uint64).reshape(-1, 1)


def operands(N, qs, k, alpha, level, polys, batch, seed=0, spare=1, edge=False):
    """a uniform key of ceil(level / alpha) + spare components and a uniform ciphertext (edge: every word q - 1)"""
    rng = np.random.default_rng(N % 991 + 13 * len(qs) + 5 * k + alpha + level + seed)
    nd = -(-level // alpha) + spare
    if edge:
        evk = np.broadcast_to(qcol(qs) - np.uint64(1), (nd, 2, len(qs), N)).copy()
        ct = np.broadcast_to(qcol(qs[:level]) - np.uint64(1), (batch, polys, level, N)).copy()
    else:
        evk, ct = H.uniform_evk(rng, qs, nd, N), H.rand_residues(rng, qs[:level], (batch, polys), N)
    return evk, ct


def plant(ct, qs, level, alpha):
    """the integers 0, 1, Q_g - 1, Q_g // 2, Q_g // 2 + 1 in coefficients 0 .. 4 of c[end], for every group of every ciphertext"""
    for G in KO.groups(level, alpha):
        Qg = math.prod(int(qs[i]) for i in G)
        for pos, v in enumerate((0, 1, Qg - 1, Qg // 2, Qg // 2 + 1)):
            for i in G:
                ct[:, -1, i, pos] = v % int(qs[i])
    return ct


def check(N, qs, k, alpha, level, polys, batch, evk, ct, rotate=None):
    ctx, ref = pair(N, qs)
    Lk = len(qs)
    devk, dct, out = dev(evk), dev(ct), poisoned(batch * 2 * level * N)
    if rotate is None:
        want = KO.keyswitch_grouped_ref(ref, level, k, alpha, evk, ct)
        ctx.keyswitch_grouped(Lk, level, k, alpha, devk.ptr, evk.shape[0], dct.ptr, polys, out.ptr, batch)
    else:
        want = KO.rotate_grouped_ref(ref, level, k, alpha, evk, rotate, ct)
        ctx.rotate_grouped(Lk, level, k, alpha, devk.ptr, evk.shape[0], rotate, dct.ptr, out.ptr, batch)
    got = out.to_numpy((batch, 2, level, N))
    assert (got < qcol(qs[:level])).all()
    assert np.array_equal(got, want), (N, k, alpha, level, polys, batch, rotate, int((got != want).sum()))
    return got


# ---- degenerate parity: the words of tfhe_keyswitch / tfhe_rotate -------------------------------------------------------------

@pytest.mark.parametrize("special", [1, 0])
@pytest.mark.parametrize("N,bits,Lk", [(64, 30, 4), (1 << 12, 50, 4), (1 << 15, 40, 4)])
def test_one_limb_per_digit_is_tfhe_keyswitch_and_tfhe_rotate(N, bits, Lk, special):
    qs = H.chain(bits, Lk, N)
    ctx, _ = pair(N, qs)
    level, batch = Lk - special, 2
    g = pow(3, N // 2 + 3, 2 * N)
    for polys in (2, 3):
        evk, ct = operands(N, qs, special, 1, level, polys, batch, spare=special)   # (tfhe_keyswitch reads `level` components)
        devk, dct = dev(evk), dev(ct)
        a, b = poisoned(batch * 2 * level * N), poisoned(batch * 2 * level * N)
        ctx.keyswitch(Lk, level, special, devk.ptr, evk.shape[0], dct.ptr, polys, a.ptr, batch)
        ctx.keyswitch_grouped(Lk, level, special, 1, devk.ptr, evk.shape[0], dct.ptr, polys, b.ptr, batch)
        assert np.array_equal(a.to_numpy(), b.to_numpy()), (N, special, polys)
        if polys == 2:
            ctx.rotate(Lk, level, special, devk.ptr, evk.shape[0], g, dct.ptr, a.ptr, batch)
            ctx.rotate_grouped(Lk, level, special, 1, devk.ptr, evk.shape[0], g, dct.ptr, b.ptr, batch)
            assert np.array_equal(a.to_numpy(), b.to_numpy()), (N, special, "rotate")


# ---- the shape matrix ---------------------------------------------------------------------------------------------------------

def _mixed13(N):
    return H.chain(61, 1, N) + H.chain(40, 3, N) + H.chain(41, 2, N)


SHAPES = [  # (N, moduli of the key ring, k, alpha, level, batch)
    pytest.param(64, lambda N: H.chain(30, 8, N), 2, 2, 6, 3, id="64-6x30-k2-a2-level6"),
    pytest.param(64, lambda N: H.chain(30, 8, N), 2, 2, 3, 3, id="64-6x30-k2-a2-level3"),
    pytest.param(64, lambda N: H.chain(30, 10, N), 3, 3, 7, 3, id="64-7-k3-a3-level7-ragged"),
    pytest.param(64, lambda N: H.chain(30, 10, N), 3, 3, 4, 3, id="64-7-k3-a3-level4-ragged"),
    pytest.param(64, lambda N: H.chain(30, 34, N), 4, 5, 30, 2, id="64-30x30-k4-a5-34-working-limbs"),
    pytest.param(1 << 12, lambda N: H.chain(50, 7, N), 2, 2, 5, 3, id="4096-5x50-k2-a2-row-kernels"),
    pytest.param(1 << 13, _mixed13, 2, 2, 4, 3, id="8192-61+3x40-2x41-mixed-ring"),
    pytest.param(1 << 15, lambda N: H.chain(40, 6, N), 2, 2, 4, 2, id="32768-4x40-k2-a2-level4"),
    pytest.param(1 << 15, lambda N: H.chain(40, 6, N), 2, 2, 3, 2, id="32768-4x40-k2-a2-level3"),
    pytest.param(64, lambda N: H.chain(30, 5, N), 1, 6, 4, 3, id="64-4-k1-a6-one-digit"),
    pytest.param(64, lambda N: H.chain(30, 7, N), 1, 6, 6, 3, id="64-6-k1-a6-one-digit-of-six-limbs"),
    pytest.param(64, lambda N: H.chain(30, 6, N), 0, 4, 6, 3, id="64-6-k0-a4-no-special-prime"),
    pytest.param(1 << 12, lambda N: H.chain(50, 6, N), 4, 4, 2, 2, id="4096-k4-a4-level2"),
]


@pytest.mark.parametrize("N,ring,k,alpha,level,batch", SHAPES)
def test_shape_matrix_matches_the_oracle(N, ring, k, alpha, level, batch):
    qs = ring(N)
    for polys in (2, 3):
        evk, ct = operands(N, qs, k, alpha, level, polys, batch, seed=polys)
        check(N, qs, k, alpha, level, polys, batch, evk, plant(ct, qs, level, alpha))
    if N <= 1 << 13:   # the rotation: apply_galois_element into the workspace, then the same key switch
        evk, ct = operands(N, qs, k, alpha, level, 2, batch, seed=9)
        check(N, qs, k, alpha, level, 2, batch, evk, ct, rotate=pow(3, N // 2 + 3, 2 * N))


def test_rotation_at_2_to_15_matches_the_oracle():
    N = 1 << 15
    qs = H.chain(40, 6, N)
    evk, ct = operands(N, qs, 2, 2, 4, 2, 2, seed=4)
    check(N, qs, 2, 2, 4, 2, 2, evk, ct, rotate=2 * N - 1)


# ---- special prime sizes: the unsigned reduction of "last" in both directions -------------------------------------------------

@pytest.mark.parametrize("ct_bits,sp_bits", [(40, 30), (30, 50), (50, 61), (61, 30)])
def test_special_primes_below_and_above_every_ciphertext_limb(ct_bits, sp_bits):
    N = 256
    qs = H.chain(ct_bits, 4, N) + H.chain(sp_bits, 3, N)
    for edge in (False, True):
        evk, ct = operands(N, qs, 3, 2, 4, 3, 2, edge=edge)
        check(N, qs, 3, 2, 4, 3, 2, evk, ct)


# ---- edge inputs ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (1 << 12, lambda N: H.chain(40, 7, N), 3, 3, 4),
                                                  (1 << 13, _mixed13, 2, 2, 4), (256, lambda N: H.chain(61, 6, N), 2, 4, 4)])
def test_every_word_q_minus_1_and_the_planted_group_integers(N, ring, k, alpha, level):
    qs = ring(N)
    evk, ct = operands(N, qs, k, alpha, level, 3, 2, edge=True)
    check(N, qs, k, alpha, level, 3, 2, evk, ct)
    check(N, qs, k, alpha, level, 3, 2, evk, plant(ct.copy(), qs, level, alpha))
    evk, _ = operands(N, qs, k, alpha, level, 3, 2, seed=1)
    check(N, qs, k, alpha, level, 3, 2, evk, plant(ct, qs, level, alpha))


# ---- batches and chunks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (1 << 12, lambda N: H.chain(50, 6, N), 2, 3, 4)])
def test_batch_one_and_batch_five_under_every_chunk_cap(N, ring, k, alpha, level):
    qs = ring(N)
    ctx, _ = pair(N, qs)
    evk, ct = operands(N, qs, k, alpha, level, 3, 1)
    check(N, qs, k, alpha, level, 3, 1, evk, ct)
    evk, ct = operands(N, qs, k, alpha, level, 2, 5, seed=2)
    g = pow(3, N // 2 + 3, 2 * N)
    words = {}
    for c in (1, 2, 0):
        with cap(ctx, c):
            words[c] = (check(N, qs, k, alpha, level, 2, 5, evk, ct), check(N, qs, k, alpha, level, 2, 5, evk, ct, rotate=g))
    for c in (1, 2):
        assert np.array_equal(words[c][0], words[0][0]) and np.array_equal(words[c][1], words[0][1])
    # an empty batch does nothing
    out = poisoned(8)
    ctx.keyswitch_grouped(len(qs), level, k, alpha, out.ptr, 9, out.ptr, 2, out.ptr, 0)
    ctx.rotate_grouped(len(qs), level, k, alpha, out.ptr, 9, 3, out.ptr, out.ptr, 0)
    assert (out.to_numpy() == np.uint64(0xA5A5A5A5A5A5A5A5)).all()


# ---- the host checks, with a context ----------------------------------------------------------------------------------------

def test_host_checks_in_the_headers_order_leave_the_output_untouched():
    N = 64
    qs = H.chain(30, 6, N)
    ctx, _ = pair(N, qs)
    buf = poisoned(2 * 4 * N)
    p = buf.ptr

    def ks(Lk=6, level=4, k=2, group=2, evk=p, nd=2, ct=p, polys=2, out=p, batch=1):
        ctx.keyswitch_grouped(Lk, level, k, group, evk, nd, ct, polys, out, batch)

    def rot(g, batch=1, nd=2):
        ctx.rotate_grouped(6, 4, 2, 2, p, nd, g, p, p, batch)
    for kw in (dict(evk=None, polys=4), dict(ct=None, Lk=0), dict(out=None, k=9)):
        with pytest.raises(AssertionError, match="null argument"):
            ks(**kw)
    with pytest.raises(AssertionError, match="2- or 3-element"):
        ks(polys=4, Lk=7)
    for lk in (0, 7):
        with pytest.raises(AssertionError, match="key_limbs"):
            ks(Lk=lk, k=5)
    for k in (-1, 5):
        with pytest.raises(AssertionError, match="n_special"):
            ks(k=k, group=0)
    with pytest.raises(AssertionError, match="group"):
        ks(group=0, level=0)
    for lv in (0, 5):
        with pytest.raises(tf.UsageError, match="level"):
            ks(level=lv, nd=0)
    with pytest.raises(tf.UsageError, match="components"):
        ks(nd=1, batch=-1)
    with pytest.raises(AssertionError, match="negative batch"):
        ks(batch=-1)
    with pytest.raises(AssertionError, match="negative batch"):
        rot(4, batch=-1)
    for g in (0, 4, 2 * N, 2 * N + 1):
        with pytest.raises(AssertionError, match="odd and below 2N"):
            rot(g)
    with pytest.raises(tf.UsageError, match="components"):
        rot(4, nd=1)
    ctx.sync()
    assert (buf.to_numpy() == np.uint64(0xA5A5A5A5A5A5A5A5)).all()


# ---- on a dirty workspace -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["keyswitch", "rotate"])
@pytest.mark.parametrize("N,ring,k,alpha,level", [(1 << 12, lambda N: H.chain(50, 6, N), 2, 2, 3), (1 << 15, lambda N: H.chain(40, 5, N), 2, 2, 3)])
def test_on_a_dirty_workspace(N, ring, k, alpha, level, entry):
    qs = ring(N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)      # a context of its own: the block is this call's
    batch, Lk = 3, len(qs)
    polys = 3 if entry == "keyswitch" else 2
    evk, ct = operands(N, qs, k, alpha, level, polys, batch)
    devk, dct, out = dev(evk), dev(ct), tf.DeviceBuffer(batch * 2 * level * N)
    g = pow(3, N // 2 + 3, 2 * N)
    if entry == "keyswitch":
        want = KO.keyswitch_grouped_ref(ref, level, k, alpha, evk, ct)
        call = lambda: ctx.keyswitch_grouped(Lk, level, k, alpha, devk.ptr, evk.shape[0], dct.ptr, polys, out.ptr, batch)
    else:
        want = KO.rotate_grouped_ref(ref, level, k, alpha, evk, g, ct)
        call = lambda: ctx.rotate_grouped(Lk, level, k, alpha, devk.ptr, evk.shape[0], g, dct.ptr, out.ptr, batch)
    on_dirty_workspace(ctx, call, out, want, moduli=qcol(qs[:level]))
    with cap(ctx, 2):
        on_dirty_workspace(ctx, call, out, want, moduli=qcol(qs[:level]))


# ---- the mirror, end to end -------------------------------------------------------------------------------------------------------

def test_mirror_square_modswitch_and_rotate_decrypt():
    """GroupedRaised(CKKSParams, 2, 2) at N = 2^12: keygen, keygen_evalmult, encrypt, keyswitch(ek, c * c), modswitch decrypt to the
    square; a rotation by one step decrypts to the rotated slots -- both within 1e-5, the tolerance tests/test_gpu_reference_mirrors.py
    holds its ModulusRaised circuit to"""
    N = 1 << 12
    qs = H.chain(40, 3, N) + H.chain(41, 2, N)
    R = tf.NegacyclicRing(N, qs)
    params = tf.GroupedRaised(tf.CKKSParams(R, 0, 3.2), 2, 2)
    assert params.R_cipher().moduli == qs[:3] and params.R_key().moduli == qs
    rng = np.random.default_rng(21)
    kp = tf.keygen(rng, params)
    ek = tf.keygen_evalmult(rng, kp.priv)
    assert len(ek.key.key) == 2                                     # ceil(3 / 2) components over the 5-limb key ring
    scale = 2**40
    x = np.linspace(-1.0, 1.0, N // 2)
    c = tf.encrypt(rng, kp, tf.ckks_encode(x.astype(complex), params.R_cipher(), scale), scale=scale)
    assert c.ring().moduli == qs[:3]
    assert np.allclose(tf.ckks_decode(tf.decrypt(kp, c), scale).real, x, atol=1e-5)
    sq = tf.modswitch(tf.keyswitch(ek, c * c))
    assert len(sq) == 2 and sq.ring().moduli == qs[:2]
    assert np.allclose(tf.ckks_decode(tf.decrypt(kp, sq), sq.scale).real, x * x, atol=1e-5)
    gk = tf.keygen_galois(rng, kp.priv, steps=1)
    r = tf.rotate(gk, c)
    assert np.allclose(tf.ckks_decode(tf.decrypt(kp, r), r.scale).real, np.roll(x, 1), atol=1e-5)
    # a key switch at a level below the key's: the second group is cut away, one digit is left (encrypted at 2^75: 2^35 after the rescale)
    hi = tf.encrypt(rng, kp, tf.ckks_encode(x.astype(complex), params.R_cipher(), 2**75), scale=2**75)
    r2 = tf.rotate(gk, tf.modswitch(hi))
    assert r2.ring().moduli == qs[:2]
    assert np.allclose(tf.ckks_decode(tf.decrypt(kp, r2), r2.scale).real, np.roll(x, 1), atol=1e-5)
    for refused in (lambda: tf.mul_relin(ek, c, c), lambda: tf.rotate_many([gk], c), lambda: gk.prepared()):
        with pytest.raises(tf.UsageError, match="grouped digits"):
            refused()


# ---- the key-switch step against its derived noise bound --------------------------------------------------------------------------

@pytest.mark.parametrize("k,alpha,level", [(2, 2, 3), (2, 2, 2), (1, 3, 3)])
def test_key_switch_step_is_within_the_derived_bound_with_host_supplied_noise(k, alpha, level):
    """a relinearisation key made by tfhe_evalkey_gen from the grouped gadget and host-supplied draws (mask_rand, noise_rand);
    keyswitch of a uniform (c0, c1, c2) moves the phase c0 + c1 s + c2 s^2 by at most
        d N (max Q_g // 2 + 1) max|e| // P + 1 + k (1 + N max|s|)
    with the maxima of the actual draws (tests/test_ks_grouped_cpu.py derives it)"""
    N = 1 << 12
    qs = H.chain(40, 3, N) + H.chain(41, k, N)
    ctx, ref = pair(N, qs)
    Lk = len(qs)
    rng = np.random.default_rng(31 + k + level)
    gadget = KO.gadget_table(qs, k, alpha)
    D = len(gadget)
    s_int = np.rint(rng.normal(0.0, 3.2, size=(1, N))).astype(np.int64)
    s = ref.nntt(KG.small_residues(s_int, 1, qs))[0]
    mask = H.rand_residues(rng, qs, (1, D), N)
    noise = np.rint(rng.normal(0.0, 3.2, size=(1, D, N))).astype(np.int64)
    key = poisoned(D * 2 * Lk * N)
    ds, dmask, dnoise = dev(s), dev(mask), dev_i32(noise)
    ctx.evalkey_gen(Lk, ds.ptr, [key.ptr], D, gadget=gadget, galois_elements=[0], mask_rand=dmask.ptr, noise_rand=dnoise.ptr)
    ct = H.rand_residues(rng, qs[:level], (1, 3), N)
    dct, out = dev(ct), poisoned(2 * level * N)
    ctx.keyswitch_grouped(Lk, level, k, alpha, key.ptr, D, dct.ptr, 3, out.ptr, 1)
    got = out.to_numpy((2, level, N))
    evk = key.to_numpy((D, 2, Lk, N))
    assert np.array_equal(got, KO.keyswitch_grouped_ref(ref, level, k, alpha, evk, ct)[0])
    idx = list(range(level))
    sl = s[:level][None]
    mul = lambda a, b: ref.pointwise("mul", a, b, idx=idx)
    hat = lambda a: ref.nntt(a[None], idx=idx)
    before = mul(hat(ct[0, 1]), sl).astype(object) + mul(mul(hat(ct[0, 2]), sl), sl).astype(object)
    after = mul(hat(got[1]), sl)
    ql = qcol(qs[:level]).astype(object)
    diff = ref.inntt(((after.astype(object) - before) % ql[None]).astype(np.uint64), idx=idx)[0].astype(object) + got[0].astype(object) - ct[0, 0].astype(object)
    Q = math.prod(qs[:level])
    delta = KO.crt_ints(list(diff % ql), qs[:level])
    delta = max(abs(int(v) - Q if int(v) > Q // 2 else int(v)) for v in delta)
    groups = KO.groups(level, alpha)
    qg = max(math.prod(qs[i] for i in G) for G in groups)
    P = math.prod(qs[Lk - k:])
    bound = len(groups) * N * (qg // 2 + 1) * int(np.abs(noise).max()) // P + 1 + k * (1 + N * int(np.abs(s_int).max()))
    print(f"k={k} alpha={alpha} level={level}: |delta phase| = {delta}, bound = {bound}")
    assert delta <= bound, (delta, bound)
