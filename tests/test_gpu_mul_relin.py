"""tfhe_mul_relin on the device: every case bit for bit against (1) the oracle's chain enc_mul -> keyswitch -> modswitch
(ref_cpu; its enc_mul takes and returns coefficients: transforms, tensor, inverse transforms) and (2) the chain through the
existing entry points tfhe_nntt x2 -> tfhe_tensor -> tfhe_inntt -> tfhe_keyswitch(polys = 3) -> tfhe_rescale on the same
device buffers; then the decrypt-level statements, the host mirror she.mul_relin and the example's opt-in flag."""
import importlib.util
import os

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return tf.DeviceBuffer.from_numpy(a)


def chain(start, n, N):
    out, p = [], tf.nextprime(start, 1, 2 * N)
    for _ in range(n):
        out.append(p)
        p = tf.nextprime(p + 2 * N, 1, 2 * N)
    return out


def reference_ring(N):
    """infer.jl:97-112: 60-bit q0, five 40-bit primes, 60-bit special prime"""
    q0, ps = chain(2**60 + 1, 2, N)
    return [q0] + chain(2**40 + 1, 5, N) + [ps]


def fetch(buf, shape, picks):
    row = int(np.prod(shape[1:]))
    out = np.empty((len(picks),) + tuple(shape[1:]), dtype=np.uint64)
    for k, b in enumerate(picks):
        tmp = np.empty(row, dtype=np.uint64)
        tf.native.check(tf.native.lib().tfhe_memcpy_d2h(tmp.ctypes.data, buf.ptr + b * row * 8, row * 8))
        out[k] = tmp.reshape(shape[1:])
    return out


def composed(ctx, Lk, level, special, devk, ndig, d1, d2, ntt_in, rescale, batch):
    """the chain the callers assemble today, through the public entry points, on the same device buffers"""
    N = ctx.N
    if ntt_in:
        f1, f2 = d1, d2
    else:
        f1 = tf.DeviceBuffer(batch * 2 * level * N)
        ctx.nntt(d1.ptr, f1.ptr, batch * 2, level)
        f2 = f1
        if d2 is not d1:
            f2 = tf.DeviceBuffer(batch * 2 * level * N)
            ctx.nntt(d2.ptr, f2.ptr, batch * 2, level)
    ten = tf.DeviceBuffer(batch * 3 * level * N)
    ctx.tensor(f1.ptr, f2.ptr, ten.ptr, batch, level)
    ctx.inntt(ten.ptr, ten.ptr, batch * 3, level)
    rel = tf.DeviceBuffer(batch * 2 * level * N)
    ctx.keyswitch(Lk, level, special, devk.ptr, ndig, ten.ptr, 3, rel.ptr, batch)
    if not rescale:
        return rel
    out = tf.DeviceBuffer(batch * 2 * (level - 1) * N)
    ctx.rescale(rel.ptr, out.ptr, batch * 2, level)
    return out


def oracle(ref, level, special, evk, c1, c2, ntt_in, rescale):
    """c1, c2: host arrays [n][2][level][N] in the domain the call takes them"""
    n, N = c1.shape[0], c1.shape[-1]
    idx = range(level)
    if ntt_in:
        c1 = ref.inntt(c1.reshape(-1, level, N), idx=idx).reshape(c1.shape)
        c2 = ref.inntt(c2.reshape(-1, level, N), idx=idx).reshape(c2.shape)
    rel = ref.keyswitch(level, special, evk, ref.enc_mul(c1, c2, idx=idx))
    if not rescale:
        return rel
    return ref.modswitch(rel.reshape(-1, level, N), idx=idx).reshape(n, 2, level - 1, N)


def check_case(ctx, ref, qs, Lk, level, special, evk, devk, batch, square, ntt_in, rescale, seed, picks=None):
    N = ctx.N
    rng = np.random.default_rng(seed)
    c1 = H.rand_residues(rng, qs[:level], (batch, 2), N)
    c2 = c1 if square else H.rand_residues(rng, qs[:level], (batch, 2), N)
    d1 = dev(c1)
    d2 = d1 if square else dev(c2)
    lo = level - 1 if rescale else level
    out = tf.DeviceBuffer(batch * 2 * lo * N)
    ctx.mul_relin(Lk, level, special, devk.ptr, evk.shape[0], d1.ptr, d2.ptr, out.ptr, batch, ntt_in=ntt_in, rescale=rescale)
    got = out.to_numpy((batch, 2, lo, N))
    comp = composed(ctx, Lk, level, special, devk, evk.shape[0], d1, d2, ntt_in, rescale, batch)
    assert np.array_equal(got, comp.to_numpy((batch, 2, lo, N))), ("composed", level, square, ntt_in, rescale, batch)
    picks = list(range(batch)) if picks is None else picks
    want = oracle(ref, level, special, evk, c1[picks], c2[picks], ntt_in, rescale)
    assert np.array_equal(got[picks], want), ("oracle", level, square, ntt_in, rescale, batch)
    for j in range(lo):
        assert int(got[:, :, j].max()) < qs[j]


# ---- the reference's ring at its own degree: both fused cores in every call ------------------------------------------------------

@pytest.fixture(scope="module")
def ref_ring_13():
    N = 1 << 13
    qs = reference_ring(N)
    assert [q.bit_length() for q in qs] == [61, 41, 41, 41, 41, 41, 61]
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    assert ctx.psis == ref.psis
    _, evk = H.real_evk(513, N, qs, True)
    return N, qs, ctx, ref, evk, dev(evk)


@pytest.mark.parametrize("level", [6, 5, 4, 3, 2])
def test_reference_ring_every_level_and_form(ref_ring_13, level):
    N, qs, ctx, ref, evk, devk = ref_ring_13
    seed = 1300 + 16 * level
    for rescale in (0, 1):
        for square in (False, True):
            for ntt_in in (0, 1):
                seed += 1
                check_case(ctx, ref, qs, 7, level, True, evk, devk, 3, square, ntt_in, rescale, seed)


@pytest.mark.parametrize("batch", [1, 16])
def test_reference_ring_batches(ref_ring_13, batch):
    N, qs, ctx, ref, evk, devk = ref_ring_13
    for k, (square, ntt_in, rescale) in enumerate(((False, 0, 1), (True, 0, 1), (False, 1, 0), (True, 1, 1))):
        check_case(ctx, ref, qs, 7, 6, True, evk, devk, batch, square, ntt_in, rescale, 1390 + 10 * batch + k,
                   picks=None if batch == 1 else [0, 7, batch - 1])


# ---- uniform fp64-size rings --------------------------------------------------------------------------------------------------

def test_cfg4_shape_50_bit_chain_with_special_prime():
    N, L = 1 << 14, 6
    qs = H.chain(50, L + 1, N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(414)
    evk = H.uniform_evk(rng, qs, L + 1, N)
    devk = dev(evk)
    k = 0
    for square in (False, True):
        for ntt_in in (0, 1):
            for rescale in (0, 1):
                k += 1
                check_case(ctx, ref, qs, L + 1, L, True, evk, devk, 5, square, ntt_in, rescale, 1400 + k, picks=[0, 4])


def test_n_4096_40_bit_limbs_without_special_prime():
    N, L = 1 << 12, 4
    qs = H.chain(40, L, N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    _, evk = H.real_evk(412, N, qs, False)
    devk = dev(evk)
    k = 0
    for level in (4, 2, 1):
        for square in (False, True):
            for ntt_in in (0, 1):
                for rescale in ((0, 1) if level >= 2 else (0,)):
                    k += 1
                    check_case(ctx, ref, qs, L, level, False, evk, devk, 4, square, ntt_in, rescale, 1200 + k)


# ---- one limb on each side of TFHE_FP_QMAX: both cores in one call, at every fused degree ----------------------------------------

@pytest.mark.parametrize("logn", [12, 13, 14])
def test_one_limb_on_each_side_of_fp_qmax(logn):
    N = 1 << logn
    qs = [H.primes_below(H.FP_QMAX, 1, N)[0], H.primes_above(H.FP_QMAX, 1, N)[0], H.primes_below(H.Q_LIMIT, 1, N)[0]]
    assert qs[0] < H.FP_QMAX <= qs[1]
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(60 + logn)
    evk = H.uniform_evk(rng, qs, 3, N)
    devk = dev(evk)
    k = 0
    for special, level in ((True, 2), (False, 3)):
        for square in (False, True):
            for ntt_in in (0, 1):
                k += 1
                check_case(ctx, ref, qs, 3, level, special, evk, devk, 3, square, ntt_in, 1, 6000 + 100 * logn + k)


def test_u64_only_ring_at_2_14():
    """two 60-bit limbs at N = 2^14: the u64 core's allocation with two parking rows, alone in the call"""
    N = 1 << 14
    qs = H.primes_above(1 << 59, 2, N) + H.primes_below(H.Q_LIMIT, 1, N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(1460)
    evk = H.uniform_evk(rng, qs, 3, N)
    devk = dev(evk)
    for k, (square, ntt_in) in enumerate(((False, 0), (True, 0), (False, 1), (True, 1))):
        check_case(ctx, ref, qs, 3, 2, True, evk, devk, 3, square, ntt_in, 1, 1460 + k)


# ---- the composed sizes ---------------------------------------------------------------------------------------------------------

def test_cfg3_shape_n_32768():
    N, L = 1 << 15, 4
    qs = H.chain(40, L + 1, N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(315)
    evk = H.uniform_evk(rng, qs, L + 1, N)
    devk = dev(evk)
    for k, (square, ntt_in, rescale) in enumerate(((False, 0, 1), (True, 0, 1), (False, 1, 0), (True, 1, 1))):
        check_case(ctx, ref, qs, L + 1, L, True, evk, devk, 2, square, ntt_in, rescale, 3150 + k)


def test_cfg5_shape_n_65536():
    N = 1 << 16
    qs = reference_ring(N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(516)
    evk = H.uniform_evk(rng, qs, 7, N)
    devk = dev(evk)
    for k, (level, square, ntt_in, rescale) in enumerate(((6, False, 0, 1), (5, True, 0, 1), (6, True, 1, 0))):
        check_case(ctx, ref, qs, 7, level, True, evk, devk, 2, square, ntt_in, rescale, 5160 + k)


def test_generic_ntt_variant_takes_the_composed_path(ref_ring_13):
    N, qs, _, ref, evk, _ = ref_ring_13
    ctx = tf.Context(N, qs)
    ctx.set_ntt_variant(1)
    devk = dev(evk)
    for k, (square, ntt_in, rescale) in enumerate(((False, 0, 1), (True, 1, 1))):
        check_case(ctx, ref, qs, 7, 4, True, evk, devk, 2, square, ntt_in, rescale, 1310 + k)


def test_small_ring_below_the_fused_sizes():
    N, L = 1 << 10, 3
    qs = H.chain(40, L, N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    _, evk = H.real_evk(410, N, qs, False)
    check_case(ctx, ref, qs, L, L, False, evk, dev(evk), 3, False, 0, 1, 1010)
    check_case(ctx, ref, qs, L, L, False, evk, dev(evk), 3, True, 0, 0, 1011)


# ---- a batch larger than the internal chunk (256) ---------------------------------------------------------------------------------

def test_batch_larger_than_the_chunk():
    N, L, batch = 1 << 12, 2, 600
    qs = [H.chain(40, 1, N)[0], H.primes_above(1 << 59, 1, N)[0]]
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(600)
    evk = H.uniform_evk(rng, qs, L, N)
    devk = dev(evk)
    # ciphertexts on both sides of every chunk boundary (255 | 256, 511 | 512) and at the ends
    picks = [0, 1, 254, 255, 256, 257, 510, 511, 512, 513, batch - 1]
    check_case(ctx, ref, qs, L, L, False, evk, devk, batch, False, 0, 1, 601, picks=picks)
    check_case(ctx, ref, qs, L, L, False, evk, devk, batch, True, 0, 0, 602, picks=picks)


# ---- argument checks that need the ring -------------------------------------------------------------------------------------------

def test_overlapping_ranges_and_levels_are_rejected():
    N = 1 << 12
    qs = H.chain(40, 3, N)
    ctx = tf.Context(N, qs)
    buf = tf.DeviceBuffer(3 * 2 * 3 * N)
    key = tf.DeviceBuffer(3 * 2 * 3 * N)
    a, other = buf.ptr, tf.DeviceBuffer(2 * 3 * N)
    f = tf.native.lib().tfhe_mul_relin
    # out starts inside c1's range (batch 2 at level 3 is 2 * 2 * 3 * N words)
    assert f(ctx.h, 3, 3, 0, key.ptr, 3, a, a, 0, 0, a + 8 * N, 2) == tf.native.E_BADARG
    assert f(ctx.h, 3, 3, 0, key.ptr, 3, a + 8 * 6 * N, a + 8 * 6 * N, 0, 1, a, 2) == tf.native.E_BADARG   # out's end runs into c1
    assert f(ctx.h, 3, 4, 0, key.ptr, 4, a, a, 0, 0, other.ptr, 1) == tf.native.E_LEVEL
    assert f(ctx.h, 3, 3, 1, key.ptr, 3, a, a, 0, 0, other.ptr, 1) == tf.native.E_LEVEL                   # special: level <= Lk - 1
    assert f(ctx.h, 3, 3, 0, key.ptr, 2, a, a, 0, 0, other.ptr, 1) == tf.native.E_PARAMS
    assert f(ctx.h, 3, 3, 0, key.ptr, 3, a, a, 0, 0, other.ptr, 0) == tf.native.OK                        # batch == 0 does nothing


# ---- decrypt level ----------------------------------------------------------------------------------------------------------------

def test_bgv_product_mod_t_on_genuine_ciphertexts():
    """mirrors test_cfg4_bgv_product_and_keyswitch_on_genuine_ciphertexts: the product decrypts to the products mod t before the
    switch, and mul_relin(ek, c, c) is the oracle's key switch of it"""
    N, L, t = 1 << 14, 6, 257
    qs = H.chain(50, L + 1, N)
    R = tf.NegacyclicRing(N, qs)
    params = tf.ModulusRaised(tf.BGVParams(R, t))
    rng = tf.DeviceRng(46)
    kp = tf.keygen(rng, params)
    ms = [[m] + [0] * (N - 1) for m in (6, 11, 200)]
    c = tf.she.encrypt_zero(rng, kp.pub, batch=3) + params.R_cipher()(ms)
    y = c * c
    assert [d[0] for d in tf.decrypt(kp, y)] == [36, 121, 200 * 200 % t]
    ek = tf.keygen_evalmult(rng, kp.priv)
    z = tf.she.mul_relin(ek, c, c)
    assert len(z) == 2 and z.scale is None
    cin = np.stack([x.to_numpy("primal") for x in y.cs], axis=1)
    evk = ek.key.packed().to_numpy((L + 1, 2, L + 1, N))
    want = ref_cpu.RefCtx(N, qs).keyswitch(L, True, evk, cin)
    assert np.array_equal(np.stack([x.to_numpy("primal") for x in z.cs], axis=1), want)
    # without the special prime the switched product still decrypts to the product mod t (the key's noise is t e)
    p2 = tf.BGVParams(tf.NegacyclicRing(1 << 12, H.chain(50, 3, 1 << 12)), t)
    kp2 = tf.keygen(rng, p2)
    ms2 = [[m] + [0] * ((1 << 12) - 1) for m in (6, 11, 200)]
    c2 = tf.she.encrypt_zero(rng, kp2.pub, batch=3) + p2.R_cipher()(ms2)
    z2 = tf.she.mul_relin(tf.keygen_evalmult(rng, kp2.priv), c2, c2)
    assert [d[0] for d in tf.decrypt(kp2, z2)] == [36, 121, 200 * 200 % t]


def test_ckks_square_with_rescale_decodes_to_x_squared():
    """the circuit of test_cfg5_ckks_mnist_ring_decrypt_level (x*x -> relinearise -> rescale) at the reference's own degree,
    within that test's tolerance"""
    N = 1 << 13
    R = tf.NegacyclicRing(N, reference_ring(N))
    params = tf.ModulusRaised(tf.CKKSParams(R, 0, 3.2))
    rng = tf.DeviceRng(513)
    kp = tf.keygen(rng, params)
    scale = 2**40
    x = np.linspace(-1.5, 1.5, N // 2).astype(complex)
    c = tf.encrypt(rng, kp, tf.ckks_encode(x, params.R_cipher(), scale), scale=scale)
    ek = tf.keygen_evalmult(rng, kp.priv)
    sq = tf.she.mul_relin(ek, c, c, rescale=True)
    assert sq.ring().L == 5
    got = tf.ckks_decode(tf.decrypt(kp, sq), sq.scale)
    assert np.abs(got - x * x).max() < 1e-4


# ---- the host mirror ----------------------------------------------------------------------------------------------------------------

def _same(a, b):
    assert len(a) == len(b) == 2 and a.scale == b.scale and a.ring().moduli == b.ring().moduli
    for x, y in zip(a.cs, b.cs):
        assert np.array_equal(x.to_numpy("primal"), y.to_numpy("primal"))


@pytest.mark.parametrize("raised", [True, False])
@pytest.mark.parametrize("batch", [None, 3])
def test_she_mul_relin_matches_the_composed_mirror(raised, batch):
    N = 1 << 13
    qs = reference_ring(N)
    inner = tf.CKKSParams(tf.NegacyclicRing(N, qs if raised else qs[:-1]), 0, 3.2)
    params = tf.ModulusRaised(inner) if raised else inner
    rng = tf.DeviceRng(77)
    kp = tf.keygen(rng, params)
    ek = tf.keygen_evalmult(rng, kp.priv)
    scale = 2**40
    n = batch or 1
    xs = np.linspace(-1, 1, n * (N // 2)).reshape(n, N // 2).astype(complex)
    x = xs if batch else xs[0]
    c = tf.encrypt(rng, kp, tf.ckks_encode(x, params.R_cipher(), scale), scale=scale)
    d = tf.encrypt(rng, kp, tf.ckks_encode(x[..., ::-1].copy(), params.R_cipher(), scale), scale=scale)
    for rescale in (True, False):
        want = tf.keyswitch(ek, c * c)
        _same(tf.she.mul_relin(ek, c, c, rescale=rescale), tf.modswitch(want) if rescale else want)
        want = tf.keyswitch(ek, c * d)
        _same(tf.she.mul_relin(ek, c, d, rescale=rescale), tf.modswitch(want) if rescale else want)
    # a chained call takes the unsplit packed result of the previous one; operands that exist only as NTT images go in as such
    r1 = tf.she.mul_relin(ek, c, c, rescale=True)
    w1 = tf.modswitch(tf.keyswitch(ek, c * c))
    _same(tf.she.mul_relin(ek, r1, r1, rescale=True), tf.modswitch(tf.keyswitch(ek, w1 * w1)))
    m = c.mul_plain(0.5)
    _same(tf.she.mul_relin(ek, m, m, rescale=True), tf.modswitch(tf.keyswitch(ek, m * m)))


def test_she_mul_relin_windowed_key_and_foreign_parameters():
    N = 1 << 12
    R = tf.NegacyclicRing(N, H.chain(40, 3, N))
    params = tf.CKKSParams(R, 8, 3.2)                              # relin_window = 8: the composed path
    rng = tf.DeviceRng(78)
    kp = tf.keygen(rng, params)
    ek = tf.keygen_evalmult(rng, kp.priv)
    scale = 2**30
    x = np.linspace(-1, 1, N // 2).astype(complex)
    c = tf.encrypt(rng, kp, tf.ckks_encode(x, params.R_cipher(), scale), scale=scale)
    _same(tf.she.mul_relin(ek, c, c, rescale=True), tf.modswitch(tf.keyswitch(ek, c * c)))
    _same(tf.she.mul_relin(ek, c, c), tf.keyswitch(ek, c * c))
    other = tf.CKKSParams(R, 8, 3.2)
    kq = tf.keygen(rng, other)
    d = tf.encrypt(rng, kq, tf.ckks_encode(x, other.R_cipher(), scale), scale=scale)
    with pytest.raises(tf.UsageError):
        tf.she.mul_relin(ek, c, d)
    # BFV multiplies through its plan
    ch = H.chain(50, 5, N)
    bp = tf.BFVParams(tf.NegacyclicRing(N, ch[:2]), tf.NegacyclicRing(N, ch), 65537)
    kb = tf.keygen(rng, bp)
    cb = tf.encrypt(rng, kb, [3] + [0] * (N - 1))
    with pytest.raises(tf.UsageError, match="plan"):
        tf.she.mul_relin(tf.keygen_evalmult(rng, kb.priv), cb, cb)


# ---- the example's opt-in flag ------------------------------------------------------------------------------------------------------

def test_example_flag_gives_identical_logits():
    spec = importlib.util.spec_from_file_location("encrypted_mnist_example", os.path.join(ROOT, "examples", "encrypted_mnist.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    base = ex.run(logn=12, seed=3, verbose=False, model="synthetic", return_logits=True)
    flag = ex.run(logn=12, seed=3, verbose=False, model="synthetic", return_logits=True, mul_relin=True)
    assert np.array_equal(base[3], flag[3])
    assert base[:3] == flag[:3]
