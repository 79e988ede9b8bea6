"""tfhe_mul_relin_grouped on the device against tests/mul_relin_grouped_oracle.py -- the chain tfhe_nntt x2 -> tfhe_tensor -> tfhe_inntt
-> tfhe_keyswitch_grouped(polys = 3) [-> tfhe_rescale] -- word for word, into poisoned buffers, every word read back below its
modulus: the two degenerate cases against tfhe_mul_relin itself; the shape matrix, every shape with and without the rescale, on
coefficient-domain operands and on NTT images, squaring and a general product (every K of the rescaling tail, ragged groups, levels
down to 2, 34 working limbs, no special prime, one digit, the fused product cores, a mixed ring on both lanes, N = 2^15); special
primes below and above every ciphertext limb; an output that is not 16-byte aligned; batches under every chunk cap; every word at
q - 1; a dirty workspace; every host check with a context; the mirror on packed operands and on NTT images, decrypting to the product;
and the encrypted-MNIST example with its square layers through the one call."""
import importlib.util
import os

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import helpers as H
from tests import mul_relin_grouped_oracle as MO
from tests.dirty_ws import on_dirty_workspace
from tests.test_gpu_chunk_seams import cap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)


def dev(a):
    return tf.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.uint64))


def poisoned(words):
    return dev(np.full(words, POISON, dtype=np.uint64))


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


def operands(N, qs, k, alpha, level, batch, seed=0, spare=1, edge=False):
    """a uniform key of ceil(level / alpha) + spare components and two uniform ciphertexts (edge: every word q - 1)"""
    rng = np.random.default_rng(N % 991 + 13 * len(qs) + 5 * k + alpha + level + seed)
    nd = -(-level // min(alpha, level)) + spare
    if edge:
        evk = np.broadcast_to(qcol(qs) - np.uint64(1), (nd, 2, len(qs), N)).copy()
        c1 = np.broadcast_to(qcol(qs[:level]) - np.uint64(1), (batch, 2, level, N)).copy()
        return evk, c1, c1.copy()
    return H.uniform_evk(rng, qs, nd, N), H.rand_residues(rng, qs[:level], (batch, 2), N), H.rand_residues(rng, qs[:level], (batch, 2), N)


class Case:
    """one (ring, gadget, level, key, operands) with its oracle words, computed once: the key switch of the square and of the general
    product (the rescaled words and those on NTT images follow from them)"""

    def __init__(self, N, qs, k, alpha, level, batch, seed=0, edge=False, spare=1):
        self.N, self.qs, self.k, self.alpha, self.level, self.batch = N, qs, k, alpha, level, batch
        self.ctx, self.ref = pair(N, qs)
        self.evk, self.c1, self.c2 = operands(N, qs, k, alpha, level, batch, seed, spare, edge)
        idx = list(range(level))
        self.ntt = {id(c): self.ref.nntt(c.reshape(-1, level, N), idx=idx).reshape(c.shape) for c in (self.c1, self.c2)}
        self.want = {}
        for square in (True, False):
            ks = MO.mul_relin_grouped_ref(self.ref, level, k, alpha, self.evk, self.c1, self.c1 if square else self.c2)
            self.want[square, 0] = ks
            if level >= 2:
                self.want[square, 1] = MO.rescale_ref(self.ref, level, ks)
        self.devk = dev(self.evk)
        self.dev = {(ntt_in, id(c)): dev(self.ntt[id(c)] if ntt_in else c) for ntt_in in (0, 1) for c in (self.c1, self.c2)}

    def call(self, out_ptr, square, ntt_in, rescale, ctx=None):
        a, b = self.dev[ntt_in, id(self.c1)], self.dev[ntt_in, id(self.c1 if square else self.c2)]
        (ctx or self.ctx).mul_relin_grouped(len(self.qs), self.level, self.k, self.alpha, self.devk.ptr, self.evk.shape[0], a.ptr, b.ptr, out_ptr,
                                            self.batch, ntt_in=ntt_in, rescale=rescale)

    def check(self, square, ntt_in, rescale, offset=0):
        lo = self.level - rescale
        words = self.batch * 2 * lo * self.N
        out = poisoned(words + offset)
        self.call(out.ptr + 8 * offset, square, ntt_in, rescale)
        raw = out.to_numpy()
        assert (raw[:offset] == POISON).all()
        got = raw[offset:].reshape(self.batch, 2, lo, self.N)
        assert (got < qcol(self.qs[:lo])).all(), (square, ntt_in, rescale)
        want = self.want[square, rescale]
        assert np.array_equal(got, want), (self.N, self.k, self.alpha, self.level, square, ntt_in, rescale, int((got != want).sum()))
        return got

    def check_all(self):
        for rescale in ((0, 1) if self.level >= 2 else (0,)):
            for ntt_in in (0, 1):
                for square in (True, False):
                    self.check(square, ntt_in, rescale)


# ---- degenerate parity: the words of tfhe_mul_relin ---------------------------------------------------------------------------

@pytest.mark.parametrize("special", [1, 0])
@pytest.mark.parametrize("N,bits,Lk", [(64, 30, 4), (1 << 12, 50, 4), (1 << 15, 40, 4)])
def test_one_limb_per_digit_is_tfhe_mul_relin(N, bits, Lk, special):
    qs = H.chain(bits, Lk, N)
    ctx, _ = pair(N, qs)
    level, batch = Lk - special, 2
    evk, c1, c2 = operands(N, qs, special, 1, level, batch, spare=special)   # (tfhe_mul_relin reads `level` components)
    devk, d1, d2 = dev(evk), dev(c1), dev(c2)
    for rescale in (0, 1):
        for b in (d1, d2):                                  # a square and a general product
            words = batch * 2 * (level - rescale) * N
            x, y = poisoned(words), poisoned(words)
            ctx.mul_relin(Lk, level, special, devk.ptr, evk.shape[0], d1.ptr, b.ptr, x.ptr, batch, rescale=rescale)
            ctx.mul_relin_grouped(Lk, level, special, 1, devk.ptr, evk.shape[0], d1.ptr, b.ptr, y.ptr, batch, rescale=rescale)
            got = y.to_numpy((batch, 2, level - rescale, N))
            assert (got < qcol(qs[:level - rescale])).all()
            assert np.array_equal(x.to_numpy(), y.to_numpy()), (N, special, rescale, b is d1)


# ---- the shape matrix ---------------------------------------------------------------------------------------------------------

def _mixed13(N):
    return H.chain(61, 1, N) + H.chain(40, 3, N) + H.chain(41, 2, N)


SHAPES = [  # (N, moduli of the key ring, k, alpha, level, batch)
    pytest.param(64, lambda N: H.chain(30, 8, N), 2, 2, 6, 2, id="64-8x30-k2-a2-level6"),
    pytest.param(64, lambda N: H.chain(30, 8, N), 2, 2, 3, 2, id="64-8x30-k2-a2-level3"),
    pytest.param(64, lambda N: H.chain(30, 8, N), 2, 2, 2, 2, id="64-8x30-k2-a2-level2-one-output-limb"),
    pytest.param(64, lambda N: H.chain(30, 8, N), 1, 2, 5, 2, id="64-k1"),
    pytest.param(64, lambda N: H.chain(30, 8, N), 3, 2, 5, 2, id="64-k3"),
    pytest.param(64, lambda N: H.chain(30, 8, N), 4, 2, 4, 2, id="64-k4"),
    pytest.param(64, lambda N: H.chain(30, 10, N), 3, 3, 7, 2, id="64-k3-a3-level7-ragged"),
    pytest.param(64, lambda N: H.chain(30, 34, N), 4, 5, 30, 1, id="64-34x30-k4-a5-level30-across-the-32-limb-seam"),
    pytest.param(64, lambda N: H.chain(30, 6, N), 0, 4, 6, 2, id="64-k0-composed-tail"),
    pytest.param(64, lambda N: H.chain(30, 6, N), 0, 1, 2, 2, id="64-k0-level2"),
    pytest.param(64, lambda N: H.chain(30, 7, N), 1, 9, 6, 2, id="64-one-digit-group-above-level"),
    pytest.param(1 << 12, lambda N: H.chain(50, 7, N), 2, 2, 5, 2, id="4096-7x50-k2-a2-level5-fused-cores"),
    pytest.param(1 << 13, _mixed13, 2, 2, 4, 2, id="8192-61+3x40+2x41-k2-both-lanes"),
    pytest.param(1 << 15, lambda N: H.chain(40, 6, N), 2, 2, 4, 1, id="32768-6x40-k2-level4"),
    pytest.param(1 << 15, lambda N: H.chain(40, 6, N), 2, 2, 3, 1, id="32768-6x40-k2-level3"),
]


@pytest.mark.parametrize("N,ring,k,alpha,level,batch", SHAPES)
def test_shape_matrix_matches_the_oracle(N, ring, k, alpha, level, batch):
    Case(N, ring(N), k, alpha, level, batch).check_all()


@pytest.mark.parametrize("ct_bits,sp_bits", [(40, 30), (30, 50), (50, 61), (61, 30)])
def test_special_primes_below_and_above_every_ciphertext_limb(ct_bits, sp_bits):
    N = 256
    Case(N, H.chain(ct_bits, 4, N) + H.chain(sp_bits, 3, N), 3, 2, 4, 2).check_all()


# ---- alignment: an output at an 8-byte but not 16-byte offset takes one coefficient per thread ---------------------------------

@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (1 << 12, lambda N: H.chain(50, 6, N), 3, 2, 3)])
def test_an_output_that_is_not_16_byte_aligned_gets_the_same_words(N, ring, k, alpha, level):
    case = Case(N, ring(N), k, alpha, level, 2, seed=3)
    for rescale in (0, 1):
        for square in (True, False):
            assert np.array_equal(case.check(square, 0, rescale, offset=1), case.check(square, 0, rescale))


# ---- batches and chunks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", [3, 5])
@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (1 << 12, lambda N: H.chain(50, 6, N), 2, 3, 4)])
def test_batches_under_every_chunk_cap(N, ring, k, alpha, level, batch):
    case = Case(N, ring(N), k, alpha, level, batch, seed=batch)
    for rescale in (0, 1):
        whole = case.check(False, 0, rescale)
        for c in (1, 2):
            with cap(case.ctx, c):
                assert np.array_equal(case.check(False, 0, rescale), whole)
                assert np.array_equal(case.check(True, 1, rescale), case.want[True, rescale])


# ---- edge inputs ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (1 << 12, lambda N: H.chain(40, 7, N), 3, 3, 4),
                                                  (1 << 13, _mixed13, 2, 2, 4), (256, lambda N: H.chain(61, 6, N), 2, 4, 4)])
def test_every_operand_and_key_word_q_minus_1(N, ring, k, alpha, level):
    Case(N, ring(N), k, alpha, level, 2, edge=True).check_all()


# ---- on a dirty workspace -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rescale", [0, 1])
@pytest.mark.parametrize("N,ring,k,alpha,level", [(1 << 12, lambda N: H.chain(50, 6, N), 2, 2, 3), (1 << 15, lambda N: H.chain(40, 5, N), 2, 2, 3),
                                                  (256, lambda N: H.chain(30, 5, N), 0, 2, 4)])
def test_on_a_dirty_workspace(N, ring, k, alpha, level, rescale):
    qs = ring(N)
    case = Case(N, qs, k, alpha, level, 3)
    ctx = tf.Context(N, qs)                                  # a context of its own: the block is this call's
    lo = level - rescale
    out = tf.DeviceBuffer(3 * 2 * lo * N)
    call = lambda: case.call(out.ptr, False, 0, rescale, ctx=ctx)
    on_dirty_workspace(ctx, call, out, case.want[False, rescale], moduli=qcol(qs[:lo]))
    with cap(ctx, 2):
        on_dirty_workspace(ctx, call, out, case.want[False, rescale], moduli=qcol(qs[:lo]))


# ---- the host checks, with a context ----------------------------------------------------------------------------------------

def test_host_checks_in_the_headers_order_leave_the_output_untouched():
    N = 64
    qs = H.chain(30, 6, N)
    ctx, _ = pair(N, qs)
    ct_words = 2 * 4 * N
    buf = poisoned(3 * ct_words)
    a, b, o = buf.ptr, buf.ptr + 8 * ct_words, buf.ptr + 16 * ct_words

    def mr(Lk=6, level=4, k=2, group=2, evk=a, nd=2, c1=a, c2=b, ntt_in=0, rescale=0, out=o, batch=1):
        tf.native.check(tf.native.lib().tfhe_mul_relin_grouped(ctx.h, Lk, level, k, group, evk, nd, c1, c2, ntt_in, rescale, out, batch))

    for kw in (dict(evk=None, batch=-1), dict(c1=None, ntt_in=2), dict(c2=None, Lk=0), dict(out=None, k=9)):
        with pytest.raises(AssertionError, match="null argument"):
            mr(**kw)
    with pytest.raises(AssertionError, match="negative batch"):
        mr(batch=-1, ntt_in=2, out=a)
    for kw in (dict(ntt_in=2), dict(rescale=-1), dict(rescale=2, level=1)):
        with pytest.raises(AssertionError, match="ntt_in and rescale are 0 or 1"):
            mr(out=a, **kw)
    with pytest.raises(tf.UsageError, match="needs level >= 2"):
        mr(rescale=1, level=1, out=a)
    for kw in (dict(out=a), dict(out=b), dict(out=a, c2=a)):
        with pytest.raises(AssertionError, match="out overlaps an operand"):
            mr(Lk=0, **kw)
    for lk in (0, 7):
        with pytest.raises(AssertionError, match="key_limbs"):
            mr(Lk=lk, k=5, out=a + 8)
    for k in (-1, 5):
        with pytest.raises(AssertionError, match="n_special"):
            mr(k=k, group=0, out=a + 8)
    with pytest.raises(AssertionError, match="group"):
        mr(group=0, level=0, out=a + 8)
    for lv in (0, 5):
        with pytest.raises(tf.UsageError, match="level"):
            mr(level=lv, nd=0, out=a + 8)
    with pytest.raises(tf.UsageError, match="components"):
        mr(nd=1, out=a + 8)
    for kw in (dict(out=a + 8), dict(out=b - 8), dict(out=b + 8, rescale=1), dict(out=b - 8 * 2 * 3 * N + 8, rescale=1)):
        with pytest.raises(AssertionError, match="out overlaps an operand"):
            mr(**kw)
    with pytest.raises(AssertionError, match="bad batch"):
        mr(batch=1 << 27, c1=1 << 40, c2=1 << 41, out=1 << 50)
    mr(batch=0)                                              # an empty batch: TFHE_OK, nothing written
    mr(batch=0, out=a + 8, rescale=1)
    ctx.sync()
    assert (buf.to_numpy() == POISON).all()


# ---- the mirror -------------------------------------------------------------------------------------------------------------------

def _ntt_only(c):
    """a copy of a 2-element ciphertext whose components hold their NTT images and no coefficient image"""
    out = tf.CipherText(c.params, [tf.RingElement(x.ring, dual=x.coeffs_dual(), batch=x.batch) for x in c.cs], c.scale)
    assert all(p.primal is None and p.dual is not None for p in out.cs)
    return out


def _words(c):
    return [p.to_numpy() for p in c.cs]


@pytest.mark.parametrize("N", [64, 1 << 12])
def test_mirror_equals_the_composed_calls_and_decrypts_to_the_product(N):
    """GroupedRaised(CKKSParams, 2, 2): tf.mul_relin_grouped(ek, c1, c2, rescale) is modswitch(keyswitch(ek, c1 * c2)) / keyswitch(ek,
    c1 * c2) word for word, on packed inputs and on inputs that exist only as NTT images, and (three 40-bit limbs, two 41-bit special primes,
    scale 2^40) decrypts to the product of the plaintexts within 1e-5, the tolerance tests/test_gpu_ks_grouped.py uses for its end-to-end case"""
    qs = H.chain(40, 3, N) + H.chain(41, 2, N)
    R = tf.NegacyclicRing(N, qs)
    params = tf.GroupedRaised(tf.CKKSParams(R, 0, 3.2), 2, 2)
    level = len(qs) - 2
    rng = np.random.default_rng(21)
    kp = tf.keygen(rng, params)
    ek = tf.keygen_evalmult(rng, kp.priv)
    assert len(ek.key.key) == -(-level // 2)
    scale = 2**40
    x, y = np.linspace(-1.0, 1.0, N // 2), np.cos(np.linspace(0.0, 3.0, N // 2))
    enc = lambda v: tf.encrypt(rng, kp, tf.ckks_encode(v.astype(complex), params.R_cipher(), scale), scale=scale)
    cx, cy = enc(x), enc(y)

    for rescale in (False, True):
        for a, b, plain in ((cx, cx, x * x), (cx, cy, x * y)):
            composed = tf.keyswitch(ek, a * b)
            composed = tf.modswitch(composed) if rescale else composed
            one = tf.mul_relin_grouped(ek, a, b, rescale=rescale)
            assert len(one) == 2 and one.ring().moduli == qs[:level - int(rescale)] and one.scale == composed.scale
            want = _words(composed)
            for p, q in zip(_words(one), want):
                assert np.array_equal(p, q), (N, rescale, a is b)
            an = _ntt_only(a)                                 # operands that exist only as NTT images go in as they are (ntt_in)
            again = tf.mul_relin_grouped(ek, an, an if b is a else _ntt_only(b), rescale=rescale)
            assert all(p.primal is None for p in an.cs)
            for p, q in zip(_words(again), want):
                assert np.array_equal(p, q), (N, rescale, a is b, "ntt_in")
            assert np.allclose(tf.ckks_decode(tf.decrypt(kp, one), one.scale).real, plain, atol=1e-5)
    for refused in (lambda: tf.mul_relin(ek, cx, cx), lambda: tf.mul_relin(ek, cx, cy, rescale=True)):
        with pytest.raises(tf.UsageError, match="mul_relin has no support for keys with grouped digits"):
            refused()


# ---- the example ------------------------------------------------------------------------------------------------------------------

def test_example_square_layers_through_the_one_call_give_bit_identical_logits():
    spec = importlib.util.spec_from_file_location("encrypted_mnist_example", os.path.join(ROOT, "examples", "encrypted_mnist.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    kw = dict(logn=13, seed=1, verbose=False, model="reference", hoisted=True, fused=True, return_logits=True, grouped=(3, 3))
    base = ex.run(**kw)
    got = ex.run(mul_relin_grouped=True, **kw)
    assert base[1] > 1.0 and got[3].shape == base[3].shape
    assert np.array_equal(got[3].argmax(0), base[3].argmax(0))
    assert np.array_equal(got[3], base[3]), float(np.abs(got[3] - base[3]).max())
    for bad in (dict(hoisted=True), dict()):
        with pytest.raises(ValueError, match="mul_relin_grouped"):
            ex.run(logn=13, seed=1, verbose=False, mul_relin_grouped=True, **bad)
