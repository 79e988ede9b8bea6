"""The rectangular matrix product through the mirror: she.rotate_sum (tfhe_rotate_sum) and she.matmul_bsgs_fold (tfhe_matmul_bsgs_fold)
against the compositions of public calls they replace, word for word -- every step is exact arithmetic on canonical residues -- and at
the decrypt level: the extended diagonals and fold steps of she.rect_diagonals give W @ x for wide matrices, for a wide layer followed
by a tall one, and for the last layer of examples/encrypted_mnist.py (--rect)."""
import numpy as np
import pytest

import toyfhe_jl_amd as tf
from tests.test_gpu_matmul_bsgs_blocks import _add_bias, _bias, _composition, _ring, _rows, _same_words, _setup, chain

pytestmark = pytest.mark.gpu


def _rotate_sum_chain(groups, c):
    """per group rotate_many -> +"""
    for grp in groups:
        f = c
        for r in tf.rotate_many(grp, c):
            f = f + r
        c = f
    return c


def _fold_keys(kp, seed, steps):
    rng = tf.DeviceRng(seed)
    return [tf.keygen_galois_many(rng, kp.priv, steps=list(grp)) for grp in steps]


@pytest.mark.parametrize("raised", [True, False])
@pytest.mark.parametrize("batch", [None, 3])
def test_rotate_sum_is_word_for_word_rotate_many_and_add(raised, batch):
    """N = 2^10: one-key steps, a three-key step and both mixed; with the special prime the sum is formed in the evaluation domain
    (k_md_fold), without it in the coefficient domain"""
    N = 1 << 10
    kp, cs, _, _, _, _ = _setup(N, _ring(N, [60, 40, 40, 60] if raised else [60, 40, 40]), raised, 0, 0, 1, batch, 3100)
    c = cs[0]
    for steps in ([[8]], [[8], [16], [32]], [[4, 8, 12]], [[4, 8, 12], [16]]):
        groups = _fold_keys(kp, 3101, steps)
        got = tf.rotate_sum(groups, c)
        assert got.scale == c.scale and all(x.primal is not None for x in got.cs)      # c's scale, coefficient domain
        _same_words(got, _rotate_sum_chain(groups, c), steps)
    lo = tf.modswitch(c)                                                                  # a level below the keys
    groups = _fold_keys(kp, 3102, [[4, 8, 12], [16]])
    _same_words(tf.rotate_sum(groups, lo), _rotate_sum_chain(groups, lo), "lower level")


@pytest.mark.parametrize("raised", [True, False])
def test_matmul_bsgs_fold_is_word_for_word_blocks_rotate_sum_and_bias(raised):
    """N = 2^10, two inputs, 2 baby and 2 giant steps, a batch of 2: fold steps (1, 1) and (3,), with and without the bias; without
    fold steps the words of matmul_bsgs_blocks"""
    N, n_baby, n_giant, n_in, batch = 1 << 10, 2, 2, 2, 2
    kp, cs, baby, giant, dv, bv = _setup(N, _ring(N, [60, 40, 40, 60] if raised else [60, 40, 40]), raised, n_baby, n_giant, n_in, batch, 3200)
    rows = _rows(dv, cs[0][0].ring, cs[0].scale, n_baby, n_giant)
    bias = _bias(bv, cs[0])
    for steps in ([[16], [32]], [[16, 32, 48]]):
        groups = _fold_keys(kp, 3201, steps)
        for b in (bias, None):
            want = _add_bias(tf.rotate_sum(groups, tf.matmul_bsgs_blocks(baby, giant, rows, cs)), b, batch)
            got = tf.matmul_bsgs_fold(baby, giant, rows, cs, groups, b)
            assert got.scale == cs[0].scale ** 2 and all(x.primal is not None for x in got.cs)
            _same_words(got, want, (steps, b is not None))
            # ... and of the public calls underneath
            _same_words(got, _add_bias(_rotate_sum_chain(groups, _composition(baby, giant, rows, cs, batch)), b, batch), (steps, "chain"))
    _same_words(tf.matmul_bsgs_fold(baby, giant, rows, cs, [], bias), tf.matmul_bsgs_blocks(baby, giant, rows, cs, bias), "no fold step")


# ---- decrypt level -----------------------------------------------------------------------------------------------------------

def _small():
    """the parameters of test_decrypts_to_the_matrix_product: N = 64, 4 x 40 bits, ModulusRaised, scale 2^40, 8 rows of 4 slots"""
    N = 64
    R = tf.NegacyclicRing(N, chain(2**40 + 1, 4, N))
    params = tf.ModulusRaised(tf.CKKSParams(R, 0, 3.2))
    rng = np.random.default_rng(13)
    return N, params, rng, tf.keygen(rng, params), 2**40


def _rect_layer(rng, kp, params, W, c, n1, block, radix=2):
    """W @ (the rows of c) through rect_diagonals + matmul_bsgs_fold, the diagonals encoded at c's scale"""
    D, bsteps, gsteps, fsteps = tf.rect_diagonals(W, n1, block=block, fold_radix=radix)
    baby = [tf.keygen_galois(rng, kp.priv, steps=s) for s in bsteps]
    giant = [tf.keygen_galois(rng, kp.priv, steps=s) for s in gsteps]
    folds = [[tf.keygen_galois(rng, kp.priv, steps=s) for s in grp] for grp in fsteps]
    enc = tf.ckks_encode(D.reshape(-1, D.shape[-1]).astype(complex), c[0].ring, c.scale)
    return tf.matmul_bsgs_fold(baby, giant, [enc], [c], folds)


@pytest.mark.parametrize("m0", [2, 3])
def test_wide_product_decrypts_to_the_matrix_product(m0):
    """W is m0 x 8 in blocks of 4 slots, n1 = 2: the slots equal W @ x replicated over the 8 rows (3 x 8: the padded fourth row reads
    0), to atol = 1e-5, the bound of test_decrypts_to_the_matrix_product; both fold radices.  The maximum errors are printed."""
    N, params, rng, kp, scale = _small()
    n, B = 8, 4
    x = rng.normal(0, 1, N // 2)
    W = rng.normal(0, 1, (m0, n))
    c = tf.encrypt(rng, kp, tf.ckks_encode(x.astype(complex), params.R_cipher(), scale), scale=scale)
    m = 1 << (m0 - 1).bit_length()
    want = np.zeros((m, B))
    want[:m0] = W @ x.reshape(n, B)
    want = np.tile(want, (n // m, 1))
    for radix in (2, 4):
        res = _rect_layer(rng, kp, params, W, c, 2, B, radix)
        got = tf.ckks_decode(tf.decrypt(kp, res), res.scale).real.reshape(n, B)
        print(f"{m0} x 8, fold radix {radix}: max |error| {np.abs(got - want).max():.3e}")
        assert np.allclose(got, want, atol=1e-5)


def test_wide_then_tall_decrypts_to_the_product_of_both():
    """a 2 x 8 layer, then an 8 x 2 layer on its replicated output (5 x 40 bits: one modswitch between them); to atol = 1e-5"""
    N = 64
    R = tf.NegacyclicRing(N, chain(2**40 + 1, 5, N))
    params = tf.ModulusRaised(tf.CKKSParams(R, 0, 3.2))
    rng = np.random.default_rng(14)
    kp = tf.keygen(rng, params)
    scale, n, B = 2**40, 8, 4
    x = rng.normal(0, 1, N // 2)
    W1, W2 = rng.normal(0, 1, (2, n)), rng.normal(0, 1, (n, 2))
    c = tf.encrypt(rng, kp, tf.ckks_encode(x.astype(complex), params.R_cipher(), scale), scale=scale)
    mid = tf.modswitch(_rect_layer(rng, kp, params, W1, c, 2, B))
    res = _rect_layer(rng, kp, params, W2, mid, 2, B)
    got = tf.ckks_decode(tf.decrypt(kp, res), res.scale).real.reshape(n, B)
    want = W2 @ (W1 @ x.reshape(n, B))
    print(f"2 x 8 then 8 x 2: max |error| {np.abs(got - want).max():.3e}")
    assert np.allclose(got, want, atol=1e-5)


def test_encrypted_mnist_with_the_rectangular_last_layer():
    """examples/encrypted_mnist.py --bsgs 4 --rect at the reference's parameters (N = 2^13, the infer.jl ring, the trained model, two
    ciphertext sets): the bound and shape of test_encrypted_mnist_by_baby_and_giant_steps"""
    import importlib.util
    import os
    spec_ = importlib.util.spec_from_file_location("encrypted_mnist", os.path.join(os.path.dirname(__file__), "..", "examples", "encrypted_mnist.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    err, rng_, agree = mod.run(logn=13, seed=1, verbose=False, model="reference", batches=2, bsgs=4, rect=True)
    print(f"--bsgs 4 --rect: max |encrypted - plaintext| {err:.3e}, logit range {rng_:.2f}, argmax agreement {agree}")
    assert rng_ > 1.0 and err < 1e-3 and agree == 1.0
