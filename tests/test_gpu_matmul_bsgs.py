"""tfhe_matmul_bsgs (she.matmul_bsgs): the diagonal matrix product by baby and giant steps in one device call, against the composition
of public calls it replaces -- rotate_many over the baby keys, the forward transforms and dot_plain per giant step, the inverse
transforms, rotate per giant step, + -- word for word: every step is exact arithmetic on canonical residues."""
import numpy as np
import pytest

import toyfhe_jl_amd as tf

pytestmark = pytest.mark.gpu


def chain(start, n, N):
    """n primes = 1 mod 2N from `start` upwards"""
    out, p = [], tf.nextprime(start, 1, 2 * N)
    for _ in range(n):
        out.append(p)
        p = tf.nextprime(p + 2 * N, 1, 2 * N)
    return out


def _ring(N, bits):
    qs, used = [], set()
    for b in bits:
        q = tf.nextprime(2**b + 1, 1, 2 * N)
        while q in used:
            q = tf.nextprime(q + 2 * N, 1, 2 * N)
        used.add(q); qs.append(q)
    return qs


def _setup(N, qs, raised, n_baby, n_giant, batch, seed, scale=2**30, steps=None):
    params = tf.CKKSParams(tf.NegacyclicRing(N, qs), 0, 3.2)
    if raised:
        params = tf.ModulusRaised(params)
    rng = tf.DeviceRng(seed)
    kp = tf.keygen(rng, params)
    nrng = np.random.default_rng(seed)
    shape = (N // 2,) if batch is None else (batch, N // 2)
    c = tf.encrypt(rng, kp, tf.ckks_encode(nrng.normal(0, 1, shape).astype(complex), params.R_cipher(), scale), scale=scale)
    if steps is None:
        steps = list(range(1, n_baby + 1)), [j * (n_baby + 1) for j in range(1, n_giant + 1)]
    baby = tf.keygen_galois_many(rng, kp.priv, steps=steps[0])
    giant = tf.keygen_galois_many(rng, kp.priv, steps=steps[1])
    dv = nrng.normal(0, 1, ((n_giant + 1) * (n_baby + 1), N // 2)).astype(complex)
    return kp, c, baby, giant, dv


def _rows(dv, ring, scale, n_baby, n_giant):
    return [[tf.ckks_encode(dv[j * (n_baby + 1) + i], ring, scale) for i in range(n_baby + 1)] for j in range(n_giant + 1)]


def _composition(baby, giant, rows, c, batch):
    """rotate_many -> (nntt) dot_plain per giant step -> (inntt) rotate per giant step j >= 1 -> +"""
    rots = [c] + list(tf.rotate_many(baby, c))
    bc = lambda d: d if batch is None else d.broadcast_to(batch)
    inner = [tf.CipherText.dot_plain(rots, [bc(d) for d in row]) for row in rows]
    res = inner[0]
    for gk, x in zip(giant, inner[1:]):
        res = res + tf.rotate(gk, x)
    return res


def _same_words(got, want, what=None):
    assert got.scale == want.scale and len(got) == 2
    for a, b in zip(got.cs, want.cs):
        assert np.array_equal(a.to_numpy(), b.to_numpy()), what


CASES = [(6, [40, 40, 40, 40], 3, 2, None, True), (12, [60, 40, 40, 60], 2, 2, 3, True), (14, [50, 50, 50, 50], 2, 1, 2, True),
         (15, [40, 40, 40, 40], 1, 2, 2, True), (16, [60, 40, 40, 40, 60], 1, 1, 2, True),
         (12, [60, 40, 40], 2, 2, 3, False), (16, [50, 50, 50], 1, 1, 2, False)]


@pytest.mark.parametrize("logn,bits,n_baby,n_giant,batch,raised", CASES)
def test_matmul_bsgs_is_word_for_word_the_composition(logn, bits, n_baby, n_giant, batch, raised):
    """uniform rings, the mixed 60/40-bit CKKS rings (two lanes) and the sub-block transforms of N = 2^15 / 2^16; with the special
    prime the baby phase ends in the evaluation domain (k_md_acc), without it in the coefficient tail (k_md_acc_dense); the
    diagonals as lists and as one stacked element; once more a level down, on the same keys"""
    N = 1 << logn
    kp, c, baby, giant, dv = _setup(N, _ring(N, bits), raised, n_baby, n_giant, batch, 2000 + logn)
    R = c[0].ring
    rows = _rows(dv, R, c.scale, n_baby, n_giant)
    want = _composition(baby, giant, rows, c, batch)
    for diags in (rows, tf.ckks_encode(dv, R, c.scale)):
        got = tf.matmul_bsgs(baby, giant, diags, c)
        assert all(x.primal is not None for x in got.cs)                       # coefficient-domain result
        _same_words(got, want, (logn, "stacked" if isinstance(diags, tf.RingElement) else "lists"))
    lo = tf.modswitch(c)
    rows_lo = _rows(dv, lo.ring(), lo.scale, n_baby, n_giant)
    _same_words(tf.matmul_bsgs(baby, giant, rows_lo, lo), _composition(baby, giant, rows_lo, lo, batch), (logn, "lower level"))


@pytest.mark.parametrize("raised", [True, False])
def test_degenerate_forms(raised):
    """no giant step: the inverse transform of matmul_diag; no baby step: plain products, rotated and added; neither: one product"""
    N = 256
    qs = chain(2**40 + 1, 3, N) + ([tf.nextprime(2**50 + 1, 1, 2 * N)] if raised else [])
    kp, c, baby, giant, dv = _setup(N, qs, raised, 3, 2, 2, 31 + raised)
    R = c[0].ring
    enc = lambda v: tf.ckks_encode(v, R, c.scale)
    # n_giant = 0
    row = [enc(dv[i]) for i in range(4)]
    md = tf.matmul_diag(baby, row, c)
    got = tf.matmul_bsgs(baby, [], [row], c)
    assert got.scale == md.scale
    for a, b in zip(got.cs, md.cs):
        assert np.array_equal(a.to_numpy(), b.to_numpy())                      # (to_numpy inverse-transforms matmul_diag's image)
    # n_baby = 0
    rows = [[enc(dv[j])] for j in range(3)]
    _same_words(tf.matmul_bsgs([], giant, rows, c), _composition([], giant, rows, c, 2), "n_baby = 0")
    # both zero
    _same_words(tf.matmul_bsgs([], [], [[row[0]]], c), _composition([], [], [[row[0]]], c, 2), "no keys")
    with pytest.raises(AssertionError):
        tf.matmul_bsgs(baby, giant, [row], c)                                  # one row of diagonals per giant step plus one
    with pytest.raises(tf.UsageError):
        tf.matmul_bsgs(baby, giant, enc(dv[:5]), c)                            # a stacked element of the wrong count


@pytest.mark.parametrize("raised", [True, False])
def test_lazy_reduction_seam(raised):
    """N = 2^6, a 60-bit and a 61-bit limb (4 and 2 products between two reductions), six terms per inner sum"""
    N = 64
    qs = _ring(N, [59, 60] + ([59] if raised else []))          # the next primes above 2^59 and 2^60: 60 and 61 bits
    assert (qs[0].bit_length(), qs[1].bit_length()) == (60, 61)
    for batch in (None, 3):
        kp, c, baby, giant, dv = _setup(N, qs, raised, 5, 1, batch, 77)
        rows = _rows(dv, c[0].ring, c.scale, 5, 1)
        _same_words(tf.matmul_bsgs(baby, giant, rows, c), _composition(baby, giant, rows, c, batch), (raised, batch))


@pytest.mark.parametrize("raised", [True, False])
def test_chunk_seam(raised):
    """N = 2^10, batch 5 under a chunk cap of 2 (chunks 2, 2, 1; the nested key switch chunks under the same cap): the words of the
    uncapped call"""
    N = 1 << 10
    qs = chain(2**40 + 1, 3, N) + ([tf.nextprime(2**50 + 1, 1, 2 * N)] if raised else [])
    kp, c, baby, giant, dv = _setup(N, qs, raised, 2, 2, 5, 55)
    stacked = tf.ckks_encode(dv, c[0].ring, c.scale)
    base = tf.matmul_bsgs(baby, giant, stacked, c)
    _same_words(base, _composition(baby, giant, _rows(dv, c[0].ring, c.scale, 2, 2), c, 5))
    ctx = baby[0].key.key[0].mask.ring.ctx
    for cap in (2, 1):
        ctx.set_chunk(cap)
        try:
            got = tf.matmul_bsgs(baby, giant, stacked, c)
        finally:
            ctx.set_chunk(0)
        _same_words(got, base, ("cap", cap))


@pytest.mark.parametrize("seed", range(8))
def test_matmul_bsgs_random_small_shapes(seed):
    """random small rings (N = 2^4 .. 2^9, one to four ciphertext limbs of 30-60 bits, mostly with the special prime, single and
    batched), one to six baby and zero to five giant steps at random rotation steps: whole and ragged output tiles of every size"""
    rs = np.random.default_rng(1900 + seed)
    logn = int(rs.integers(4, 10)); N = 1 << logn
    L = int(rs.integers(1, 5)); raised = bool(rs.integers(0, 4))
    qs, used = [], set()
    for _ in range(L + (1 if raised else 0)):
        q = tf.nextprime(2 ** int(rs.choice([30, 40, 50, 60])) + 1, 1, 2 * N)
        while q in used:
            q = tf.nextprime(q + 2 * N, 1, 2 * N)
        used.add(q); qs.append(q)
    n_baby = int(rs.integers(1, min(7, N // 2 - 1))); n_giant = int(rs.integers(0, min(6, N // 2 - 1)))
    batch = [None, 2, 3][int(rs.integers(0, 3))]
    steps = ([int(k) for k in rs.choice(np.arange(1, N // 2), n_baby, replace=False)],
             [int(k) for k in rs.choice(np.arange(1, N // 2), n_giant, replace=False)])
    kp, c, baby, giant, dv = _setup(N, qs, raised, n_baby, n_giant, batch, 8000 + seed, scale=2**20, steps=steps)
    rows = _rows(dv, c[0].ring, c.scale, n_baby, n_giant)
    _same_words(tf.matmul_bsgs(baby, giant, rows, c), _composition(baby, giant, rows, c, batch), (logn, qs, raised, n_baby, n_giant, batch))


def test_decrypts_to_the_matrix_product():
    """the parameters of test_matmul_by_hoisted_rotations (N = 64, 4 x 40 bits, ModulusRaised, scale 2^40, an 8 x 8 matrix in blocks
    of 4 slots) with n1 = 4: three baby keys, one giant key, the diagonals regrouped by bsgs_diagonals; W @ x to that test's
    atol = 1e-5.  The two maximum errors are printed."""
    N = 64
    R = tf.NegacyclicRing(N, chain(2**40 + 1, 4, N))
    params = tf.ModulusRaised(tf.CKKSParams(R, 0, 3.2))
    rng = np.random.default_rng(13)
    kp = tf.keygen(rng, params)
    scale = 2**40
    n = 8
    x = rng.normal(0, 1, N // 2)
    W = rng.normal(0, 1, (n, n))
    c = tf.encrypt(rng, kp, tf.ckks_encode(x.astype(complex), params.R_cipher(), scale), scale=scale)
    B = N // 2 // n
    dv = np.array([np.repeat(np.array([W[i, (i - k) % n] for i in range(n)]), B) for k in range(n)])
    D, bsteps, gsteps = tf.bsgs_diagonals(dv, 4, block=B)
    assert bsteps == [B, 2 * B, 3 * B] and gsteps == [4 * B] and D.shape == (2, 4, N // 2)
    baby = [tf.keygen_galois(rng, kp.priv, steps=s) for s in bsteps]
    giant = [tf.keygen_galois(rng, kp.priv, steps=s) for s in gsteps]
    want = W @ x.reshape(n, B)
    res = tf.matmul_bsgs(baby, giant, tf.ckks_encode(D.reshape(-1, N // 2).astype(complex), params.R_cipher(), scale), c)
    got = tf.ckks_decode(tf.decrypt(kp, res), res.scale).real.reshape(n, B)
    # the 63-key shape of the same product, for the record
    gks = [tf.keygen_galois(rng, kp.priv, steps=k * B) for k in range(1, n)]
    md = tf.matmul_diag(gks, tf.ckks_encode(dv.astype(complex), params.R_cipher(), scale), c)
    got_md = tf.ckks_decode(tf.decrypt(kp, md), md.scale).real.reshape(n, B)
    print(f"max |error|: matmul_bsgs {np.abs(got - want).max():.3e}, matmul_diag {np.abs(got_md - want).max():.3e}")
    assert np.allclose(got, want, atol=1e-5)


def test_encrypted_mnist_by_baby_and_giant_steps():
    """examples/encrypted_mnist.py --bsgs 8 at the reference's parameters (N = 2^13, the infer.jl ring, the trained model, two
    ciphertext sets): 7 + 7 Galois keys per 64 x 64 product.  The bound is the one the chained loop (63 accumulated rotations) and
    the 63 hoisted keys (one rotation) both meet on this seed (tests/test_gpu_scheme_mirror.py): two chained rotations lie between."""
    import importlib.util
    import os
    spec_ = importlib.util.spec_from_file_location("encrypted_mnist", os.path.join(os.path.dirname(__file__), "..", "examples", "encrypted_mnist.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    err, rng_, agree = mod.run(logn=13, seed=1, verbose=False, model="reference", batches=2, bsgs=8)
    print(f"encrypted MNIST --bsgs 8: max |logit error| {err:.3e}, logit range {rng_:.2f}, argmax agreement {agree}")
    assert rng_ > 1.0 and err < 1e-3 and agree == 1.0, (err, rng_, agree)
