"""tfhe_matmul_bsgs_blocks (she.matmul_bsgs_blocks): the block-row matrix product by baby and giant steps -- several ciphertext inputs,
each with its own diagonals, one set of giant rotations -- in one device call, against the composition of public calls it replaces:
rotate_many over the baby keys per input, ONE dot_plain per giant step over the concatenated term lists, rotate per giant step, +,
the bias added to component 0 -- word for word: every step is exact arithmetic on canonical residues."""
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


def _setup(N, qs, raised, n_baby, n_giant, n_in, batch, seed, scale=2**30, steps=None):
    """keys, n_in ciphertexts of one ring, scale and batch, one set of slot vectors [n_in][(n_giant + 1)(n_baby + 1)][N / 2] and a bias
    slot vector"""
    params = tf.CKKSParams(tf.NegacyclicRing(N, qs), 0, 3.2)
    if raised:
        params = tf.ModulusRaised(params)
    rng = tf.DeviceRng(seed)
    kp = tf.keygen(rng, params)
    nrng = np.random.default_rng(seed)
    shape = (N // 2,) if batch is None else (batch, N // 2)
    cs = [tf.encrypt(rng, kp, tf.ckks_encode(nrng.normal(0, 1, shape).astype(complex), params.R_cipher(), scale), scale=scale)
          for _ in range(n_in)]
    if steps is None:
        steps = list(range(1, n_baby + 1)), [j * (n_baby + 1) for j in range(1, n_giant + 1)]
    baby = tf.keygen_galois_many(rng, kp.priv, steps=steps[0])
    giant = tf.keygen_galois_many(rng, kp.priv, steps=steps[1])
    dv = nrng.normal(0, 1, (n_in, (n_giant + 1) * (n_baby + 1), N // 2)).astype(complex)
    bv = nrng.normal(0, 1, N // 2).astype(complex)
    return kp, cs, baby, giant, dv, bv


def _rows(dv, ring, scale, n_baby, n_giant):
    """per input: [n_giant + 1][n_baby + 1] single plaintext elements"""
    return [[[tf.ckks_encode(d[j * (n_baby + 1) + i], ring, scale) for i in range(n_baby + 1)] for j in range(n_giant + 1)] for d in dv]


def _stacked(dv, ring, scale):
    return [tf.ckks_encode(d, ring, scale) for d in dv]


def _bias(bv, c):
    """a plaintext element at the result's scale"""
    return tf.ckks_encode(bv, c[0].ring, c.scale ** 2)


def _add_bias(res, bias, batch):
    """the bias onto component 0 (tfhe_add, limb-wise)"""
    if bias is None:
        return res
    b = bias if batch is None else bias.broadcast_to(batch)
    return tf.CipherText(res.params, (res.cs[0] + b,) + tuple(res.cs[1:]), res.scale)


def _composition(baby, giant, rows, cs, batch, bias=None):
    """rotate_many per input -> (nntt) ONE dot_plain per giant step over all n_in (n_baby + 1) terms -> (inntt) rotate per giant step
    j >= 1 -> + -> + bias on component 0"""
    rots = [r for c in cs for r in [c] + list(tf.rotate_many(baby, c))]
    bc = lambda d: d if batch is None else d.broadcast_to(batch)
    inner = [tf.CipherText.dot_plain(rots, [bc(d) for rm in rows for d in rm[j]]) for j in range(len(giant) + 1)]
    res = inner[0]
    for gk, x in zip(giant, inner[1:]):
        res = res + tf.rotate(gk, x)
    if not giant:                                        # (dot_plain leaves its sum in the NTT domain; the call's result is coefficients)
        for x in res.cs:
            x.coeffs_primal()
    return _add_bias(res, bias, batch)


def _same_words(got, want, what=None):
    assert got.scale == want.scale and len(got) == 2
    for a, b in zip(got.cs, want.cs):
        assert np.array_equal(a.to_numpy(), b.to_numpy()), what


CASES = [(6, [40, 40, 40, 40], 3, 2, 3, None, True), (12, [60, 40, 40, 60], 2, 2, 2, 3, True), (14, [50, 50, 50, 50], 2, 1, 2, 2, True),
         (15, [40, 40, 40, 40], 1, 2, 2, 2, True), (16, [60, 40, 40, 40, 60], 1, 1, 2, 2, True),
         (12, [60, 40, 40], 2, 2, 3, 3, False)]


@pytest.mark.parametrize("logn,bits,n_baby,n_giant,n_in,batch,raised", CASES)
def test_blocks_is_word_for_word_the_composition(logn, bits, n_baby, n_giant, n_in, batch, raised):
    """uniform rings, the mixed 60/40-bit CKKS rings (two lanes) and the sub-block transforms of N = 2^15 / 2^16; with the special
    prime the baby phase ends in the evaluation domain (k_md_acc, seeded from input 1 on), without it in the coefficient tail
    (k_md_acc_dense); the diagonals as lists and stacked; with a bias; once more a level down, on the same keys"""
    N = 1 << logn
    kp, cs, baby, giant, dv, bv = _setup(N, _ring(N, bits), raised, n_baby, n_giant, n_in, batch, 2100 + logn)
    R = cs[0][0].ring
    rows = _rows(dv, R, cs[0].scale, n_baby, n_giant)
    bias = _bias(bv, cs[0])
    want = _composition(baby, giant, rows, cs, batch, bias)
    for diags in (rows, _stacked(dv, R, cs[0].scale)):
        got = tf.matmul_bsgs_blocks(baby, giant, diags, cs, bias)
        assert all(x.primal is not None for x in got.cs)                       # coefficient-domain result
        _same_words(got, want, (logn, "stacked" if isinstance(diags[0], tf.RingElement) else "lists"))
    lo = [tf.modswitch(c) for c in cs]
    rows_lo = _rows(dv, lo[0].ring(), lo[0].scale, n_baby, n_giant)
    bias_lo = tf.ckks_encode(bv, lo[0].ring(), lo[0].scale ** 2)
    _same_words(tf.matmul_bsgs_blocks(baby, giant, rows_lo, lo, bias_lo), _composition(baby, giant, rows_lo, lo, batch, bias_lo), (logn, "lower level"))


@pytest.mark.parametrize("raised", [True, False])
def test_one_input_bias_and_repeated_input(raised):
    """n_in = 1 without a bias: the words of tf.matmul_bsgs; with a bias the words differ by exactly the bias on component 0; the
    same ciphertext given twice equals the composition"""
    N = 256
    qs = chain(2**40 + 1, 3, N) + ([tf.nextprime(2**50 + 1, 1, 2 * N)] if raised else [])
    kp, cs, baby, giant, dv, bv = _setup(N, qs, raised, 3, 2, 2, 2, 41 + raised)
    R = cs[0][0].ring
    rows = _rows(dv, R, cs[0].scale, 3, 2)
    one = tf.matmul_bsgs_blocks(baby, giant, rows[:1], cs[:1])
    _same_words(one, tf.matmul_bsgs(baby, giant, rows[0], cs[0]), "n_in = 1")
    bias = _bias(bv, cs[0])
    with_bias = tf.matmul_bsgs_blocks(baby, giant, rows[:1], cs[:1], bias)
    _same_words(with_bias, _add_bias(one, bias, 2), "bias")
    assert np.array_equal(with_bias.cs[1].to_numpy(), one.cs[1].to_numpy())
    q = np.array(R.moduli, dtype=object).reshape(1, -1, 1)
    diff = (with_bias.cs[0].to_numpy().astype(object) - one.cs[0].to_numpy().astype(object)) % q
    assert np.array_equal(diff, np.broadcast_to(bias.to_numpy().astype(object).reshape(1, len(R.moduli), N), diff.shape))
    twice = [cs[0], cs[0]]
    _same_words(tf.matmul_bsgs_blocks(baby, giant, rows, twice), _composition(baby, giant, rows, twice, 2), "the same input twice")


@pytest.mark.parametrize("raised", [True, False])
def test_degenerate_forms(raised):
    """n_in = 2 with no giant step (the sum of two matmul_diag, inverse-transformed), no baby step (plain products, rotated and added),
    neither (two products)"""
    N = 256
    qs = chain(2**40 + 1, 3, N) + ([tf.nextprime(2**50 + 1, 1, 2 * N)] if raised else [])
    kp, cs, baby, giant, dv, bv = _setup(N, qs, raised, 3, 2, 2, 2, 31 + raised)
    R = cs[0][0].ring
    enc = lambda v: tf.ckks_encode(v, R, cs[0].scale)
    bias = _bias(bv, cs[0])
    # n_giant = 0
    rows = [[[enc(d[i]) for i in range(4)]] for d in dv]
    _same_words(tf.matmul_bsgs_blocks(baby, [], rows, cs, bias), _composition(baby, [], rows, cs, 2, bias), "n_giant = 0")
    # n_baby = 0
    rows = [[[enc(d[j])] for j in range(3)] for d in dv]
    _same_words(tf.matmul_bsgs_blocks([], giant, rows, cs), _composition([], giant, rows, cs, 2), "n_baby = 0")
    # both zero
    rows = [[[enc(d[0])]] for d in dv]
    _same_words(tf.matmul_bsgs_blocks([], [], rows, cs, bias), _composition([], [], rows, cs, 2, bias), "no keys")
    with pytest.raises(tf.UsageError):
        tf.matmul_bsgs_blocks([], [], rows, cs[:1])                            # one set of diagonals per input
    with pytest.raises(tf.UsageError):
        tf.matmul_bsgs_blocks([], [], rows, [cs[0], tf.modswitch(cs[1])])      # one ring and level
    with pytest.raises(tf.UsageError):
        tf.matmul_bsgs_blocks([], [], rows, cs, tf.modswitch(cs[0])[0])        # the bias is an element of the ciphertexts' ring


@pytest.mark.parametrize("raised", [True, False])
def test_lazy_reduction_seam(raised):
    """N = 2^6, a 60-bit and a 61-bit limb (4 and 2 products between two reductions), 5 baby steps and three inputs: 18 terms per
    inner sum across two seeds"""
    N = 64
    qs = _ring(N, [59, 60] + ([59] if raised else []))          # the next primes above 2^59 and 2^60: 60 and 61 bits
    assert (qs[0].bit_length(), qs[1].bit_length()) == (60, 61)
    for batch in (None, 3):
        kp, cs, baby, giant, dv, bv = _setup(N, qs, raised, 5, 1, 3, batch, 77)
        rows = _rows(dv, cs[0][0].ring, cs[0].scale, 5, 1)
        _same_words(tf.matmul_bsgs_blocks(baby, giant, rows, cs), _composition(baby, giant, rows, cs, batch), (raised, batch))


@pytest.mark.parametrize("raised", [True, False])
def test_chunk_seam(raised):
    """N = 2^10, batch 5, two inputs under chunk caps of 2 and 1 (chunks 2, 2, 1 / five of 1): the words of the uncapped call.  Input 0
    of every chunk after the first finds the previous chunk's sums in the accumulator and must not add to them"""
    N = 1 << 10
    qs = chain(2**40 + 1, 3, N) + ([tf.nextprime(2**50 + 1, 1, 2 * N)] if raised else [])
    kp, cs, baby, giant, dv, bv = _setup(N, qs, raised, 2, 2, 2, 5, 55)
    R = cs[0][0].ring
    stacked = _stacked(dv, R, cs[0].scale)
    bias = _bias(bv, cs[0])
    base = tf.matmul_bsgs_blocks(baby, giant, stacked, cs, bias)
    _same_words(base, _composition(baby, giant, _rows(dv, R, cs[0].scale, 2, 2), cs, 5, bias))
    ctx = baby[0].key.key[0].mask.ring.ctx
    for cap in (2, 1):
        ctx.set_chunk(cap)
        try:
            got = tf.matmul_bsgs_blocks(baby, giant, stacked, cs, bias)
        finally:
            ctx.set_chunk(0)
        _same_words(got, base, ("cap", cap))


@pytest.mark.parametrize("seed", range(8))
def test_blocks_random_small_shapes(seed):
    """random small rings (N = 2^4 .. 2^9, one to four ciphertext limbs of 30-60 bits, mostly with the special prime, single and
    batched), one to six baby and zero to five giant steps at random rotation steps, one to four inputs, with or without a bias:
    whole and ragged output tiles of every size in both forms"""
    rs = np.random.default_rng(2900 + seed)
    logn = int(rs.integers(4, 10)); N = 1 << logn
    L = int(rs.integers(1, 5)); raised = bool(rs.integers(0, 4))
    qs, used = [], set()
    for _ in range(L + (1 if raised else 0)):
        q = tf.nextprime(2 ** int(rs.choice([30, 40, 50, 60])) + 1, 1, 2 * N)
        while q in used:
            q = tf.nextprime(q + 2 * N, 1, 2 * N)
        used.add(q); qs.append(q)
    n_baby = int(rs.integers(1, min(7, N // 2 - 1))); n_giant = int(rs.integers(0, min(6, N // 2 - 1)))
    n_in = int(rs.integers(1, 5)); has_bias = bool(rs.integers(0, 2))
    batch = [None, 2, 3][int(rs.integers(0, 3))]
    steps = ([int(k) for k in rs.choice(np.arange(1, N // 2), n_baby, replace=False)],
             [int(k) for k in rs.choice(np.arange(1, N // 2), n_giant, replace=False)])
    kp, cs, baby, giant, dv, bv = _setup(N, qs, raised, n_baby, n_giant, n_in, batch, 9000 + seed, scale=2**20, steps=steps)
    rows = _rows(dv, cs[0][0].ring, cs[0].scale, n_baby, n_giant)
    bias = _bias(bv, cs[0]) if has_bias else None
    _same_words(tf.matmul_bsgs_blocks(baby, giant, rows, cs, bias), _composition(baby, giant, rows, cs, batch, bias),
                (logn, qs, raised, n_baby, n_giant, n_in, has_bias, batch))


def test_decrypts_to_the_block_row_product():
    """the parameters of test_decrypts_to_the_matrix_product (N = 64, 4 x 40 bits, ModulusRaised, scale 2^40, blocks of 4 slots, n1 = 4)
    with an 8 x 16 matrix over two ciphertexts and a bias: W[:, :8] @ x0 + W[:, 8:] @ x1 + b to that test's atol = 1e-5.  The two
    maximum errors (the one call; two matmul_bsgs calls, + and the bias) are printed."""
    N = 64
    R = tf.NegacyclicRing(N, chain(2**40 + 1, 4, N))
    params = tf.ModulusRaised(tf.CKKSParams(R, 0, 3.2))
    rng = np.random.default_rng(13)
    kp = tf.keygen(rng, params)
    scale = 2**40
    n = 8
    B = N // 2 // n
    xs = [rng.normal(0, 1, N // 2) for _ in range(2)]
    W = rng.normal(0, 1, (n, 2 * n))
    b = rng.normal(0, 1, n)
    cs = [tf.encrypt(rng, kp, tf.ckks_encode(x.astype(complex), params.R_cipher(), scale), scale=scale) for x in xs]
    Ds = []
    for m in range(2):
        Wm = W[:, m * n:(m + 1) * n]
        dv = np.array([np.repeat(np.array([Wm[i, (i - k) % n] for i in range(n)]), B) for k in range(n)])
        D, bsteps, gsteps = tf.bsgs_diagonals(dv, 4, block=B)
        Ds.append(tf.ckks_encode(D.reshape(-1, N // 2).astype(complex), params.R_cipher(), scale))
    assert bsteps == [B, 2 * B, 3 * B] and gsteps == [4 * B]
    baby = [tf.keygen_galois(rng, kp.priv, steps=s) for s in bsteps]
    giant = [tf.keygen_galois(rng, kp.priv, steps=s) for s in gsteps]
    bias = tf.ckks_encode(np.repeat(b, B).astype(complex), params.R_cipher(), scale ** 2)
    want = W[:, :n] @ xs[0].reshape(n, B) + W[:, n:] @ xs[1].reshape(n, B) + b[:, None]
    res = tf.matmul_bsgs_blocks(baby, giant, Ds, cs, bias)
    got = tf.ckks_decode(tf.decrypt(kp, res), res.scale).real.reshape(n, B)
    # the call-by-call shape of the same layer, for the record
    parts = tf.matmul_bsgs(baby, giant, Ds[0], cs[0]) + tf.matmul_bsgs(baby, giant, Ds[1], cs[1])
    parts = _add_bias(parts, bias, None)
    got_parts = tf.ckks_decode(tf.decrypt(kp, parts), parts.scale).real.reshape(n, B)
    print(f"max |error|: matmul_bsgs_blocks {np.abs(got - want).max():.3e}, two matmul_bsgs + bias {np.abs(got_parts - want).max():.3e}")
    assert np.allclose(got, want, atol=1e-5)


def test_encrypted_mnist_with_the_first_dense_layer_in_one_call():
    """examples/encrypted_mnist.py --bsgs 8 --blocks at the reference's parameters (N = 2^13, the infer.jl ring, the trained model, two
    ciphertext sets): the first dense layer (64 x 256 over the four squares, + bias) as one tfhe_matmul_bsgs_blocks call.  The bounds
    are those of test_encrypted_mnist_by_baby_and_giant_steps."""
    import importlib.util
    import os
    spec_ = importlib.util.spec_from_file_location("encrypted_mnist", os.path.join(os.path.dirname(__file__), "..", "examples", "encrypted_mnist.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    err, rng_, agree = mod.run(logn=13, seed=1, verbose=False, model="reference", batches=2, bsgs=8, blocks=True)
    err0, _, _ = mod.run(logn=13, seed=1, verbose=False, model="reference", batches=2, bsgs=8)
    print(f"encrypted MNIST --bsgs 8 --blocks: max |logit error| {err:.3e} (--bsgs 8 alone: {err0:.3e}), logit range {rng_:.2f}, "
          f"argmax agreement {agree}")
    assert rng_ > 1.0 and err < 1e-3 and agree == 1.0, (err, rng_, agree)
