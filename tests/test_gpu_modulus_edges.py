"""The engine at the edges of every modulus size class, against the oracle word for word.

Every arithmetic policy rests on a range bound that binds at one end of its class (tests/helpers.py names the thresholds and
tests/test_modulus_edges_cpu.py reads them back out of the sources).  The other GPU tests take their primes from the
comfortable end, the first NTT-friendly primes above a power of two; these take them where the bound binds -- the largest
prime below a threshold, the smallest above it, and for the high-word fold of k_ks_inner the primes just above 2^64 / 9 and
2^64 / 5, where 2^64 mod q is close to q -- with inputs that maximise growth: all q - 1, alternating 0 / q - 1, (q -+ 1)/2, the
centring edges and one uniform row, batched into one launch."""
import math

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu, spec
from tests import helpers as H

pytestmark = pytest.mark.gpu


def dev(a):
    return tf.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.uint64))


def edge(name, n, N):
    """n distinct NTT-friendly primes at the named edge"""
    if name.startswith("top") and name[3:].isdigit():                 # largest primes below 2^b
        return H.primes_below(1 << int(name[3:]), n, N)
    return {"fps-top": lambda: H.primes_below(H.FPS_QMAX, n, N), "fps-above": lambda: H.primes_above(H.FPS_QMAX, n, N),
            "fp-top": lambda: H.primes_below(H.FP_QMAX, n, N), "u64-bottom": lambda: H.primes_above(H.FP_QMAX, n, N),
            "above52": lambda: H.primes_above(1 << 52, n, N),
            "fold61": lambda: H.primes_above_ratio(9, 61, n, N), "fold62": lambda: H.primes_above_ratio(5, 62, n, N),
            "below26": lambda: H.primes_below(1 << 26, n, N), "below31": lambda: H.primes_below(1 << 31, n, N),
            "p65537": lambda: [65537] * min(n, 1), "p12289": lambda: [12289] * min(n, 1)}[name]()


def edge_rows(qs, N, seed, copies=1):
    """[6 copies][L][N]: all q - 1, alternating 0 / q - 1, all (q - 1)/2, all (q + 1)/2, the centring edges, one uniform row"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(copies):
        for kind in range(6):
            r = np.empty((len(qs), N), dtype=np.uint64)
            for l, q in enumerate(qs):
                r[l] = {0: lambda: np.full(N, q - 1), 1: lambda: np.tile([0, q - 1], N // 2),
                        2: lambda: np.full(N, (q - 1) // 2), 3: lambda: np.full(N, (q + 1) // 2),
                        4: lambda: np.resize(np.array([0, 1, q - 1, q // 2, q // 2 + 1], dtype=np.uint64), N),
                        5: lambda: rng.integers(0, q, size=N, dtype=np.uint64)}[kind]()
            rows.append(r)
    return np.stack(rows)


def run_ntt(ctx, a, inverse=False, idx=None):
    d = dev(a)
    (ctx.inntt if inverse else ctx.nntt)(d.ptr, d.ptr, a.shape[0], a.shape[1], idx)
    return d.to_numpy(a.shape)


# ---------------------------------------------------------------------------------------------------
# transforms: the block / fused / top-stage kernels of each policy (ntt_core.h)
# ---------------------------------------------------------------------------------------------------
NTT_CASES = ([(r, n) for r in ("fp-top", "fps-top", "top62", "u64-bottom") for n in (10, 11, 12, 13, 14, 15, 16)] +
             [(r, n) for r in ("fps-above", "top52", "above52", "fold61", "fold62", "top56", "top57", "top58", "top59", "top60", "top61",
                               "below26", "below31") for n in (10, 13, 14, 16)] +
             [("p65537", n) for n in (10, 12, 14, 15)] + [("p12289", 10), ("p12289", 11), ("fp-top", 17), ("top62", 17)])


@pytest.mark.parametrize("name,logn", NTT_CASES)
def test_transforms_at_the_class_edges(name, logn):
    """nntt / inntt on growth-maximising rows at each edge: fp-top = ArithFp at a = 0.25025 (sweeps planned at 7.9 p), fps-top /
    fps-above = the ArithFpS class limit and the ArithFp kernels just above it, u64-bottom / top62 / the fold primes = the u64
    butterflies (lazy range 4q < 2^64 at the top), small primes = the fp64 kernels far from the limit.  Variants 1-3 (generic
    radix-2, forced u64, one operation per launch) must agree up to 2^14, variant 2 above.  The inverse also runs on
    growth-maximising evaluation-domain rows."""
    N = 1 << logn
    qs = edge(name, 2, N)
    a = edge_rows(qs, N, logn)
    ref, ctx = ref_cpu.RefCtx(N, qs), tf.Context(N, qs)
    want, want_inv = ref.nntt(a), ref.inntt(a)
    for variant in ((0, 1, 2, 3) if logn <= 14 else (0, 2)):
        ctx.set_ntt_variant(variant)
        assert np.array_equal(run_ntt(ctx, a), want), (name, variant)
        assert np.array_equal(run_ntt(ctx, want, inverse=True), a), (name, variant)
        assert np.array_equal(run_ntt(ctx, a, inverse=True), want_inv), (name, variant)


@pytest.mark.parametrize("logn,copies", [(14, 4), (16, 1)])
def test_transforms_on_a_mixed_ring_at_the_policy_boundary(logn, copies):
    """the top fp64 prime, the bottom u64 prime and a 62-bit prime in one ring, with more than TFHE_MIXED_MIN_WORDS words: the
    two-lane split (one pass per policy over its limbs, toyfhe_hip.hip launch_ntt) next to the forced-u64 path"""
    N = 1 << logn
    qs = edge("fp-top", 1, N) + edge("u64-bottom", 1, N) + edge("top62", 1, N)
    a = edge_rows(qs, N, logn, copies)
    assert a.size >= H.MIXED_MIN_WORDS
    ref, ctx = ref_cpu.RefCtx(N, qs), tf.Context(N, qs)
    want, want_inv = ref.nntt(a), ref.inntt(a)
    for variant in (0, 2):
        ctx.set_ntt_variant(variant)
        assert np.array_equal(run_ntt(ctx, a), want), variant
        assert np.array_equal(run_ntt(ctx, want, inverse=True), a), variant
        assert np.array_equal(run_ntt(ctx, a, inverse=True), want_inv), variant


# ---------------------------------------------------------------------------------------------------
# limb-wise operations (kernels.h k_pointwise / k_scalar_mul / k_tensor): the full cross product of an operand edge set
# ---------------------------------------------------------------------------------------------------
def _operand_edges(q, rng):
    return [0, 1, 2, q - 2, q - 1, (q - 1) // 2, (q + 1) // 2, math.isqrt(q), 1 << (q.bit_length() - 1), int(rng.integers(0, q))]


@pytest.mark.parametrize("name", ["fps-top", "fps-above", "fp-top", "u64-bottom", "top52", "above52", "fold61", "fold62", "top56",
                                  "top57", "top58", "top59", "top60", "top61", "top62", "p65537", "p12289", "below26", "below31"])
def test_limbwise_operations_on_the_operand_edge_cross_product(name):
    N = 1024
    qs = edge(name, 2, N)
    L = len(qs)
    rng = np.random.default_rng(len(name))
    a, b, c = (H.rand_residues(rng, qs, (2,), N) for _ in range(3))
    for l, q in enumerate(qs):
        E = _operand_edges(q, rng)
        n = len(E)
        for k in range(n * n):                                         # row 0: every (edge, edge) pair
            a[0, l, k], b[0, l, k], c[0, l, k] = E[k // n], E[k % n], E[(k * 7) % n]
    ref, ctx = ref_cpu.RefCtx(N, qs), tf.Context(N, qs)
    da, db, dc, do = dev(a), dev(b), dev(c), tf.DeviceBuffer(a.size)
    for op in ("add", "sub", "mul"):
        getattr(ctx, op)(da.ptr, db.ptr, do.ptr, 2, L)
        assert np.array_equal(do.to_numpy(a.shape), ref.pointwise(op, a, b)), op
    ctx.neg(da.ptr, do.ptr, 2, L)
    assert np.array_equal(do.to_numpy(a.shape), ref.pointwise("neg", a))
    ctx.mad(dc.ptr, da.ptr, db.ptr, do.ptr, 2, L)
    assert np.array_equal(do.to_numpy(a.shape), ref.pointwise("add", c, ref.pointwise("mul", a, b)))
    for pick in (4, 6, 7, 8, 9):                                       # q - 1, (q + 1)/2, isqrt(q), 2^(bits - 1), random
        s = [_operand_edges(q, np.random.default_rng(pick))[pick] for q in qs]
        ctx.scalar_mul(s, da.ptr, do.ptr, 2, L)
        assert np.array_equal(do.to_numpy(a.shape), ref.scalar_mul(s, a)), pick
    x, y = np.stack([a, c], axis=1), np.stack([b, a], axis=1)           # [2][2][L][N]
    dx, dy, dt = dev(x), dev(y), tf.DeviceBuffer(2 * 3 * L * N)
    ctx.tensor(dx.ptr, dy.ptr, dt.ptr, 2, L)
    got = dt.to_numpy((2, 3, L, N))
    m = lambda u, v: ref.pointwise("mul", u, v)
    assert np.array_equal(got[:, 0], m(x[:, 0], y[:, 0]))
    assert np.array_equal(got[:, 1], ref.pointwise("add", m(x[:, 0], y[:, 1]), m(x[:, 1], y[:, 0])))
    assert np.array_equal(got[:, 2], m(x[:, 1], y[:, 1]))


# ---------------------------------------------------------------------------------------------------
# sums in the Barrett window (k_dot, k_lincomb, k_lincomb_many, k_md_acc, k_md_acc_dense): chunk = 2^(62 - bits) products between two
# reductions (csrc/lazy_sum.h lazy_chunk)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["top56", "top57", "top58", "top59", "top60", "top61", "top62", "fold61", "fold62", "top52",
                                  "fp-top", "u64-bottom"])
def test_sums_with_every_operand_q_minus_1(name):
    """Row 0 of every operand is q - 1 (each product (q - 1)^2, the largest sum of a chunk: chunk (q - 1)^2 just below
    2^(bits + 62) at the largest prime below 2^b), row 1 uniform.  Term counts chunk, chunk + 1, 64, 65 and 130 cross each
    reduction boundary and, for tfhe_dot, the second launch (> 64 terms) at the maximum sum; tfhe_lincomb / _many take at most
    64 terms per call."""
    N = 1024
    qs = edge(name, 2, N)
    L = len(qs)
    chunk = H.sum_chunk(max(q.bit_length() for q in qs))
    nmax = 130
    rng = np.random.default_rng(nmax + len(name))
    qv = np.array(qs, dtype=object)[None, :, None]
    ops = []
    for _ in range(nmax):
        x = H.rand_residues(rng, qs, (2,), N)
        x[0] = (np.array(qs, dtype=np.uint64) - 1)[:, None]
        ops.append(x)
    dops = [dev(x) for x in ops]
    scal = [[q - 1 for q in qs]] * nmax
    scal2 = [[int(rng.integers(0, q)) if k % 2 else q - 1 for q in qs] for k in range(nmax)]
    out, out2 = tf.DeviceBuffer(2 * L * N), tf.DeviceBuffer(2 * L * N)
    ctx = tf.Context(N, qs)
    for terms in sorted({chunk, chunk + 1, 64, 65, nmax}):
        A = [x.astype(object) for x in ops[:terms]]
        ptrs = [d.ptr for d in dops[:terms]]
        ctx.dot(None, ptrs, ptrs[::-1], out.ptr, 2, L)
        want = sum(x * y for x, y in zip(A, A[::-1])) % qv
        assert np.array_equal(out.to_numpy((2, L, N)), want.astype(np.uint64)), ("dot", terms)
        if terms > 64:
            continue
        ctx.lincomb(scal[:terms], ptrs, out.ptr, 2, L)
        want1 = sum(x * np.array(s, dtype=object)[None, :, None] for x, s in zip(A, scal[:terms])) % qv
        assert np.array_equal(out.to_numpy((2, L, N)), want1.astype(np.uint64)), ("lincomb", terms)
        ctx.lincomb_many([scal[:terms], scal2[:terms]], ptrs, [out.ptr, out2.ptr], 2, L)
        want2 = sum(x * np.array(s, dtype=object)[None, :, None] for x, s in zip(A, scal2[:terms])) % qv
        assert np.array_equal(out.to_numpy((2, L, N)), want1.astype(np.uint64)), ("lincomb_many 0", terms)
        assert np.array_equal(out2.to_numpy((2, L, N)), want2.astype(np.uint64)), ("lincomb_many 1", terms)


@pytest.mark.parametrize("raised", [True, False])
@pytest.mark.parametrize("name,n_rot", [("top61", 3), ("top60", 5), ("fold62", 2), ("top62", 2)])
def test_matmul_diag_at_the_top_of_the_bit_lengths(name, n_rot, raised):
    """tfhe_matmul_diag (one sum of k_md_acc with a special prime, of k_md_acc_dense without: n_rot + 1 products, more than the chunk
    of 2^(62 - bits)) against rotate_many and dot_plain, word for word, on a ring of the largest primes below 2^62 (chunk 1: a fold
    before every rotated term) / 2^61 / 2^60 and the fold primes, diagonals of q - 1"""
    N = 1 << 10
    R = tf.NegacyclicRing(N, edge(name, 3, N))
    assert n_rot + 1 > H.sum_chunk(min(q.bit_length() for q in R.moduli))      # every limb folds at least once
    params = tf.CKKSParams(R, 0, 3.2)
    if raised:
        params = tf.ModulusRaised(params)
    rng = tf.DeviceRng(77)
    kp = tf.keygen(rng, params)
    c = tf.encrypt(rng, kp, tf.ckks_encode(np.ones(N // 2, dtype=complex), params.R_cipher(), 2**30), scale=2**30)
    gks = [tf.keygen_galois(rng, kp.priv, steps=k) for k in range(1, n_rot + 1)]
    cr = params.R_cipher()
    diags = [cr.from_residues(np.array([[q - 1] * N for q in cr.moduli], dtype=np.uint64)) for _ in range(n_rot + 1)]
    got = tf.matmul_diag(gks, diags, c)
    want = tf.CipherText.dot_plain([c] + list(tf.rotate_many(gks, c)), diags)
    for a, b in zip(got.cs, want.cs):
        assert np.array_equal(a.to_numpy("dual"), b.to_numpy("dual"))


# ---------------------------------------------------------------------------------------------------
# key switching: k_ks_inner (fold above 52 bits), k_ks_inner_n2 (acc52 up to 52), k_ks_fused (fp64 class at 2^13 / 2^14),
# k_ks_fused_sub (ArithFpS below 2^42, ArithFp above) at 2^15 / 2^16
# ---------------------------------------------------------------------------------------------------
KS_CASES = [("fold62", 10, 11), ("fold61", 10, 11), ("top62", 10, 4), ("above52", 12, 10), ("top52", 12, 10),
            ("fp-top", 14, 4), ("u64-bottom", 14, 4), ("fps-top", 15, 4), ("fps-above", 15, 4), ("fps-top", 16, 3),
            ("fps-above", 16, 3), ("fp-top", 16, 3), ("below31", 13, 4)]


def _ks_ct(qs, level, polys, N, rng):
    """batch 2: ciphertext 0 with its last component at the centring edges 0, 1, q - 1, floor(q/2), floor(q/2) + 1 and
    all q - 1 in its other components, ciphertext 1 uniform"""
    ct = H.rand_residues(rng, qs[:level], (2, polys), N)
    for l in range(level):
        q = qs[l]
        ct[0, polys - 1, l] = np.resize(np.array([0, 1, q - 1, q // 2, q // 2 + 1], dtype=np.uint64), N)
        ct[0, :polys - 1, l] = q - 1
    return ct


@pytest.mark.parametrize("name,logn,Lk", KS_CASES)
@pytest.mark.parametrize("special", [True, False])
def test_keyswitch_and_rotations_at_the_class_edges(name, logn, Lk, special):
    """keys of all q - 1 (every key product (q - 1) x digit), digits at the centring edges; levels 1 to L, more digits than
    DCH = 8 at the fold primes (lazy sums of DCH terms at 61 bits, 3 at 62: z' = hi (2^64 mod q) + lo < 2^(bits + 62)).
    keyswitch at 2 and 3 components, then rotate, rotate_many and rotate with a prepared key at the top level."""
    N = 1 << logn
    qs = edge(name, Lk, N)
    ref, ctx = ref_cpu.RefCtx(N, qs), tf.Context(N, qs)
    rng = np.random.default_rng(logn * 10 + Lk + special)
    evk = np.broadcast_to((np.array(qs, dtype=np.uint64) - 1)[None, None, :, None], (Lk, 2, Lk, N)).copy()
    devk = dev(evk)
    top = Lk - 1 if special else Lk
    levels = sorted({1, 9 if top > 9 else top, top}) if N <= 1 << 14 else [top]
    for level in levels:
        for polys in ((2, 3) if level == top or N <= 1 << 12 else (2,)):
            ct = _ks_ct(qs, level, polys, N, rng)
            dct, dout = dev(ct), tf.DeviceBuffer(2 * 2 * level * N)
            ctx.keyswitch(Lk, level, special, devk.ptr, Lk, dct.ptr, polys, dout.ptr, 2)
            assert np.array_equal(dout.to_numpy((2, 2, level, N)), ref.keyswitch(level, special, evk, ct)), (level, polys)
    level = top
    ct = _ks_ct(qs, level, 2, N, rng)
    dct, dout = dev(ct), tf.DeviceBuffer(2 * 2 * level * N)
    gs = [pow(3, 5, 2 * N), 2 * N - 1]
    want = [ref.keyswitch(level, special, evk, ref.galois(g, ct.reshape(-1, level, N), idx=range(level)).reshape(ct.shape)) for g in gs]
    ctx.rotate(Lk, level, special, devk.ptr, Lk, gs[0], dct.ptr, dout.ptr, 2)
    assert np.array_equal(dout.to_numpy((2, 2, level, N)), want[0])
    many = tf.DeviceBuffer(len(gs) * 2 * 2 * level * N)
    ctx.rotate_many(Lk, level, special, [devk.ptr] * len(gs), Lk, gs, dct.ptr, many.ptr, 2)
    got = many.to_numpy((len(gs), 2, 2, level, N))
    for r in range(len(gs)):
        assert np.array_equal(got[r], want[r]), r
    prep = tf.DeviceBuffer(evk.size)
    ctx.galois_key_prepare(Lk, Lk, gs[1], devk.ptr, prep.ptr)
    ctx.rotate(Lk, level, special, prep.ptr, Lk, gs[1], dct.ptr, dout.ptr, 2, prepared=True)
    assert np.array_equal(dout.to_numpy((2, 2, level, N)), want[1])


@pytest.mark.parametrize("special", [True, False])
def test_keyswitch_on_a_mixed_ring_at_the_policy_boundary(special):
    """the top fp64 prime, the bottom u64 prime and 62-bit primes (fold primes among them) in one key ring: the digit lift, both
    inner-product kernels side by side on disjoint limbs, the inverse transforms one pass per policy (batch past the split)"""
    N, batch = 1 << 12, 48
    qs = edge("fp-top", 1, N) + edge("u64-bottom", 1, N) + edge("fold62", 1, N) + edge("top52", 1, N) + edge("top62", 1, N)
    Lk = len(qs)
    level = Lk - 1 if special else Lk
    ref, ctx = ref_cpu.RefCtx(N, qs), tf.Context(N, qs)
    rng = np.random.default_rng(5 + special)
    evk = np.broadcast_to((np.array(qs, dtype=np.uint64) - 1)[None, None, :, None], (Lk, 2, Lk, N)).copy()
    ct = np.concatenate([_ks_ct(qs, level, 2, N, rng) for _ in range(batch // 2)])
    devk, dct, dout = dev(evk), dev(ct), tf.DeviceBuffer(batch * 2 * level * N)
    want = ref.keyswitch(level, special, evk, ct)
    for variant in (0, 2):
        ctx.set_ntt_variant(variant)
        ctx.keyswitch(Lk, level, special, devk.ptr, Lk, dct.ptr, 2, dout.ptr, batch)
        assert np.array_equal(dout.to_numpy(want.shape), want), variant


@pytest.mark.parametrize("name,N,L,w,special", [("fold62", 32, 2, 32, False), ("top62", 16, 3, 20, False), ("fold61", 32, 3, 16, True),
                                                 ("top62", 16, 2, 31, True)])
def test_keyswitch_window_at_the_top_of_the_u64_class(name, N, L, w, special):
    """base-2^w digits of the exact integer (k_ks_window_digits) against spec.keyswitch, keys of all q - 1, with and without
    the special prime (the key ring one limb longer), x = 0, Q - 1, 1 and Q // 2 among the inputs"""
    qs = edge(name, L + special, N)
    cq = qs[:L]
    keyring, cring = spec.Ring(N, qs), spec.Ring(N, cq)
    nkey = spec.ndigits(keyring.Q if special else cring.Q, 2 ** w)
    evk_c = [([[q - 1] * N for q in qs], [[q - 1] * N for q in qs]) for _ in range(nkey)]
    evk_ntt = np.array([[spec.poly_nntt(m, keyring), spec.poly_nntt(md, keyring)] for m, md in evk_c], dtype=np.uint64)
    ctx = tf.Context(N, qs)
    devk = dev(evk_ntt)
    rng = np.random.default_rng(N + w)
    for polys in (2, 3):
        ct = H.rand_residues(rng, cq, (1, polys), N)
        for k, x in enumerate([0, cring.Q - 1, 1, cring.Q // 2, cring.Q // 2 + 1]):
            ct[0, polys - 1, :, k] = [x % q for q in cq]
        dct, dout = dev(ct), tf.DeviceBuffer(2 * L * N)
        ctx.keyswitch_window(L, w, devk.ptr, nkey, dct.ptr, polys, dout.ptr, 1, key_limbs=len(qs), special=special)
        want = spec.keyswitch(evk_c, [[list(map(int, l)) for l in c] for c in ct[0]], cring, keyring, special, relin_window=w)
        assert np.array_equal(dout.to_numpy((2, L, N)), np.array(want, dtype=np.uint64)), polys


# ---------------------------------------------------------------------------------------------------
# BFV: k_bfv_core_fused and the exact conversions, narrow (acc52 / acc52_redc below TFHE_FP_QMAX, ns + 2, np + 2 <= 16) and wide
# ---------------------------------------------------------------------------------------------------
# The narrow bodies (acc52 / acc52_redc) exist only on the register-resident fast path, which is compiled for (ns, np) = (8, 9),
# (3, 4), (2, 3) and (6, 7) of superset rings (bfv_api.inc TFHE_FAST_PAIRS): at most NS + 2 = 10 and NP + 2 = 11 terms per sum.
# Wider rings (14 / 14 below) and disjoint ones take the general k_bfv_expand / k_bfv_contract kernels.
BFV_CASES = [("fp-top", 12, 14, 14, "superset"),      # general kernels at the fp64 class top, 14 + 14 limbs
             ("u64-bottom", 12, 14, 14, "superset"),  # the same shape just above 2^50 + 2^40
             ("fp-top", 13, 3, 4, "superset"),        # k_bfv_core_fused, narrow fast conversions at the class top
             ("fp-top", 12, 8, 9, "superset"),        # the widest narrow shape at the class top: 10 / 11 terms into acc52_redc
             ("u64-bottom", 12, 8, 9, "superset"),    # the same shape just above 2^50 + 2^40: the wide fast conversions
             ("fp-top", 12, 8, 9, "disjoint"),        # general kernels
             ("top62", 11, 3, 4, "superset"),         # every modulus 62 bits: lazy = 1
             ("top62", 10, 2, 3, "disjoint"),
             ("below31", 12, 8, 9, "superset"),       # narrow fast conversions, primes below 2^31 (acc52_redc: r < (1 + 2^-23) p)
             ("below31", 11, 3, 4, "disjoint")]


@pytest.mark.parametrize("name,logn,ns,np_,mode", BFV_CASES)
def test_bfv_at_the_class_edges(name, logn, ns, np_, mode):
    """expand / contract on the edge values of test_bfv_expand_contract_mul plus rows of q - 1, mul on a ragged chunk and
    mul_relin with a key of all q - 1, all against the oracle"""
    N, t = 1 << logn, 65537
    ch = edge(name, ns + np_, N)
    qs = ch[:ns]
    pb = ch if mode == "superset" else ch[ns:]                        # np_ limbs of P either way
    rs, rb = ref_cpu.RefCtx(N, qs), ref_cpu.RefCtx(N, pb)
    small, big = spec.Ring(N, qs), spec.Ring(N, pb)
    if mode == "superset":
        cbig = tf.Context(N, pb); csmall = cbig
        plan = tf.BfvPlan(csmall, cbig, t, idx_s=list(range(ns)))
    else:
        csmall, cbig = tf.Context(N, qs), tf.Context(N, pb)
        plan = tf.BfvPlan(csmall, cbig, t)
    rng = np.random.default_rng(logn * 100 + ns)
    a = H.rand_residues(rng, qs, (3,), N)
    for k, x in enumerate([0, 1, small.Q - 1, small.Q // 2, small.Q // 2 + 1]):
        a[0, :, k] = [x % q for q in qs]
    a[1] = (np.array(qs, dtype=np.uint64) - 1)[:, None]
    da, de = dev(a), tf.DeviceBuffer(3 * len(pb) * N)
    plan.expand(da.ptr, de.ptr, 3)
    assert np.array_equal(de.to_numpy((3, len(pb), N)), ref_cpu.switch(rs, rb, a))
    y = H.rand_residues(rng, pb, (3,), N)
    tinv = pow(t, -1, big.Q)
    edges = [0, 1, big.Q - 1, big.Q // 2, big.Q // 2 + 1, small.Q // 2, small.Q // 2 + 1, small.Q,
             5 * small.Q + small.Q // 2, 5 * small.Q + small.Q // 2 + 1, big.Q - small.Q // 2 - 1]
    for k, x in enumerate(edges):
        y[0, :, k] = [(x * tinv) % big.Q % p for p in pb]
    y[1] = (np.array(pb, dtype=np.uint64) - 1)[:, None]
    dy, dc = dev(y), tf.DeviceBuffer(3 * ns * N)
    plan.contract(dy.ptr, dc.ptr, 3)
    assert np.array_equal(dc.to_numpy((3, ns, N)), ref_cpu.contract(rb, rs, t, y))
    batch = 3
    plan.set_chunk(2)
    c1, c2 = H.rand_residues(rng, qs, (batch, 2), N), H.rand_residues(rng, qs, (batch, 2), N)
    c1[0] = (np.array(qs, dtype=np.uint64) - 1)[None, :, None]
    c2[0] = (np.array(qs, dtype=np.uint64) - 1)[None, :, None]
    d1, d2, do = dev(c1), dev(c2), tf.DeviceBuffer(batch * 3 * ns * N)
    plan.mul(d1.ptr, d2.ptr, do.ptr, batch)
    prod = ref_cpu.bfv_mul(rs, rb, t, c1, c2)
    assert np.array_equal(do.to_numpy((batch, 3, ns, N)), prod)
    evk = np.broadcast_to((np.array(qs, dtype=np.uint64) - 1)[None, None, :, None], (ns, 2, ns, N)).copy()
    devk, do2 = dev(evk), tf.DeviceBuffer(batch * 2 * ns * N)
    plan.mul_relin(devk.ptr, ns, d1.ptr, d2.ptr, do2.ptr, batch)
    assert np.array_equal(do2.to_numpy((batch, 2, ns, N)), rs.keyswitch(ns, False, evk, prod))


# ---------------------------------------------------------------------------------------------------
# plaintext codec and noise maximum on one 62-bit limb (plain_core.h)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tkind", ["2", "2^61", "prime"])
def test_plain_codec_on_a_62_bit_limb(tkind):
    N = 1 << 12
    q = edge("top62", 1, N)[0]
    t = {"2": 2, "2^61": 1 << 61, "prime": q - 2}[tkind]
    while tkind == "prime" and not spec.is_prime(t):                  # the largest prime below min(Q, 2^62) = q
        t -= 1
    assert t == {"2": 2, "2^61": 1 << 61}.get(tkind, t)
    ctx = tf.Context(N, [q])
    plan = tf.PlainPlan(ctx, t)
    rng = np.random.default_rng(len(tkind))
    delta = q // t
    res = H.rand_residues(rng, [q], (3,), N)
    e = [0, 1, 2, q - 1, q - 2, q // 2, q // 2 + 1, delta, delta - 1, delta + 1, delta // 2, delta // 2 + 1, q - delta, q - delta // 2]
    res[0, 0, :len(e)] = e
    res[1, 0] = q - 1
    src = dev(res)
    out = tf.DeviceBuffer(3 * N)
    ring = spec.Ring(N, [q], [1])
    for scheme, dec in ((tf.native.PLAIN_BFV, spec.bfv_decode), (tf.native.PLAIN_BGV, spec.bgv_decode)):
        plan.decode(scheme, src.ptr, out.ptr, 3)
        got = out.to_numpy((3, N))
        for b in range(3):
            assert got[b].tolist() == dec([[int(v) for v in res[b, 0]]], ring, t), (scheme, b)
    m = rng.integers(0, t, size=(2, N), dtype=np.uint64)
    m[0, :6] = [0, 1, t - 1, t // 2, (t // 2 + 1) % t, (t // 2 - 1) % t]
    dm, enc = dev(m), tf.DeviceBuffer(2 * N)
    plan.encode(tf.native.PLAIN_BFV, dm.ptr, enc.ptr, 2)
    got = enc.to_numpy((2, 1, N))
    for b in range(2):
        assert got[b].tolist() == spec.bfv_encode([int(x) for x in m[b]], ring, t), b
    plan.encode(tf.native.PLAIN_BGV, dm.ptr, enc.ptr, 2)
    assert np.array_equal(enc.to_numpy((2, 1, N))[:, 0], m % np.uint64(q))
    words = tf.DeviceBuffer(3 * plan.delta_words)
    plan.noise_max(src.ptr, words.ptr, 3)
    got = words.to_numpy((3, plan.delta_words))
    for b in range(3):
        worst = max((delta - x % delta) if x % delta > delta // 2 else x % delta for x in (int(v) for v in res[b, 0]))
        assert sum(int(w) << (64 * i) for i, w in enumerate(got[b])) == worst, b
