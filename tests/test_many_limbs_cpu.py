"""17 to 40 limbs without a GPU.  tests/test_gpu_many_limbs.py compares the device against oracle/ref_cpu.c on rings of up
to TFHE_MAX_LIMBS = 40 limbs, so the C oracle is pinned first, at those widths, to the Python big-integer spec (its tables
are sized [64]; nothing had run it past 17 limbs).  Then the kernel-body harness tests/emul, wherever it takes a limb count
(the exact base conversion behind bfv_expand / bfv_contract / keyswitch_window), at 33, 34 and 40 limbs.

spec.keyswitch costs O(limbs^2) pure-Python transforms, so it runs at N = 32; at N = 1024 the oracle's
key switch is checked against the same formula assembled from the primitives (transform, product, modswitch) that this
module pins to the spec at N = 1024 on the same ring."""
import random

import numpy as np
import pytest

from oracle import ref_cpu, spec
from tests import helpers as H
from tests import many_limbs as ML
from tests.emul import emul


def _L(a):
    return [[int(x) for x in limb] for limb in a]


def _edges(a, qs):
    """0, 1, q - 1, q / 2, q / 2 + 1 on every limb of the first element"""
    for l, q in enumerate(qs):
        a[0, l, :5] = [0, 1, q - 1, q // 2, q // 2 + 1]
    return a


@pytest.mark.parametrize("N", [32, 1024])
@pytest.mark.parametrize("name", ["U40", "W40", "M34"])
def test_oracle_ring_ops_match_spec(name, N):
    qs = ML.ring(name, N)
    ring, ctx = spec.Ring(N, qs), ref_cpu.RefCtx(N, qs)
    assert ctx.psis == ring.psis
    rng = np.random.default_rng(N + len(qs))
    a, b = _edges(H.rand_residues(rng, qs, (2,), N), qs), H.rand_residues(rng, qs, (2,), N)
    fw = ctx.nntt(a)
    assert _L(fw[0]) == spec.poly_nntt(_L(a[0]), ring)
    assert np.array_equal(ctx.inntt(fw), a)
    assert _L(ctx.inntt(b)[1]) == spec.poly_inntt(_L(b[1]), ring)
    assert _L(ctx.pointwise("mul", a, b)[0]) == spec.poly_pointwise(_L(a[0]), _L(b[0]), ring)
    for g in (3, 2 * N - 1, pow(3, N // 2 - 1, 2 * N)):
        assert _L(ctx.galois(g, a)[0]) == spec.poly_galois(_L(a[0]), g, ring), g
    assert _L(ctx.modswitch(a)[0]) == spec.modswitch_poly(_L(a[0]), ring)
    # a 33-limb selection in another order, rescaled by its own last limb
    idx = ML.shuffled(len(qs), 33, N)
    sub_ring = ring.select(idx)
    sub = np.ascontiguousarray(a[:, idx])
    assert _L(ctx.nntt(sub, idx)[0]) == spec.poly_nntt(_L(sub[0]), sub_ring)
    assert _L(ctx.modswitch(sub, idx)[0]) == spec.modswitch_poly(_L(sub[0]), sub_ring)
    assert _L(ctx.galois(5, sub, idx)[1]) == spec.poly_galois(_L(sub[1]), 5, sub_ring)


KS_CASES = [("M34", 33, True, 2), ("M34", 33, True, 3), ("U40", 39, True, 3), ("W40", 40, False, 2), ("U40", 40, False, 3)]


@pytest.mark.parametrize("name,level,special,polys", KS_CASES)
def test_oracle_keyswitch_matches_spec(name, level, special, polys):
    """level 33 + special prime (34 working limbs), level 39 + special (the last idx slot) and level 40 plain, 2 and 3
    components, uniform key components (the arithmetic does not care whether the key decrypts)"""
    N = 32
    qs = ML.ring(name, N)
    keyring, kctx = spec.Ring(N, qs), ref_cpu.RefCtx(N, qs)
    cring = keyring.select(range(level))
    rng = np.random.default_rng(level * 4 + polys)
    evk = H.rand_residues(rng, qs, (level, 2), N)                          # coefficient domain
    evk_ntt = kctx.nntt(evk.reshape(-1, len(qs), N)).reshape(evk.shape)
    ct = H.rand_residues(rng, qs[:level], (2, polys), N)
    _edges(ct[:, polys - 1], qs[:level])
    out = kctx.keyswitch(level, special, evk_ntt, ct)
    pairs = [(_L(p[0]), _L(p[1])) for p in evk]
    for b in range(2):
        want = spec.keyswitch(pairs, [_L(p) for p in ct[b]], cring, keyring, special=special)
        assert [_L(p) for p in out[b]] == want, b


def _keyswitch_from_primitives(ref, qs, level, special, evk_ntt, ct):
    """rlwe_she.jl:315-347 / modulusraising.jl:35-49 on one ciphertext, from ref.nntt / pointwise / inntt / modswitch"""
    N, Lk = ref.N, len(qs)
    which = list(range(level)) + ([Lk - 1] if special else [])
    wq = [qs[j] for j in which]
    polys = ct.shape[0]
    S = np.zeros((2, len(which), N), dtype=np.uint64)
    for i in range(level):
        c = ct[-1, i].astype(object)
        c = np.where(c > qs[i] // 2, c - qs[i], c)                          # SignedMod, signedmod.jl:12-19
        dig = np.array([[int(x) % q for x in c] for q in wq], dtype=np.uint64)[None]
        dig = ref.nntt(dig, which)
        for s in (0, 1):
            S[s] = ref.pointwise("add", S[s][None], ref.pointwise("mul", evk_ntt[i, s][which][None], dig, which), which)[0]
    S = ref.inntt(S, which)
    out = np.empty((2, level, N), dtype=np.uint64)
    for s, comp in ((1, 0), (0, 1)):                                        # masked -> c1, mask -> c2
        add = ct[comp] if comp < polys - 1 else np.zeros((level, N), dtype=np.uint64)
        if special:
            P = qs[-1]
            up = np.zeros((len(which), N), dtype=np.uint64)
            up[:level] = ref.scalar_mul([P % q for q in qs[:level]], add[None], range(level))[0]
            out[comp] = ref.modswitch(ref.pointwise("add", up[None], S[s][None], which), which)[0]
        else:
            out[comp] = ref.pointwise("add", add[None], S[s][None], which)[0]
    return out


@pytest.mark.parametrize("name,level,special,polys", [("M34", 33, True, 2), ("W40", 40, False, 3)])
def test_oracle_keyswitch_at_1024_matches_its_pinned_primitives(name, level, special, polys):
    N = 1024
    qs = ML.ring(name, N)
    ref = ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(level + polys)
    evk = H.uniform_evk(rng, qs, level, N)
    ct = H.rand_residues(rng, qs[:level], (1, polys), N)
    _edges(ct[:, polys - 1], qs[:level])
    want = _keyswitch_from_primitives(ref, qs, level, special, evk, ct[0])
    assert np.array_equal(ref.keyswitch(level, special, evk, ct)[0], want)


@pytest.mark.parametrize("mode", ["superset", "disjoint"])
def test_oracle_bfv_at_13_of_27_limbs_matches_spec(mode):
    N, t, ns, nb = 32, 65537, 13, 27
    ch = H.chain(50, ns + nb, N)
    qs = ch[:ns]
    pb = ch[:nb] if mode == "superset" else ch[ns:]
    small, big = spec.Ring(N, qs), spec.Ring(N, pb)
    cs, cb = ref_cpu.RefCtx(N, qs), ref_cpu.RefCtx(N, pb)
    rng = np.random.default_rng(ns)
    a = H.rand_residues(rng, qs, (2,), N)
    for k, x in enumerate([0, 1, small.Q - 1, small.Q // 2, small.Q // 2 + 1]):
        a[0, :, k] = [x % q for q in qs]
    assert _L(ref_cpu.switch(cs, cb, a)[0]) == spec.switch_poly(_L(a[0]), small, big)
    y = H.rand_residues(rng, pb, (2,), N)
    tinv = pow(t, -1, big.Q)
    for k, x in enumerate([0, 1, big.Q - 1, big.Q // 2, big.Q // 2 + 1, small.Q // 2, small.Q // 2 + 1, small.Q]):
        y[0, :, k] = [(x * tinv) % big.Q % p for p in pb]
    assert _L(ref_cpu.contract(cb, cs, t, y)[0]) == spec.switch_poly(spec.multround_poly(_L(y[0]), big, t, small.Q), big, small)
    c1, c2 = H.rand_residues(rng, qs, (1, 2), N), H.rand_residues(rng, qs, (1, 2), N)
    out = ref_cpu.bfv_mul(cs, cb, t, c1, c2)
    assert [_L(p) for p in out[0]] == spec.bfv_enc_mul([_L(p) for p in c1[0]], [_L(p) for p in c2[0]], small, big, t)


def test_oracle_bfv_at_13_of_27_limbs_matches_spec_at_1024():
    """the same at a block-kernel degree, N = 1024 (superset arrangement): switch, contract and the whole product"""
    N, t, ns, nb = 1024, 65537, 13, 27
    pb = H.chain(50, nb, N)
    qs = pb[:ns]
    small, big = spec.Ring(N, qs), spec.Ring(N, pb)
    cs, cb = ref_cpu.RefCtx(N, qs), ref_cpu.RefCtx(N, pb)
    rng = np.random.default_rng(1024 + ns)
    a = H.rand_residues(rng, qs, (1,), N)
    for k, x in enumerate([0, 1, small.Q - 1, small.Q // 2, small.Q // 2 + 1]):
        a[0, :, k] = [x % q for q in qs]
    assert _L(ref_cpu.switch(cs, cb, a)[0]) == spec.switch_poly(_L(a[0]), small, big)
    y = H.rand_residues(rng, pb, (1,), N)
    tinv = pow(t, -1, big.Q)
    for k, x in enumerate([0, 1, big.Q - 1, big.Q // 2, big.Q // 2 + 1, small.Q // 2, small.Q // 2 + 1, small.Q]):
        y[0, :, k] = [(x * tinv) % big.Q % p for p in pb]
    assert _L(ref_cpu.contract(cb, cs, t, y)[0]) == spec.switch_poly(spec.multround_poly(_L(y[0]), big, t, small.Q), big, small)
    c1, c2 = H.rand_residues(rng, qs, (1, 2), N), H.rand_residues(rng, qs, (1, 2), N)
    out = ref_cpu.bfv_mul(cs, cb, t, c1, c2)
    assert [_L(p) for p in out[0]] == spec.bfv_enc_mul([_L(p) for p in c1[0]], [_L(p) for p in c2[0]], small, big, t)


def test_oracle_switch_and_contract_at_19_of_40_limbs_match_spec():
    N, t, ns, nb = 32, 257, 19, 40
    pb = H.chain(61, nb, N)
    qs = pb[:ns]
    small, big = spec.Ring(N, qs), spec.Ring(N, pb)
    cs, cb = ref_cpu.RefCtx(N, qs), ref_cpu.RefCtx(N, pb)
    rng = np.random.default_rng(nb)
    a = H.rand_residues(rng, qs, (1,), N)
    assert _L(ref_cpu.switch(cs, cb, a)[0]) == spec.switch_poly(_L(a[0]), small, big)
    y = H.rand_residues(rng, pb, (1,), N)
    assert _L(ref_cpu.contract(cb, cs, t, y)[0]) == spec.switch_poly(spec.multround_poly(_L(y[0]), big, t, small.Q), big, small)


# ---------------------------------------------------------------------------------------------------
# the kernel bodies (tests/emul) where the harness takes a limb count
# ---------------------------------------------------------------------------------------------------
def _conv_ref(a, t, vals, centred):
    A = 1
    for x in a:
        A *= x
    return np.array([[(spec.centred(v, A) if centred else v) % ti for ti in t] for v in vals], dtype=np.uint64)


@pytest.mark.parametrize("bits,k,m", [(40, 33, 7), (61, 33, 7), (50, 40, 40), (61, 40, 1), (40, 34, 34)])
@pytest.mark.parametrize("centred", [False, True])
def test_exact_conversion_bodies_at_33_to_40_source_limbs(bits, k, m, centred):
    """conv_core.h conv_prepare / conv_eval with every row of conv_tab_t in use (k = 40 sources, m = 40 targets)"""
    N = 64
    ch = H.chain(bits, k + m, N)
    a, t = ch[:k], ch[k:]
    A = 1
    for x in a:
        A *= x
    rng = random.Random(bits * k + m)
    vals = [rng.randrange(A) for _ in range(200)]
    vals += [0, 1, 2, A - 1, A - 2, A // 2, A // 2 + 1, A // 2 - 1, A // 2 + 2, a[0], a[-1], A // a[0], A - A // a[-1]]
    res = np.array([[v % x for x in a] for v in vals], dtype=np.uint64)
    got, slow = emul.conv(a, t, res, centred)
    assert np.array_equal(got, _conv_ref(a, t, vals, centred))
    assert slow > 0                                                       # the structured values force the exact multi-word branch


@pytest.mark.parametrize("bits,k,w", [(40, 33, 16), (50, 34, 16), (61, 40, 32), (40, 40, 7)])
def test_window_digit_bodies_at_33_to_40_limbs(bits, k, w):
    """conv_core.h window_digits_coeff: the reconstruction runs at k words (words[TFHE_MAX_LIMBS + 1] at k = 40)"""
    qs = H.chain(bits, k, 64)
    Q = 1
    for q in qs:
        Q *= q
    nwin = -(-Q.bit_length() // w)
    rng = random.Random(bits * 100 + k)
    xs = [0, 1, Q - 1, Q // 2, Q // 2 + 1, 1 << (Q.bit_length() - 1), (1 << 64) % Q, (1 << (64 * (k - 1))) % Q] + [rng.randrange(Q) for _ in range(200)]
    res = np.array([[x % q for q in qs] for x in xs], dtype=np.uint64)
    got = emul.window_digits(qs, w, nwin, res)
    want = np.array([[(x >> (i * w)) & ((1 << w) - 1) for i in range(nwin)] for x in xs], dtype=np.uint64)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("mode", ["superset", "disjoint"])
@pytest.mark.parametrize("bits,ns,nb", [(50, 13, 27), (61, 19, 40), (40, 7, 33)])
def test_bfv_expand_contract_bodies_beyond_the_fast_tables(mode, bits, ns, nb):
    """bfv_core.h bfv_expand_coeff / bfv_contract_coeff (the general kernels' bodies) at basis sizes past TFHE_FAST_MAX = 12,
    up to a 40-limb extension basis"""
    N, t = 32, 65537
    ch = H.chain(bits, ns + nb, N)
    qs = ch[:ns]
    pb = ch[:nb][::-1] if mode == "superset" else ch[ns:]                  # superset: shared primes last
    cs, cb = ref_cpu.RefCtx(N, qs), ref_cpu.RefCtx(N, pb)
    small, big = spec.Ring(N, qs), spec.Ring(N, pb)
    rng = np.random.default_rng(bits + ns)
    a = H.rand_residues(rng, qs, (3,), N)
    for k, x in enumerate([0, 1, small.Q - 1, small.Q // 2, small.Q // 2 + 1, 7, small.Q - 7]):
        a[0, :, k] = [x % q for q in qs]
    got, _ = emul.bfv(qs, pb, t, a, N, contract=False)
    assert np.array_equal(got, ref_cpu.switch(cs, cb, a))
    y = H.rand_residues(rng, pb, (3,), N)
    tinv = pow(t, -1, big.Q)
    edges = [0, 1, big.Q - 1, big.Q // 2, big.Q // 2 + 1, small.Q // 2, small.Q // 2 + 1, small.Q, small.Q - 1,
             3 * small.Q + small.Q // 2, 3 * small.Q + small.Q // 2 + 1, big.Q - small.Q // 2, big.Q - small.Q // 2 - 1]
    for k, x in enumerate(edges):
        y[0, :, k] = [(x * tinv) % big.Q % p for p in pb]
    got, slow = emul.bfv(qs, pb, t, y, N, contract=True)
    assert np.array_equal(got, ref_cpu.contract(cb, cs, t, y))
    assert slow > 0


@pytest.mark.parametrize("smant,sexp", [(1, 40), (1, 80), (12345, 30)])
def test_ckks_magnitudes_beyond_1024_bits_scale_into_a_double(smant, sexp):
    """ckks_core.h ckks_words_to_double on the magnitudes of 17 and more 61-bit limbs (Q > 2^1024): the magnitude alone is no
    double, its quotient by the scale is whenever it stays below 2^1024 -- against exact rational arithmetic (ckks.jl:52-58);
    beyond that range the result is +-inf, as the reference's Float64(n / scale) gives"""
    from fractions import Fraction
    scale = Fraction(smant) * Fraction(2) ** sexp
    rng = random.Random(smant + sexp)
    top = 1023 + scale.numerator.bit_length() - 1                     # largest bit length whose quotient is surely finite
    for bits in [1020, 1024, 1025, 1037, top - 1, top] + [rng.randint(1000, top) for _ in range(60)]:
        mag = rng.getrandbits(bits) | (1 << (bits - 1))
        neg = rng.random() < 0.5
        got = emul.ckks_to_double(mag, neg, smant, sexp)
        exact = Fraction(-mag if neg else mag) / scale
        if smant == 1:
            assert got == float(exact), (bits, neg)
        else:
            assert abs(Fraction(got) - exact) <= abs(exact) * Fraction(1, 2**51), (bits, neg)
    assert emul.ckks_to_double(1 << 2400, False, smant, sexp) == float("inf")
    assert emul.ckks_to_double(1 << 2400, True, smant, sexp) == float("-inf")
