"""tfhe_ckks_encode / tfhe_ckks_decode against exact references (tests/exact_ref.py).

(a) The exact parts as compiled for the device, bit for bit.  A slot vector whose entries are all the same real c leaves the
    passes, in exact double arithmetic, as c in coefficient 0 and zero elsewhere (every butterfly adds equal values or multiplies
    by roots[0] = 1; N c is a power-of-two scaling; tw[0] = 1 -- tests/test_exact_ref_cpu.py shows it on the numpy passes).  So a
    batch of constants observes ckks_round_scaled and ckks_residue word for word against Fraction, and a polynomial with only
    coefficient 0 set observes the CRT centring and ckks_words_to_double the same way.
(b) The transforms against the exact coefficients and slots:
        |n_k - scale X_k| <= 1/2 + scale T,   T  = K eps log2(N) ||cm||_2 / N
        |slot - exact|    <= T',              T' = K eps log2(N) ||v||_2  (+ 2^-51 ||v||_1 where the scale's mantissa is not 1:
                                                                            the representation error ckks_words_to_double may have)
    K is 4 times the largest error, in those units, that the numpy restatement of the passes shows against the exact reference
    over this file's own inputs (4: fp contraction and the sinl / cosl tables change single roundings, not the order)."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from tests import exact_ref as X
from tests import helpers as H
from tests import many_limbs as ML

pytestmark = pytest.mark.gpu
mpf, mpc = X.mpf, X.mpc


def dev(a):
    return tf.DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def encode(ctx, L, mant, exp2, slots):
    """slots [batch][N/2] complex128 -> words [batch][L][N]"""
    slots = np.ascontiguousarray(slots, dtype=np.complex128)
    out = tf.DeviceBuffer(slots.shape[0] * L * ctx.N)
    ctx.ckks_encode(L, mant, exp2, dev(slots.view(np.uint64)).ptr, out.ptr, slots.shape[0])
    return out.to_numpy((slots.shape[0], L, ctx.N))


def decode(ctx, L, mant, exp2, words):
    """words [batch][L][N] -> slots [batch][N/2] complex128"""
    out = tf.DeviceBuffer(words.shape[0] * ctx.N)
    ctx.ckks_decode(L, mant, exp2, dev(words).ptr, out.ptr, words.shape[0])
    return out.to_numpy().view(np.complex128).reshape(words.shape[0], ctx.N // 2)


# ----------------------------------------------------------------------------------------------------------------------
# (a) the exact parts
# ----------------------------------------------------------------------------------------------------------------------
SCALE_PARTS = [(1, 0), (1, 40), (1, 80), (12345, 20), (2**63 + 12345, -23)]
T_LEGS = [-40, -7, 0, 1, 30, 63, 64, 65, 100, 127, 128, 129, 140]     # t = -(e + sexp): lshift leg (t <= 0), 1 <= t < 64, 64, 64 < t < 128, 128, above


def constants_for(mant, sexp):
    rng = np.random.default_rng(mant % 1000 + sexp + 100)
    xs = [0.0, -0.0, 1.0, -1.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 1e-300, 5e-324, 123456.789, 3.75e10, -3.75e10,
          2.0**70 + 2.0**20, -(2.0**70 + 2.0**20), 1.5 * 2.0**100, -1e30]                    # ties at scale 1; magnitudes >= 2^64, >= q
    for t in T_LEGS:
        e = -t - sexp
        for m in [2**52, 2**52 + 1, 2**53 - 1] + [int(v) | 2**52 for v in rng.integers(0, 2**52, size=3)]:
            if -1022 <= e + 52 <= 1023:
                xs += [float(np.ldexp(float(m), e)) * (-1) ** (m & 1)]
    # ties: x scale = k + 1/2 exactly.  mant = 1: x = (2k + 1) 2^-(sexp + 1); mant odd: x = j 2^-(sexp + 1) with j odd gives mant j / 2
    for j in [1, 3, 5, 7, -1, -3, -5, 2**20 + 1, 2**20 + 3, -(2**41 + 1), 2**41 + 3, 2**52 + 1, 2**52 + 3]:
        xs.append(float(np.ldexp(float(j), -(sexp + 1))))
    return np.array(xs, dtype=np.float64)


@pytest.mark.parametrize("N", [16, 1 << 12])
@pytest.mark.parametrize("mant,sexp", SCALE_PARTS)
def test_constant_slots_show_the_device_rounding_word_for_word(N, mant, sexp):
    qs = H.chain(61, 1, N) + H.chain(50, 1, N) + H.chain(30, 1, N)
    ctx = tf.Context(N, qs)
    cs = constants_for(mant, sexp)
    scale = Fraction(mant) * Fraction(2) ** sexp
    prods = [Fraction(float(c)) * scale for c in cs]
    ns = [X.round_half_even(p) for p in prods]
    ties = sum(1 for p in prods if p.denominator == 2)
    assert ties >= 13 and sum(1 for n in ns if abs(n) >= 2**64) >= 4 and sum(1 for n in ns if abs(n) >= qs[0]) >= 4 and min(ns) < 0
    got = encode(ctx, 3, mant, sexp, np.repeat(cs[:, None], N // 2, axis=1).astype(np.complex128))
    for l, q in enumerate(qs):
        want = np.array([n % q for n in ns], dtype=np.uint64)
        bad = np.flatnonzero(got[:, l, 0] != want)
        assert bad.size == 0, [(float(cs[i]).hex(), int(got[i, l, 0]), int(want[i])) for i in bad[:5]]
    assert not got[:, :, 1:].any()                                    # every other word is 0


def _decode_rings(N):
    return {1: H.chain(61, 1, N), 2: H.chain(61, 1, N) + H.chain(50, 1, N), 17: H.chain(61, 17, N), 40: ML.ring("W40", N)}


@pytest.mark.parametrize("N", [16, 1 << 12])
@pytest.mark.parametrize("L", [1, 2, 17, 40])
def test_single_coefficient_shows_the_device_centring_and_conversion(N, L):
    """only coefficient 0 set, to the residues of n: every slot decodes to the same double -- float(n / scale) for a
    power-of-two scale, within relative 2^-51 of it otherwise (the figure tests/test_kernel_bodies_cpu.py holds the host build
    to) -- with imaginary part +-0.  n of every length up to L limbs, both signs, and the centring seam Q / 2, Q / 2 + 1"""
    qs = _decode_rings(N)[L]
    ctx = tf.Context(N, qs)
    Q = 1
    for q in qs:
        Q *= q
    rng = np.random.default_rng(L)
    ns = [0, 1, -1, 12345, -12345, 2**53 + 1, -(2**53 + 3), Q // 2, Q // 2 + 1, Q // 2 - 1, -(Q // 2) + 1]
    ns += [s * v for v in (2**64 - 1, 2**64, 2**64 + 2**11, 2**128 - 1, 2**128 + 2**75) if v < Q // 2 for s in (1, -1)]
    for bits in sorted({Q.bit_length() - 2, Q.bit_length() // 2, 100, 64 * (Q.bit_length() // 64)}):
        if 1 < bits < Q.bit_length() - 1:
            ns += [s * (int.from_bytes(rng.bytes(bits // 8 + 1), "little") % (1 << bits) | 1 << (bits - 1)) for s in (1, -1)]
    assert all(-(Q // 2) <= n <= Q // 2 + 1 for n in ns)
    words = np.zeros((len(ns), L, N), dtype=np.uint64)
    words[:, :, 0] = np.array([[n % q for q in qs] for n in ns], dtype=np.uint64)
    centred = [n - Q if n > Q // 2 else n for n in ns]                # ckks.jl:54-56
    top = Q.bit_length()
    for mant in (1, 12345, 2**63 + 12345):
        for sexp in sorted({40, max(40, top - 60), max(40, top - 900)}):
            if top - sexp - mant.bit_length() > 1000:
                continue                                               # the quotient itself would not be a double
            scale = Fraction(mant) * Fraction(2) ** sexp
            got = decode(ctx, L, mant, sexp, words)
            assert np.array_equal(got.real, np.repeat(got.real[:, :1], N // 2, axis=1)) and not got.imag.any()
            for i, n in enumerate(centred):
                exact = Fraction(n) / scale
                g = float(got[i, 0].real)
                if n != 0 and abs(exact) < Fraction(1, 2**1021):      # below the normal range: neither figure applies
                    assert abs(g) <= 2.0**-1021
                elif mant == 1:
                    assert g == float(exact), (n, sexp, g, float(exact))
                else:
                    assert abs(Fraction(g) - exact) <= abs(exact) * Fraction(1, 2**51), (n, mant, sexp, g, float(exact))
                assert n != 0 or (g == 0.0 and np.signbit(g) == False)


# ----------------------------------------------------------------------------------------------------------------------
# (b) the transforms
# ----------------------------------------------------------------------------------------------------------------------
ALL_SIZES = X.CKKS_FULL_SIZES + X.CKKS_SAMPLED_SIZES


def scale_parts(scale):
    mant, exp2 = tf.she.scale_parts(scale)
    return mant, exp2, Fraction(mant) * Fraction(2) ** exp2           # the scale the device is told, exactly


@functools.lru_cache(maxsize=None)
def ratios_np():
    """the error of the numpy passes in units of eps log2(N) ||.||_2 (/ N) over every input of this file"""
    out = {}
    for N in ALL_SIZES:
        for kind in X.CKKS_KINDS:
            out[("encode", kind, N)] = X.encode_ratio_np(kind, N)
        for label, scale, bits, L in X.CKKS_SCALES:
            mant, exp2, _ = scale_parts(scale)
            out[("decode", label, N)] = X.decode_ratio_parts_np(N, tuple(H.chain(bits, L, N)), mant, exp2)
    return out


def K():
    return X.K_FACTOR * max(ratios_np().values())


def _items(ex):
    return ex.items() if isinstance(ex, dict) else enumerate(ex)


@pytest.mark.parametrize("N", ALL_SIZES)
def test_encode_against_the_exact_coefficients(N):
    k_const = K()
    ctxs = {}
    for label, scale, bits, L in X.CKKS_SCALES:
        qs = tuple(H.chain(bits, L, N))
        if qs not in ctxs:
            ctxs[qs] = tf.Context(N, list(qs))
        ctx = ctxs[qs]
        Q = 1
        for q in qs:
            Q *= q
        mant, exp2, s = scale_parts(scale)
        D = s.denominator << X.FIXED_P
        for kind in X.CKKS_KINDS:
            z = X.ckks_slots_input(kind, N)
            got = encode(ctx, L, mant, exp2, z)
            used, worst = 0, 0.0
            for b, (ks, xi) in enumerate(X.exact_coeffs_fixed(kind, N)):
                # exact integer work on y_k = scale X_k = num_k / D  (X_k to 2^-256: far below what any bound here resolves)
                n = X.crt_centred(got[b][:, ks], qs)
                num = xi * s.numerator
                fl = num // D
                rem2 = 2 * (num - fl * D)
                R = fl + ((rem2 > D).astype(bool) | ((rem2 == D).astype(bool) & (fl % 2 == 1).astype(bool)))   # rint(y_k), ties to even
                d = (n - R + Q // 2) % Q - Q // 2                       # n_k - rint(scale X_k), modulo Q (magnitudes may wrap)
                err = abs(d * D + R * D - num)                          # |n_k - y_k| D
                unit = float(s) * X.encode_unit(z[b], N)
                bound = Fraction(0.5) + Fraction(k_const * unit)
                bad = np.flatnonzero((err > int(bound * D)).astype(bool))
                assert bad.size == 0, (label, kind, N, b, [(int(ks[i]), float(Fraction(int(err[i]), D)), float(bound)) for i in bad[:5]])
                free = np.flatnonzero((d != 0).astype(bool))            # only a coefficient this close to a half-integer is free
                used += free.size
                for i in free:
                    assert Fraction(abs(int(rem2[i]) - D), 2 * D) <= Fraction(k_const * unit), (label, kind, N, b, int(ks[i]), int(d[i]))
                if unit > 0:
                    worst = max(worst, (float(Fraction(int(err.max()), D)) - 0.5) / unit)   # the rounding's half unit taken off
            print("encode N %d scale %s %s: K %.3f, device-to-exact ratio %s, %d coefficients used the half-integer allowance"
                  % (N, label, kind, k_const, "%.3f" % worst if label == "2^80" else "n/a (rounding hides it)", used))


@pytest.mark.parametrize("N", ALL_SIZES)
def test_decode_against_the_exact_slots(N):
    k_const = K()
    ctxs = {}
    for label, scale, bits, L in X.CKKS_SCALES:
        qs = tuple(H.chain(bits, L, N))
        if qs not in ctxs:
            ctxs[qs] = tf.Context(N, list(qs))
        mant, exp2, s = scale_parts(scale)
        inv = mpf(s.denominator) / mpf(s.numerator)
        res, ints = X.decode_input(N, qs)
        got = decode(ctxs[qs], L, mant, exp2, res)
        sums = X.exact_slot_sums(N, qs)
        worst = 0.0
        for b in range(3):
            v = X.words_to_double_np(ints[b], mant, exp2)
            unit = X.decode_unit(np.linalg.norm(v), N)
            tol = k_const * unit + (0.0 if mant == 1 else 2.0**-51 * float(np.abs(v).sum()))
            for i, S in _items(sums[b]):
                err = float(abs(mpc(complex(got[b, i])) - S * inv))
                assert err <= tol, (label, N, b, i, err, tol)
                worst = max(worst, err / unit)
        print("decode N %d scale %s: K %.3f, device-to-exact ratio %.3f" % (N, label, k_const, worst))
