"""tfhe_sample_gaussian against the exact value of every draw: sigma sqrt(-2 ln u1) cos(2 pi u2) in mpmath (tests/exact_ref.py)
over the Philox stream the header defines.  The noise of every key and every ciphertext is "the words of tfhe_sample_gaussian"
(tests/test_gpu_encrypt.py, tests/test_gpu_keygen.py), so this is where the noise itself is pinned.

The rule |e - y| <= 1/2 + sigma 2^-44 is derived (exact_ref.GAUSS_MARGIN); tests/test_exact_ref_cpu.py shows that for the sigmas
up to 2^21 (and 3.2 2^20) no checked draw lies that close to a half-integer, so there the rule reads e == rint(y)."""
import functools

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from tests import exact_ref as X
from tests import helpers as H

pytestmark = pytest.mark.gpu

SEED = X.GAUSS_SEED


@functools.lru_cache(maxsize=None)
def ring(N):
    """limbs of 61, 50 and 30 bits"""
    qs = H.chain(61, 1, N) + H.chain(50, 1, N) + H.chain(30, 1, N)
    return tf.Context(N, qs), qs


def draw(N, level, sigma, mult, stream, first, count, seed=SEED):
    ctx, qs = ring(N)
    out = tf.DeviceBuffer(count * level * N)
    ctx.sample_gaussian(level, sigma, mult, seed, stream, first, out.ptr, count)
    return out.to_numpy((count, level, N))


def centre(words, q):
    w = words.astype(np.int64)
    return np.where(w > q // 2, w - q, w)


@functools.lru_cache(maxsize=None)
def stream_doubles(N, stream, first, count):
    _, u1, u2, z = X.philox_block_np(X.gauss_counters(first, count, N), stream, SEED)
    return u1.ravel(), u2.ravel(), z.ravel()


@pytest.mark.parametrize("N", [4096, 64])
@pytest.mark.parametrize("case", range(len(X.gauss_cases(4096))))
def test_every_coefficient_against_the_exact_value(N, case):
    sigma, stream, first, count = X.gauss_cases(N)[case]
    ctx, qs = ring(N)
    g = draw(N, 3, sigma, 1, stream, first, count)
    e = centre(g[:, 0], qs[0])                                       # |e| <= 8.6e15 < q_0 / 2: the 61-bit limb holds e itself
    for l in (1, 2):                                                 # one integer in every limb
        assert np.array_equal(g[:, l], np.mod(e, qs[l]).astype(np.uint64))
    e = e.ravel()
    u1, u2, z = stream_doubles(N, stream, first, count)
    mism = np.flatnonzero(e != X.gauss_ints_np(z, sigma))            # every disagreement with the numpy doubles goes to mpmath,
    check = np.union1d(mism, X.gauss_subset(N, count))               # and a fixed subset of the rest
    exact_form = X.gauss_exact_form(sigma)
    worst = 0.0
    for i in check:
        y = X.gauss_exact(u1[i], u2[i], sigma)
        d = abs(int(e[i]) - y)
        worst = max(worst, float(d))
        assert d <= 0.5 + sigma * X.GAUSS_MARGIN, (sigma, stream, first, int(i), int(e[i]), float(y))
        if exact_form:
            assert int(e[i]) == X.rint_exact(y), (sigma, stream, first, int(i), int(e[i]), float(y))
    print("sigma %g stream %d first %d N %d: %d of %d differ from the numpy doubles, %d sent to mpmath, largest |e - y| %.6g (allowed %.6g)"
          % (sigma, stream, first, N, mism.size, e.size, check.size, worst, 0.5 + sigma * X.GAUSS_MARGIN))
    if exact_form:
        assert mism.size == 0                                        # (the numpy doubles are the exact rounding there)


@pytest.mark.parametrize("N", [4096, 64])
def test_sigma_zero_writes_zero(N):
    for mult in (1, 2**61 - 1):
        assert not draw(N, 3, 0.0, mult, 1, 5, 8).any()


@pytest.mark.parametrize("N", [4096, 64])
@pytest.mark.parametrize("sigma", [3.2, 2.0**40])
def test_one_integer_in_every_limb_for_any_multiplier(N, sigma):
    """e from multiplier 1 (centred 61-bit limb), then every limb of a second call with the same counters must hold
    (m e) mod q_l exactly.  At sigma = 2^40 |e| exceeds the 30-bit modulus: the reduction of |e| itself in gauss_residue."""
    ctx, qs = ring(N)
    count = 8
    e = [int(v) for v in centre(draw(N, 3, sigma, 1, 1, 5, count)[:, 0], qs[0]).ravel()]
    assert max(abs(v) for v in e) >= (qs[2] if sigma > 2**30 else 8)
    for m in (65537, 2**61 - 1, qs[2], qs[2] + 1):
        g = draw(N, 3, sigma, m, 1, 5, count)
        for l, q in enumerate(qs):
            want = np.array([(m * v) % q for v in e], dtype=np.uint64).reshape(count, N)
            assert np.array_equal(g[:, l], want), (m, l)
    assert not draw(N, 3, sigma, qs[2], 1, 5, count)[:, 2].any()    # m = q_2: zero in the 30-bit limb


def test_distribution_of_a_million_draws():
    """2^20 draws at sigma = 3.2 (256 polynomials, level 1): chi-square over the integers (tails merged to an expected count of
    20, expected counts from the normal cdf in mpmath) under dof + 6 sqrt(2 dof), and no correlation between a draw and the draw
    of the next counter -- each takes both halves of its own Philox block"""
    ctx, qs = ring(X.CHI_N)
    e = centre(draw(X.CHI_N, 1, X.CHI_SIGMA, 1, X.CHI_STREAM, X.CHI_FIRST, X.CHI_POLYS, seed=X.CHI_SEED)[:, 0], qs[0])
    assert e.size == 2**20
    stat, thr = X.chi_square_gauss(e, X.CHI_SIGMA)
    r, n = X.neighbour_correlation(e)
    print("chi-square %.2f (threshold %.2f), neighbour correlation %.2e (bound %.2e)" % (stat, thr, r, 6 / np.sqrt(n)))
    assert stat <= thr
    assert abs(r) <= 6 / np.sqrt(n)
