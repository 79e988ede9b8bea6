"""tests/exact_ref.py checked against the definitions it restates, and the conditions that tests/test_gpu_gaussian_exact.py and
tests/test_gpu_ckks_exact.py rest on: the half-integer cap of the Gaussian cases, the chi-square seed, the constant K."""
import cmath
from fractions import Fraction

import numpy as np
import pytest

from oracle import spec
from tests import exact_ref as X
from tests import helpers as H

mpf, mpc, MP = X.mpf, X.mpc, X.MP


def test_philox_block_np_is_the_spec_block():
    rng = np.random.default_rng(1)
    idx = np.concatenate([np.array([0, 1, (5 << 32) | 7, ((2**32 - 1) << 32) | 4095, 2**64 - 1], dtype=np.uint64),
                          rng.integers(0, 2**63, size=200, dtype=np.uint64) * np.uint64(2) + np.uint64(1)])
    for stream, seed in ((1, X.GAUSS_SEED), (9, 0), (0xFFFFFFFF, 2**64 - 1)):
        w, u1, u2, z = X.philox_block_np(idx, stream, seed)
        for n, i in enumerate(int(v) for v in idx):
            b = spec.philox4x32_10((i & 0xFFFFFFFF, i >> 32, 0xFFFFFFFF, stream), (seed & 0xFFFFFFFF, seed >> 32))
            assert [int(w[j][n]) for j in range(4)] == list(b)
            r0, r1 = (b[1] << 32) | b[0], (b[3] << 32) | b[2]
            assert u1[n] == (float(r0 >> 11) + 1.0) * 2.0**-53 and u2[n] == float(r1 >> 11) * 2.0**-53
        assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1


def _case_draws(N, stream, first, count):
    idx = X.gauss_counters(first, count, N)
    _, u1, u2, z = X.philox_block_np(idx, stream, X.GAUSS_SEED)
    return idx.ravel(), u1.ravel(), u2.ravel(), z.ravel()


@pytest.mark.parametrize("N", [4096, 64])
def test_gauss_exact_rounds_to_the_spec_sampler_and_the_half_integer_cap_holds(N):
    """for every case of the GPU test whose sigma takes the exact form: no draw of the fixed subset lies within sigma 2^-44 of a
    half-integer, the numpy doubles round to the exact rounding on all of them, and (first case of each counter set) the exact
    rounding is oracle/spec.py's sample_gauss_int.  The cap is a cap: a seed that breaks it is changed, not the cap."""
    worst_z, seen = mpf(0), set()
    for sigma, stream, first, count in X.gauss_cases(N):
        if not X.gauss_exact_form(sigma):
            continue
        idx, u1, u2, z = _case_draws(N, stream, first, count)
        sub = X.gauss_subset(N, count)
        e_np = X.gauss_ints_np(z, sigma)
        for i in sub:
            y = X.gauss_exact(u1[i], u2[i], sigma)
            assert X.half_integer_distance(y) > sigma * X.GAUSS_MARGIN, (sigma, stream, first, int(i))
            assert X.rint_exact(y) == int(e_np[i]), (sigma, stream, first, int(i))
            worst_z = max(worst_z, abs(y / mpf(sigma) - mpf(float(z[i]))))
        if (stream, first) not in seen and sigma <= 19.2:
            seen.add((stream, first))
            for i in sub[::8]:
                assert spec.sample_gauss_int(int(idx[i]), stream, X.GAUSS_SEED, sigma) == X.rint_exact(X.gauss_exact(u1[i], u2[i], sigma))
    assert worst_z < 2e-14, worst_z          # the host libm's own |z| error sits inside the figure the margin is derived from


def test_gauss_exact_is_the_definition():
    """sigma sqrt(-2 ln u1) cos(2 pi u2) at points with a closed form, and against a 400-bit evaluation"""
    assert X.gauss_exact(1.0, 0.25, 3.2) == 0                                  # ln 1 = 0
    assert abs(X.gauss_exact(0.5, 0.0, 2.0) - 2 * MP.sqrt(2 * MP.log(2))) < mpf(2) ** -180
    assert abs(X.gauss_exact(0.5, 0.5, 2.0) + 2 * MP.sqrt(2 * MP.log(2))) < mpf(2) ** -180
    import mpmath
    with mpmath.workprec(400):
        u1, u2 = 2.0**-53, 1 - 2.0**-53
        want = 1e15 * mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(u1))) * mpmath.cos(2 * mpmath.pi * mpmath.mpf(u2))
        assert abs(mpmath.mpf(X.gauss_exact(u1, u2, 1e15)) - want) < mpmath.mpf(2) ** -120
    assert abs(X.gauss_exact(2.0**-53, 0.0, 1.0)) < 8.6                          # the |z| bound the margin uses


@pytest.mark.parametrize("N", [4, 8, 16, 64])
def test_transforms_equal_the_quadratic_definition(N):
    """both forms of the whole-polynomial transform (mpc, fixed point) and the direct single-coefficient sums against
    X_k = Re(psi^k / N sum_j cm_j w^(jk)) and slot_i = sum_k n_k / scale psi^(-k e_i) written out term by term"""
    z = X.ckks_slots_input("mixed" if N > 4 else "random", N)[1]
    cm = X.scatter_exact(z, N)
    want = [(MP.expjpi(mpf(k) / N) * sum(cm[j] * MP.expjpi(mpf(2 * j * k) / N) for j in range(N))).real / N for k in range(N)]
    tol = mpf(2) ** -150 * max(abs(c) for c in cm)
    for got in (X.ckks_coeffs_exact(z, N, fixed=False), X.ckks_coeffs_exact(z, N, fixed=True), X.ckks_coeffs_exact_some(z, N, range(N))):
        assert max(abs(g - w) for g, w in zip(got, want)) < tol
    assert all(abs((MP.expjpi(mpf(k) / N) * sum(cm[j] * MP.expjpi(mpf(2 * j * k) / N) for j in range(N))).imag) < tol for k in range(N))
    ints = [int(v) for v in np.random.default_rng(N).integers(-2**62, 2**62, size=N)] if N > 4 else [2**100 + 1, -1, 0, 3]
    scale = Fraction(10**12, 7)
    es = X.slot_exponents(N)
    want = [sum(mpf(ints[k]) * MP.expjpi(-mpf(k * es[i]) / N) for k in range(N)) * 7 / mpf(10**12) for i in range(N // 2)]
    tol = mpf(2) ** -150 * max(abs(n) for n in ints)
    for got in (X.ckks_slots_exact(ints, scale, N, fixed=False), X.ckks_slots_exact(ints, scale, N, fixed=True),
                X.ckks_slots_exact_some(ints, scale, N, range(N // 2))):
        assert max(abs(g - w) for g, w in zip(got, want)) < tol


def test_fixed_point_transform_is_the_mpc_transform_where_the_tests_switch():
    """N = 256 is the last size that runs in mpc; the fixed-point passes give the same there and at 1024, and the direct sums
    the same as the transform at 4096"""
    for N in (256, 1024):
        z = X.ckks_slots_input("random", N)[0]
        a, b = X.ckks_coeffs_exact(z, N, fixed=False), X.ckks_coeffs_exact(z, N, fixed=True)
        assert max(abs(x - y) for x, y in zip(a, b)) < mpf(2) ** -150
    N = 4096
    z = X.ckks_slots_input("mixed", N)[2]
    full, ks = X.exact_coeffs("mixed", N)[2], X.sampled_positions(N)
    assert max(abs(full[k] - v) for k, v in zip(ks, X.ckks_coeffs_exact_some(z, N, ks))) < mpf(2) ** -100
    qs = tuple(H.chain(40, 3, N))
    _, ints = X.decode_input(N, qs)
    sums, pos = X.exact_slot_sums(N, qs)[0], X.sampled_positions(N // 2)
    assert max(abs(sums[i] - v) for i, v in zip(pos, X.ckks_slots_exact_some(ints[0], 1, N, pos))) < mpf(2) ** -30   # |n| ~ 2^119


@pytest.mark.parametrize("N,bits,L,scale", [(32, 40, 3, 2**40), (256, 50, 2, 2**40), (16, 50, 2, 12345 * 2**20)])
def test_exact_transform_agrees_with_the_spec_codec_within_the_old_tolerance(N, bits, L, scale):
    """oracle/spec.py's numpy codec, the reference of the older tests, against the exact one under those tests' own allowance"""
    qs = H.chain(bits, L, N)
    ring = spec.Ring(N, qs)
    rng = np.random.default_rng(N + L)
    slots = rng.normal(size=N // 2) * 3 + 1j * rng.normal(size=N // 2)
    got = [spec.centred(v, ring.Q) for v in spec.poly_to_ints(spec.ckks_encode(list(slots), ring, scale), ring)]
    ex = X.ckks_coeffs_exact(slots, N)
    allowed = max(1, int(8 * np.log2(N) * X.EPS * np.abs(slots).max() * float(scale)))
    assert max(abs(g - X.rint_exact(e * scale)) for g, e in zip(got, ex)) <= allowed
    dec = spec.ckks_decode(spec.poly_from_ints(got, ring), ring, scale)
    exd = X.ckks_slots_exact(got, scale, N)
    tol = 8 * np.log2(N) * X.EPS * max(1.0, np.abs(dec).max()) * 4
    assert max(abs(mpc(complex(d)) - e) for d, e in zip(dec, exd)) <= tol


@pytest.mark.parametrize("N", [16, 4096, 1 << 15])
def test_constant_slots_encode_exactly_in_the_numpy_passes(N):
    """what the bit-for-bit device test of the exact parts rests on: a slot vector of one real constant leaves the passes as
    that constant in coefficient 0 and (signed) zero everywhere else -- no rounding anywhere"""
    cs = np.array([1.0, -2.5, 3.75e10, 2.0**-52, -(2.0**70), 1e-300, 12345.678, -0.0])
    x = X.ckks_encode_passes_np(np.repeat(cs[:, None], N // 2, axis=1).astype(np.complex128), N)
    assert np.array_equal(x[:, 0], cs) and not x[:, 1:].any()
    v = np.zeros((cs.size, N))
    v[:, 0] = cs
    s = X.ckks_decode_passes_np(v, N)
    assert np.array_equal(s.real, np.repeat(cs[:, None], N // 2, axis=1)) and not s.imag.any()


def test_chi_square_seed_passes_on_the_numpy_stream():
    idx = X.gauss_counters(X.CHI_FIRST, X.CHI_POLYS, X.CHI_N)
    _, _, _, z = X.philox_block_np(idx, X.CHI_STREAM, X.CHI_SEED)
    e = X.gauss_ints_np(z, X.CHI_SIGMA)
    stat, thr = X.chi_square_gauss(e, X.CHI_SIGMA)
    assert e.size == 2**20 and stat <= thr, (stat, thr)
    lo, hi, exp = X.gauss_bins(X.CHI_SIGMA, e.size)
    assert exp.min() >= 20 and abs(exp.sum() - e.size) < 1e-6 and hi >= 4 * X.CHI_SIGMA
    r, n = X.neighbour_correlation(e)
    assert abs(r) <= 6 / np.sqrt(n), r
    # the check bites: a stream whose neighbours share a uniform, or whose sigma is 2 % off, fails
    assert abs(X.neighbour_correlation(e + np.roll(e, 1, axis=1))[0]) > 6 / np.sqrt(n)
    stat_off, _ = X.chi_square_gauss(X.gauss_ints_np(z, X.CHI_SIGMA * 1.02), X.CHI_SIGMA)
    assert stat_off > thr


def test_the_constant_K_measured():
    """K of tests/test_gpu_ckks_exact.py: 4 times the largest error of the numpy passes, in units of eps log2(N) ||.||_2 (/ N),
    over the full-size inputs of that test.  Measured here so that a change of the inputs or of the restatement shows: the
    ratios of whole polynomials lie between 0.3 and 4 (alternating slots, whose energy lands in few coefficients, are the top)."""
    ratios = {(kind, N): X.encode_ratio_np(kind, N) for kind in X.CKKS_KINDS for N in X.CKKS_FULL_SIZES}
    print("encode ratios", {k: round(v, 3) for k, v in ratios.items()})
    assert 0.3 <= min(ratios.values()) and max(ratios.values()) <= 4.0
    dec = {}
    for N in X.CKKS_FULL_SIZES:
        for bits, L, scale in ((50, 2, 2**40), (40, 3, 2**80)):
            dec[(N, bits)] = X.decode_ratio_np(N, tuple(H.chain(bits, L, N)), scale)
    print("decode ratios", {k: round(v, 3) for k, v in dec.items()})
    assert 0.3 <= min(dec.values()) and max(dec.values()) <= 4.0
