"""High-precision references for the two float kernel families (host only; never loads the library).

  * the Gaussian stream of csrc/sample_kernels.h: the Philox4x32-10 block vectorised in numpy, the doubles u1, u2, z that
    sample_gauss_int forms, and sigma sqrt(-2 ln u1) cos(2 pi u2) evaluated by mpmath with u1, u2, sigma taken as the exact
    doubles they are and pi exact;
  * the CKKS codec of csrc/ckks_kernels.h: the real coefficients X_k and the decoded slots of ckksencoding.jl:56-97 with the
    root psi^k = exp(i pi k / N) exact (a radix-2 transform in mpc for whole polynomials, a direct sum for single
    coefficients at large N), and a numpy complex128 restatement of the device's own passes (same pass order, same table
    formulas, same bit-reversed positions) that is used only to size tolerances.

The tolerances the GPU tests apply, and the inputs they and tests/test_exact_ref_cpu.py share, are defined at the end."""
import functools
from fractions import Fraction

import mpmath
import numpy as np

PREC = 192                       # bits; every reference value is good to far below 2^-160 relative
MP = mpmath.mp.clone()           # a context of our own: the global mpmath precision stays what it was
MP.prec = PREC
mpf, mpc = MP.mpf, MP.mpc

EPS = 2.0 ** -53
TWO_PI_DOUBLE = 6.283185307179586476925286766559     # the literal of sample_gauss_int

# ----------------------------------------------------------------------------------------------------------------------
# the Gaussian stream
# ----------------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words (broadcast against each other) -> four word arrays"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3, k0, k1))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # 32 x 32 bits: no wrap in 64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return c0, c1, c2, c3


def philox_block_np(idx, stream, seed):
    """the block sample_gauss_int draws for counter idx (uint64 array): (words [4][...], u1, u2, z) with u1 in (0, 1],
    u2 in [0, 1) and z = sqrt(-2 log u1) cos(2 pi u2), all formed in double the way the kernel forms them"""
    idx = np.asarray(idx, dtype=np.uint64)
    b = philox4x32_10_np(idx & _M32, idx >> _S32, np.uint64(0xFFFFFFFF), np.uint64(stream),
                         np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    r0, r1 = (b[1] << _S32) | b[0], (b[3] << _S32) | b[2]
    u1 = ((r0 >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = (r1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI_DOUBLE * u2)
    return np.stack(b), u1, u2, z


def gauss_counters(first_poly, count, N):
    """the counters of tfhe_sample_gaussian(.., first_poly, .., count): [count][N] uint64"""
    p = (np.arange(count, dtype=np.uint64) + np.uint64(first_poly)) << _S32
    return p[:, None] | np.arange(N, dtype=np.uint64)[None, :]


def gauss_ints_np(z, sigma):
    """rint(sigma z) of the numpy doubles (ties to even), int64"""
    return np.rint(np.float64(sigma) * z).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _z_exact(u1: float, u2: float):
    return MP.sqrt(-2 * MP.log(mpf(u1))) * MP.cos(2 * MP.pi * mpf(u2))


def gauss_exact(u1, u2, sigma):
    """sigma sqrt(-2 ln u1) cos(2 pi u2) as an mpf; u1, u2, sigma are the exact doubles they are, pi is exact"""
    return mpf(float(sigma)) * _z_exact(float(u1), float(u2))


def half_integer_distance(y):
    """distance of the mpf y from the nearest half-integer"""
    f = y - MP.floor(y)
    return abs(f - mpf(0.5))


def rint_exact(y):
    """nearest integer of an mpf, ties to even (Python int)"""
    fl = int(MP.floor(y))
    r = y - fl
    if r > 0.5 or (r == 0.5 and fl % 2 == 1):
        return fl + 1
    return fl


# ----------------------------------------------------------------------------------------------------------------------
# CKKS: exact
# ----------------------------------------------------------------------------------------------------------------------
def slot_exponents(N):
    """e_i = 3^(i+1) mod 2N (ZmstarPermutation(2N)[1, :], ckksencoding.jl:49-54), i < N/2"""
    out, e = [], 1
    for _ in range(N // 2):
        e = (e * 3) % (2 * N)
        out.append(e)
    return out


@functools.lru_cache(maxsize=4)
def _quarter(N):
    """(cos, sin)(pi m / N) for m = 0 .. N/2, mpf"""
    return [MP.cos_sin(MP.pi * m / N) for m in range(N // 2 + 1)]


def _psi_pow(N, m):
    """psi^m = exp(i pi m / N) as (cos, sin), from the first quadrant by symmetry"""
    m %= 2 * N
    q = _quarter(N)
    if m <= N // 2:
        return q[m]
    if m <= N:
        c, s = q[N - m]
        return -c, s
    c, s = _psi_pow(N, m - N)
    return -c, -s


@functools.lru_cache(maxsize=4)
def _psi_table(N):
    """psi^m, m < 2N, as mpc"""
    return [mpc(*_psi_pow(N, m)) for m in range(2 * N)]


def _fft_mpc(x, N, sign):
    """y_k = sum_j x_j exp(sign 2 pi i j k / N): bit reversal, then radix-2 decimation-in-time passes in mpc"""
    logn = N.bit_length() - 1
    a = [None] * N
    for j in range(N):
        a[int(format(j, "0%db" % logn)[::-1], 2) if logn else 0] = x[j]
    psi = _psi_table(N)
    h = 1
    while h < N:
        step = N // h                                         # exp(2 pi i k / (2h)) = psi^(N k / h)
        w = [psi[(sign * step * k) % (2 * N)] for k in range(h)]
        for j0 in range(0, N, 2 * h):
            for k in range(h):
                u, t = a[j0 + k], a[j0 + k + h] * w[k]
                a[j0 + k], a[j0 + k + h] = u + t, u - t
        h *= 2
    return a


def scatter_exact(slots, N):
    """the length-N vector cm of ckksencoding.jl:75-80 as mpc"""
    cm = [mpc(0)] * N
    for i, e in enumerate(slot_exponents(N)):
        z = complex(slots[i])
        cm[e >> 1] = mpc(z.real, z.imag)
        cm[(2 * N - e) >> 1] = mpc(z.real, -z.imag)
    return cm


MPC_MAX_N = 256      # whole polynomials: the mpc transform up to here, the same passes in exact fixed point above (speed)


def ckks_coeffs_exact(slots, N, fixed=None):
    """the real coefficients X_k = Re(psi^k / N sum_j cm_j exp(2 pi i j k / N)) of ckksencoding.jl:72-97, k < N, as mpf"""
    if N > MPC_MAX_N if fixed is None else fixed:
        return _coeffs_fixed(slots, N)
    ip = _fft_mpc(scatter_exact(slots, N), N, +1)
    psi = _psi_table(N)
    return [(ip[k] * psi[k]).real / N for k in range(N)]


def ckks_slots_exact(ints, scale, N, fixed=None):
    """the decoding of integer coefficients (Python ints, centred) over the rational scale: slot_i = sum_k n_k / scale
    psi^(-k e_i)  (ckksencoding.jl:56-66), i < N/2, as mpc"""
    if N > MPC_MAX_N if fixed is None else fixed:
        return _slots_fixed(ints, scale, N)
    psi = _psi_table(N)
    f = _fft_mpc([psi[(-k) % (2 * N)] * mpf(int(ints[k])) for k in range(N)], N, -1)
    s = Fraction(scale)
    inv = mpf(s.denominator) / mpf(s.numerator)
    return [f[e >> 1] * inv for e in slot_exponents(N)]


# single coefficients by the direct O(N) sum.  Fixed point: the roots as integers with FRAC fractional bits (from mpmath), the
# doubles as the exact integers they are over a common power of two; every product and the sum are then exact integer work.
FRAC = PREC


@functools.lru_cache(maxsize=8)
def _psi_fixed(N):
    """psi^m, m < 2N, as two object arrays of integers (cos, sin) times 2^FRAC.  Up to MPC_MAX_N straight from mpmath; above,
    the even powers are the table of N/2 and the odd ones an even one times psi (from mpmath): one rounding of 2^-FRAC per
    doubling of N"""
    one = 1 << FRAC
    C, S = np.empty(2 * N, dtype=object), np.empty(2 * N, dtype=object)
    if N > MPC_MAX_N:
        C[0::2], S[0::2] = _psi_fixed(N // 2)
        c1, s1 = (int(MP.floor(v * one + 0.5)) for v in MP.cos_sin(MP.pi / N))
        C[1::2], S[1::2] = (C[0::2] * c1 - S[0::2] * s1) >> FRAC, (C[0::2] * s1 + S[0::2] * c1) >> FRAC
        return C, S
    q = [(int(MP.floor(c * one + 0.5)), int(MP.floor(s * one + 0.5))) for c, s in _quarter(N)]
    for m in range(2 * N):
        r = m % N
        c, s = q[r] if r <= N // 2 else (-q[N - r][0], q[N - r][1])
        C[m], S[m] = (c, s) if m < N else (-c, -s)
    return C, S


def _fft_fixed(re, im, N, sign):
    """_fft_mpc on object arrays of Python ints (values times a power of two that leaves FRAC guard bits below the last
    bit of any input): the same bit reversal and passes, each product rounded down at 2^-FRAC of the inputs' last place"""
    logn = N.bit_length() - 1
    C, S = _psi_fixed(N)
    j = np.arange(N)
    br = np.zeros(N, dtype=np.int64)
    for b in range(logn):
        br |= ((j >> b) & 1) << (logn - 1 - b)
    re, im = re[br], im[br]
    i = np.arange(N // 2)
    h = 1
    while h < N:
        k = i & (h - 1)
        lo = ((i - k) << 1) + k
        m = (sign * (N // h) * k) % (2 * N)
        wr, wi, yr, yi = C[m], S[m], re[lo + h], im[lo + h]
        tr, ti = (yr * wr - yi * wi) >> FRAC, (yr * wi + yi * wr) >> FRAC
        xr, xi = re[lo], im[lo]
        re[lo], im[lo], re[lo + h], im[lo + h] = xr + tr, xi + ti, xr - tr, xi - ti
        h *= 2
    return re, im


def _coeffs_fixed(slots, N):
    z = np.asarray(slots, dtype=np.complex128)
    both, shift = _as_integers(np.concatenate([z.real, z.imag]))
    zr, zi = both[:N // 2] << FRAC, both[N // 2:] << FRAC
    re, im = np.zeros(N, dtype=object), np.zeros(N, dtype=object)
    e = np.array(slot_exponents(N), dtype=np.int64)
    re[e >> 1], im[e >> 1] = zr, zi
    re[(2 * N - e) >> 1], im[(2 * N - e) >> 1] = zr, -zi
    re, im = _fft_fixed(re, im, N, +1)
    C, S = _psi_fixed(N)
    x = re * C[:N] - im * S[:N]
    den = mpf(1 << (2 * FRAC + shift)) * N
    return [mpf(int(v)) / den for v in x]


def _slots_fixed(ints, scale, N):
    n = np.array([int(v) for v in ints], dtype=object)
    C, S = _psi_fixed(N)
    mk = (-np.arange(N)) % (2 * N)
    re, im = _fft_fixed(n * C[mk], n * S[mk], N, -1)          # n_k psi^(-k) with FRAC guard bits
    s = Fraction(scale)
    inv = mpf(s.denominator) / mpf(s.numerator) / mpf(1 << FRAC)
    return [mpc(mpf(int(re[e >> 1])) * inv, mpf(int(im[e >> 1])) * inv) for e in slot_exponents(N)]


def _as_integers(x):
    """doubles -> (object array of Python ints, shift) with x = ints / 2^shift exactly"""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    mi = np.ldexp(m, 53).astype(np.int64).astype(object)      # x = mi 2^(e - 53)
    e = np.where(mi == 0, 0, e.astype(np.int64) - 53)
    emin = int(e.min())
    return mi << (e - emin).astype(object), -emin


def ckks_coeffs_exact_some(slots, N, ks):
    """X_k for the listed k by the direct sum X_k = 2/N sum_i Re(slot_i psi^(k e_i))"""
    z = np.asarray(slots, dtype=np.complex128)
    re, sr = _as_integers(z.real)
    im, si = _as_integers(z.imag)
    C, S = _psi_fixed(N)
    e = np.array(slot_exponents(N), dtype=np.int64)
    out = []
    for k in ks:
        idx = (e * int(k)) % (2 * N)
        a, b = int(np.dot(re, C[idx])), int(np.dot(im, S[idx]))
        out.append((mpf(a) / mpf(1 << (FRAC + sr)) - mpf(b) / mpf(1 << (FRAC + si))) * 2 / N)
    return out


def ckks_coeff_exact_one(slots, N, k):
    return ckks_coeffs_exact_some(slots, N, [k])[0]


def ckks_slots_exact_some(ints, scale, N, slot_idx):
    """decoded slot i for the listed i by the direct sum"""
    n = np.array([int(v) for v in ints], dtype=object)
    C, S = _psi_fixed(N)
    es = slot_exponents(N)
    kk = np.arange(N, dtype=np.int64)
    s = Fraction(scale)
    inv = mpf(s.denominator) / mpf(s.numerator) / mpf(1 << FRAC)
    out = []
    for i in slot_idx:
        idx = (kk * es[i]) % (2 * N)
        out.append(mpc(mpf(int(np.dot(n, C[idx]))) * inv, -mpf(int(np.dot(n, S[idx]))) * inv))
    return out


def ckks_slot_exact_one(ints, scale, N, i):
    return ckks_slots_exact_some(ints, scale, N, [i])[0]


def round_half_even(fr: Fraction) -> int:
    fl = fr.numerator // fr.denominator
    rem = fr - fl
    return fl + (1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1) else 0)


# ----------------------------------------------------------------------------------------------------------------------
# CKKS: the device's passes restated in numpy complex128 (sizes tolerances; never loads the library)
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=16)
def ckks_tables_np(N):
    """roots, tw, pos, gpos of toyfhe_hip.hip ckks_tables: roots from long double cos / sin rounded to double, tw from the
    Float64 angle of ckksencoding.jl:84, bit-reversed scatter and gather positions"""
    n2, logn = N // 2, N.bit_length() - 1
    t = np.arange(n2, dtype=np.longdouble)
    a = np.longdouble(-2.0) * np.longdouble("3.14159265358979323846264338327950288") * t / np.longdouble(N)
    roots = (np.cos(a).astype(np.float64), np.sin(a).astype(np.float64))
    k = np.arange(N, dtype=np.float64)
    ang = ((2 * k) / (2.0 * N)) * 3.14159265358979323846
    tw = (np.cos(ang), np.sin(ang))

    def brev(x):
        r = 0
        for i in range(logn):
            r |= ((x >> i) & 1) << (logn - 1 - i)
        return r
    es = slot_exponents(N)
    pos1 = np.array([brev(e >> 1) for e in es], dtype=np.int64)
    pos2 = np.array([brev((2 * N - e) >> 1) for e in es], dtype=np.int64)
    return roots, tw, pos1, pos2


def _fft_pass_np(re, im, roots, N, h, dif, conj_roots):
    """k_fft_pass over [batch][N], in place"""
    i = np.arange(N // 2)
    k = i & (h - 1)
    j = ((i - k) << 1) + k
    wr, wi = roots[0][k * ((N >> 1) // h)], roots[1][k * ((N >> 1) // h)]
    if conj_roots:
        wi = -wi
    xr, xi, yr, yi = re[:, j], im[:, j], re[:, j + h], im[:, j + h]
    if dif:
        dr, di = xr - yr, xi - yi
        re[:, j], im[:, j] = xr + yr, xi + yi
        re[:, j + h], im[:, j + h] = dr * wr - di * wi, dr * wi + di * wr
    else:
        tr, ti = yr * wr - yi * wi, yr * wi + yi * wr
        re[:, j], im[:, j] = xr + tr, xi + ti
        re[:, j + h], im[:, j + h] = xr - tr, xi - ti


def ckks_encode_passes_np(slots, N):
    """k_ckks_scatter, the DIT passes with conjugate roots and the real part of k_ckks_encode_finish: the doubles x_k
    [batch][N] that ckks_round_scaled then receives"""
    z = np.atleast_2d(np.asarray(slots, dtype=np.complex128))
    roots, tw, pos1, pos2 = ckks_tables_np(N)
    re, im = np.zeros((z.shape[0], N)), np.zeros((z.shape[0], N))
    re[:, pos1], im[:, pos1] = z.real, z.imag
    re[:, pos2], im[:, pos2] = z.real, -z.imag
    h = 1
    while h < N:
        _fft_pass_np(re, im, roots, N, h, 0, 1)
        h <<= 1
    return (re * tw[0] - im * tw[1]) / float(N)


def ckks_decode_passes_np(v, N):
    """the product of k_ckks_decode_start, the DIF passes and k_ckks_gather on the doubles v [batch][N] (coefficient over
    scale) -> slots [batch][N/2] complex128"""
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    roots, tw, pos1, _ = ckks_tables_np(N)
    re, im = v * tw[0], -v * tw[1]
    h = N // 2
    while h >= 1:
        _fft_pass_np(re, im, roots, N, h, 1, 0)
        h >>= 1
    return re[:, pos1] + 1j * im[:, pos1]


def ckks_passes_np(x, N, decode=False):
    return ckks_decode_passes_np(x, N) if decode else ckks_encode_passes_np(x, N)


# ----------------------------------------------------------------------------------------------------------------------
# what tests/test_gpu_ckks_exact.py and tests/test_exact_ref_cpu.py share: inputs, the error unit, the constant K
# ----------------------------------------------------------------------------------------------------------------------
CKKS_KINDS = ("random", "onehot", "alternating", "mixed")
CKKS_FULL_SIZES = (4, 8, 16, 64, 256, 1 << 10, 1 << 12, 1 << 13)
CKKS_SAMPLED_SIZES = (1 << 15, 1 << 16, 1 << 17)
K_FACTOR = 4          # fp contraction and the sinl / cosl tables change single roundings, not the order of the error


@functools.lru_cache(maxsize=None)
def ckks_slots_input(kind, N):
    """[3][N/2] complex128"""
    n2 = N // 2
    rng = np.random.default_rng([N, CKKS_KINDS.index(kind)])
    if kind == "random":
        z = rng.normal(size=(3, n2)) * 3 + 1j * rng.normal(size=(3, n2))
    elif kind == "onehot":                       # one slot set, the rest 0: every twiddle is driven by one value
        z = np.zeros((3, n2), dtype=np.complex128)
        z[0, 0], z[1, n2 // 2], z[2, n2 - 1] = 1.0, -2.5 + 0.75j, 1j * np.pi
    elif kind == "alternating":
        s = (-1.0) ** np.arange(n2)
        z = np.stack([s + 0j, -1j * s, s * (1 - 1j)])
    else:                                        # magnitudes 2^+-30 mixed: cancellation
        z = (rng.normal(size=(3, n2)) + 1j * rng.normal(size=(3, n2))) * 2.0 ** rng.choice([-30, 30], size=(3, n2))
    z = np.ascontiguousarray(z, dtype=np.complex128)
    z.setflags(write=False)
    return z


def sampled_positions(N, count=32):
    """count positions below N, always 0, 1, N/2 and N - 1"""
    rng = np.random.default_rng(N + 1)
    out = [0, 1, N // 2, N - 1]
    while len(out) < count:
        k = int(rng.integers(0, N))
        if k not in out:
            out.append(k)
    return out


def encode_unit(slots_row, N):
    """eps log2(N) ||cm||_2 / N for one slot vector (||cm||_2 = sqrt(2) ||slots||_2)"""
    return EPS * np.log2(N) * float(np.sqrt(2.0) * np.linalg.norm(slots_row)) / N


def decode_unit(v_norm2, N):
    """eps log2(N) ||v||_2"""
    return EPS * np.log2(N) * float(v_norm2)


@functools.lru_cache(maxsize=None)
def exact_coeffs(kind, N):
    """[3] lists of mpf: whole polynomials at the full sizes, {k: X_k} over sampled_positions at the sampled ones"""
    z = ckks_slots_input(kind, N)
    if N in CKKS_FULL_SIZES:
        return [ckks_coeffs_exact(z[b], N) for b in range(3)]
    ks = sampled_positions(N)
    out = []
    for b in range(3):
        mine = ks[:4] + ks[4 + b:24:3]           # 32 in all: the four fixed positions in every polynomial, 20 more shared out
        out.append(dict(zip(mine, ckks_coeffs_exact_some(z[b], N, mine))))
    return out


FIXED_P = 256


@functools.lru_cache(maxsize=None)
def exact_coeffs_fixed(kind, N):
    """exact_coeffs as integers: [3] pairs (positions k, object array floor(X_k 2^FIXED_P)), for vectorised exact comparisons"""
    out = []
    for ex in exact_coeffs(kind, N):
        ks = sorted(ex) if isinstance(ex, dict) else list(range(N))
        out.append((np.array(ks), np.array([int(MP.floor(MP.ldexp(ex[k], FIXED_P))) for k in ks], dtype=object)))
    return out


@functools.lru_cache(maxsize=None)
def encode_ratio_np(kind, N):
    """largest |x_k(numpy passes) - X_k| in units of encode_unit, over the batch"""
    z = ckks_slots_input(kind, N)
    x = ckks_encode_passes_np(z, N)
    ex = exact_coeffs(kind, N)
    worst = 0.0
    for b in range(3):
        items = ex[b].items() if isinstance(ex[b], dict) else enumerate(ex[b])
        err = max(abs(mpf(float(x[b, k])) - X) for k, X in items)
        worst = max(worst, float(err) / encode_unit(z[b], N))
    return worst


def crt_centred(residues, qs):
    """[L][N] uint64 residues -> object array [N] of the centred integers (n > Q // 2 => n - Q, ckks.jl:54-56)"""
    Q = 1
    for q in qs:
        Q *= int(q)
    acc = np.zeros(residues.shape[-1], dtype=object)
    for l, q in enumerate(qs):
        m = Q // int(q)
        acc = acc + residues[l].astype(object) * (m * pow(m, -1, int(q)))
    acc = acc % Q
    return np.where(acc > Q // 2, acc - Q, acc)


@functools.lru_cache(maxsize=None)
def decode_input(N, qs):
    """uniform residues [3][L][N] (qs a tuple) and their centred integers [3][N]"""
    rng = np.random.default_rng([N, len(qs), 77])
    res = np.stack([np.stack([rng.integers(0, int(q), size=N, dtype=np.uint64) for q in qs]) for _ in range(3)])
    res.setflags(write=False)
    return res, [crt_centred(res[b], qs) for b in range(3)]


@functools.lru_cache(maxsize=None)
def exact_slot_sums(N, qs):
    """the decoding of decode_input(N, qs) at scale 1: [3] lists of mpc (full sizes) or {i: slot_i} (sampled sizes); the
    decoding at another scale is this over the scale"""
    _, ints = decode_input(N, qs)
    if N in CKKS_FULL_SIZES:
        return [ckks_slots_exact(ints[b], 1, N) for b in range(3)]
    pos = sampled_positions(N // 2)
    out = []
    for b in range(3):
        mine = pos[:4] + pos[4 + b:24:3]
        out.append(dict(zip(mine, ckks_slots_exact_some(ints[b], 1, N, mine))))
    return out


def decode_values(ints_row, scale):
    """the doubles a correctly rounded ckks_words_to_double hands to the transform: float(n / scale)"""
    s = Fraction(scale)
    return np.array([float(Fraction(int(n)) / s) for n in ints_row], dtype=np.float64)


def decode_ratio_np(N, qs, scale):
    """largest |slot(numpy passes) - exact| in units of decode_unit over the batch"""
    _, ints = decode_input(N, qs)
    sums = exact_slot_sums(N, qs)
    s = Fraction(scale)
    inv = mpf(s.denominator) / mpf(s.numerator)
    worst = 0.0
    for b in range(3):
        v = decode_values(ints[b], scale)
        got = ckks_decode_passes_np(v, N)[0]
        items = sums[b].items() if isinstance(sums[b], dict) else enumerate(sums[b])
        err = max(abs(mpc(complex(got[i])) - S * inv) for i, S in items)
        worst = max(worst, float(err) / decode_unit(np.linalg.norm(v), N))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# what tests/test_gpu_gaussian_exact.py and tests/test_exact_ref_cpu.py share
# ----------------------------------------------------------------------------------------------------------------------
GAUSS_SEED = 0x1234567890ABCDEF
GAUSS_SIGMAS = (0.5, 3.2, 19.2, 3.2 * 2.0 ** 20, 2.0 ** 40, 1e15)
GAUSS_MARGIN = 2.0 ** -44          # |e - y| <= 1/2 + sigma 2^-44: the inexact steps of sample_gauss_int are the argument 2 pi u2
                                   # (absolute error <= 2 pi 2^-52), cos, log, sqrt and two products; with |z| <= 8.6 they sum to
                                   # below 2e-14 in z, and 2^-44 = 5.7e-14
GAUSS_EXACT_SIGMA_MAX = 2.0 ** 21  # up to here (and at 3.2 2^20, which the cap below was checked for as well) the rule and the cap
                                   # together mean e == rint(y) with no exception
GAUSS_SUBSET = 4096


def gauss_exact_form(sigma):
    return sigma <= GAUSS_EXACT_SIGMA_MAX or sigma == 3.2 * 2.0 ** 20


def gauss_cases(N):
    """(sigma, stream, first_poly, count): every sigma on stream 1 from polynomial 5, then stream 9, then the last polynomials
    before 2^32 (the high counter word all ones).  8 polynomials at N = 4096; 64 at N = 64, so that 4096 draws exist"""
    count = 8 if N >= 512 else GAUSS_SUBSET // N
    out = [(s, 1, 5, count) for s in GAUSS_SIGMAS]
    out += [(3.2, 9, 5, count), (3.2, 1, 2 ** 32 - count, count), (1e15, 9, 2 ** 32 - count, count)]
    return out


def gauss_subset(N, count):
    """the fixed positions (flat, sorted) of a [count][N] draw that go to mpmath whatever numpy says"""
    tot = count * N
    if tot <= GAUSS_SUBSET:
        return np.arange(tot)
    return np.sort(np.random.default_rng(tot).choice(tot, GAUSS_SUBSET, replace=False))


CHI_SEED, CHI_STREAM, CHI_FIRST, CHI_POLYS, CHI_N, CHI_SIGMA = 0x0DDBA11C0FFEE, 3, 1000, 256, 4096, 3.2


@functools.lru_cache(maxsize=None)
def gauss_bins(sigma, n):
    """integer bins lo .. hi with both tails merged into the end bins until every expected count is >= 20:
    (lo, hi, expected counts [hi - lo + 1]) from Phi((k + 1/2) / sigma) - Phi((k - 1/2) / sigma)"""
    def p(k):
        return MP.ncdf((k + mpf(0.5)) / mpf(sigma)) - MP.ncdf((k - mpf(0.5)) / mpf(sigma))
    hi = 0
    while n * (1 - MP.ncdf((hi + 1 - mpf(0.5)) / mpf(sigma))) >= 20:      # the merged tail [hi + 1, inf) still holds 20
        hi += 1
    # bins -hi .. hi; the end bins take the whole tail beyond them
    exp = [float(n * p(k)) for k in range(-hi, hi + 1)]
    tail = float(n * (1 - MP.ncdf((hi + mpf(0.5)) / mpf(sigma))))
    exp[0] += tail
    exp[-1] += tail
    assert min(exp) >= 20
    return -hi, hi, np.array(exp)


def chi_square_gauss(e, sigma):
    """(statistic, threshold dof + 6 sqrt(2 dof)) of integer draws e against the rounded Gaussian"""
    e = np.asarray(e).ravel()
    lo, hi, exp = gauss_bins(float(sigma), e.size)
    obs = np.bincount(np.clip(e, lo, hi) - lo, minlength=hi - lo + 1)
    dof = exp.size - 1
    return float(((obs - exp) ** 2 / exp).sum()), dof + 6 * np.sqrt(2 * dof)


def neighbour_correlation(e):
    """empirical correlation of e [polys][N] with the e of counter + 1 (the next coefficient of the same polynomial)"""
    a, b = e[:, :-1].ravel().astype(np.float64), e[:, 1:].ravel().astype(np.float64)
    return float(np.corrcoef(a, b)[0, 1]), a.size


# the scales of tests/test_gpu_ckks_exact.py (b): (label, scale, bits and count of the limbs it runs on)
CKKS_SCALES = (("2^40", Fraction(2 ** 40), 50, 2), ("12345*2^20", Fraction(12345 * 2 ** 20), 50, 2),
               ("2^80", Fraction(2 ** 80), 40, 3), ("10^12/7", Fraction(10 ** 12, 7), 50, 2))


def words_to_double_np(ints_row, mant, exp2):
    """ckks_words_to_double restated: the magnitude rounded once to 53 bits (ties to even), divided by the mantissa of the
    scale when that is not 1, scaled by the power of two"""
    d, sh = np.empty(len(ints_row)), np.zeros(len(ints_row), dtype=np.int64)
    for i, n in enumerate(int(v) for v in ints_row):
        m = abs(n)
        s = max(0, m.bit_length() - 64)                                    # the top 64 bits and a sticky bit, as the kernel takes them
        top = (m >> s) | (1 if m & ((1 << s) - 1) else 0)
        d[i], sh[i] = (-float(top) if n < 0 else float(top)), s            # int -> float rounds to nearest even
    if mant != 1:
        d = d / float(mant)
    return np.ldexp(d, sh - exp2)


def decode_ratio_parts_np(N, qs, mant, exp2):
    """decode_ratio_np with the device's own conversion of the integers (scale = mant 2^exp2)"""
    _, ints = decode_input(N, qs)
    sums = exact_slot_sums(N, qs)
    s = Fraction(mant) * Fraction(2) ** exp2
    inv = mpf(s.denominator) / mpf(s.numerator)
    worst = 0.0
    for b in range(3):
        v = words_to_double_np(ints[b], mant, exp2)
        got = ckks_decode_passes_np(v, N)[0]
        items = sums[b].items() if isinstance(sums[b], dict) else enumerate(sums[b])
        err = max(abs(mpc(complex(got[i])) - S * inv) for i, S in items)
        worst = max(worst, float(err) / decode_unit(np.linalg.norm(v), N))
    return worst
