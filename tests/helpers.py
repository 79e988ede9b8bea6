"""Shared helpers for the parity tests: seeded inputs, evaluation keys (built with the spec/C oracle
on the host, like the Julia callers keygen/make_eval_key would), device round trips."""
import random

import numpy as np

from oracle import ref_cpu, spec


def chain(bits, n, N):
    return spec.prime_chain(2**bits + 1, n, N)


def rand_residues(rng: np.random.Generator, qs, shape_prefix, N):
    """uniform residues, layout [*shape_prefix][len(qs)][N]"""
    cols = [rng.integers(0, int(q), size=tuple(shape_prefix) + (N,), dtype=np.uint64) for q in qs]
    return np.stack(cols, axis=len(shape_prefix))


def uniform_evk(rng, qs, ndig, N):
    """an evaluation key with uniform components (throughput runs): [ndig][2][Lk][N], NTT domain"""
    return rand_residues(rng, qs, (ndig, 2), N)


def real_evk(seed, N, qs, special, sigma=3.2):
    """a genuine RNS-gadget key switching key for s^2 -> s via the fast C oracle NTT.
    Returns (secret [Lk][N] coefficient domain, evk [Lk][2][Lk][N] NTT domain)."""
    prng = random.Random(seed)
    rng = np.random.default_rng(seed)
    Lk = len(qs)
    ctx = ref_cpu.RefCtx(N, qs)
    s_int = spec.sample_gauss_ints(prng, N, sigma)
    secret = np.array([[x % q for x in s_int] for q in qs], dtype=np.uint64)
    s_ntt = ctx.nntt(secret[None])[0]
    s2_ntt = ctx.pointwise("mul", s_ntt[None], s_ntt[None])[0]
    s2 = ctx.inntt(s2_ntt[None])[0]
    premul = int(qs[-1]) if special else 1
    evk = np.empty((Lk, 2, Lk, N), dtype=np.uint64)
    for i in range(Lk):
        mask = rand_residues(rng, qs, (), N)
        e_int = spec.sample_gauss_ints(prng, N, sigma)
        e = np.array([[x % q for x in e_int] for q in qs], dtype=np.uint64)
        g = np.zeros((Lk, N), dtype=np.uint64)
        g[i] = (s2[i].astype(object) * (premul % int(qs[i])) % int(qs[i])).astype(np.uint64)
        m_ntt = ctx.nntt(mask[None])[0]
        ms = ctx.inntt(ctx.pointwise("mul", m_ntt[None], s_ntt[None]))[0]
        masked = ctx.pointwise("sub", g[None], ctx.pointwise("add", ms[None], e[None]))[0]
        evk[i, 0] = m_ntt
        evk[i, 1] = ctx.nntt(masked[None])[0]
    return secret, evk


# ---------------------------------------------------------------------------------------------------
# modulus size classes of the engine (each bound is read back out of the sources by tests/test_modulus_edges_cpu.py)
# ---------------------------------------------------------------------------------------------------
Q_LIMIT = 1 << 62                  # tfhe_ctx_create: every prime below 2^62
FP_QMAX = (1 << 50) + (1 << 40)    # fp64arith.h TFHE_FP_QMAX: fp64 transforms, narrow BFV conversions below it
FPS_QMAX = 1 << 42                 # fp64arith.h TFHE_FPS_QMAX: ArithFpS in k_ks_fused_sub when every working limb is below it
FOLD_BITS = 52                     # kernels.h k_ks_inner: high-word fold for moduli wider than 52 bits (acc52 forms up to 52)
KS_FOLD_LAZY_62 = 3                # kernels.h k_ks_inner: terms between two reductions at 62 bits (DCH up to 61 bits)
MIXED_MIN_WORDS = 1 << 20          # toyfhe_hip.hip TFHE_MIXED_MIN_WORDS: words before a mixed ring is split per policy


def sum_chunk(bits):
    """lazy_sum.h lazy_chunk (k_dot / k_lincomb / k_lincomb_many / k_dot_view / k_md_acc / k_md_acc_dense): products summed between two Barrett
    reductions, 2^(62 - bits(q)) capped at 64 (chunk (q - 1)^2 < 2^(bits + 62), the Barrett window)"""
    return 1 if bits >= 62 else min(64, 1 << (62 - bits))


def conv_lazy(bits, k):
    """bfv_tables.h lazy_of: exact-conversion products summed between two reductions"""
    return max(1, min(k, 1 << 20 if 62 - bits >= 20 else 1 << max(0, 62 - bits)))


def primes_below(bound, n, N):
    """the n largest NTT-friendly primes (q = 1 mod 2N) below `bound`, largest first"""
    q = (bound - 2) // (2 * N) * (2 * N) + 1
    out = []
    while len(out) < n:
        assert q > 2 * N, (bound, n, N)
        if spec.is_prime(q):
            out.append(q)
        q -= 2 * N
    return out


def primes_above(bound, n, N):
    """the n smallest NTT-friendly primes above `bound`, smallest first"""
    q = bound // (2 * N) * (2 * N) + 1
    q += 2 * N if q <= bound else 0
    out = []
    while len(out) < n:
        if spec.is_prime(q):
            out.append(q)
        q += 2 * N
    return out


def row_policy_cases():
    """(logn, q, fp) of the fused row kernels' body tests: the u64 policy at the largest prime below 2^62 and at a 53-bit prime,
    N = 2^12 and 2^14; the fp64 policy at the top of its class (the largest prime below TFHE_FP_QMAX), N = 2^12, 2^13, 2^14"""
    out = []
    for logn in (12, 14):
        N = 1 << logn
        out += [(logn, primes_below(Q_LIMIT, 1, N)[0], 0), (logn, primes_above(1 << 52, 1, N)[0], 0)]
    out += [(logn, primes_below(FP_QMAX, 1, 1 << logn)[0], 1) for logn in (12, 13, 14)]
    return out


def words_mod(rng, q, shape, edge):
    """random residues, or (edge) every word q - 1"""
    if edge:
        return np.full(shape, q - 1, dtype=np.uint64)
    return (rng.integers(0, 1 << 62, shape, dtype=np.uint64) % np.uint64(q)).astype(np.uint64)


def galois_pos(n, g):
    """the evaluation-domain gather of x -> x^g (modarith.h galois_ntt_pos): the position output k reads, for k < n"""
    k = np.arange(n, dtype=object)
    return np.array([int(((g * (2 * int(x) + 1) - 1) >> 1) & (n - 1)) for x in k])


def primes_above_ratio(k, bits, n, N):
    """the n smallest NTT-friendly primes above 2^64 / k, all of `bits` bits: there 2^64 mod q = 2^64 - (k - 1) q is
    close to q, the worst case of the high-word fold in k_ks_inner (z' = hi (2^64 mod q) + lo)"""
    out = primes_above((1 << 64) // k, n, N)
    assert all(q.bit_length() == bits for q in out), (k, bits, out)
    return out
