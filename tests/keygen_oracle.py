"""The oracle's statement of tfhe_evalkey_gen (rlwe_she.jl:155-166, 273-304; modulusraising.jl:28-32) on residues, built from the C
oracle's transforms, limb-wise products and coefficient-domain automorphism (oracle/ref_cpu.py) and from the stream definition
of oracle/spec.py: shared by tests/test_keygen_cpu.py and tests/test_gpu_keygen.py.

    evk_k[i][0][j] = NTT_j(a_m)
    evk_k[i][1][j] = gamma[i][j] old_k[j] - ( NTT_j(a_m) s^[j] + NTT_j(mult_e e_m) ),      m = k n_digits + i

old_k is a given NTT-domain row, s^ s^ (galois 0), or NTT(sigma_g(INTT(s^))) -- the automorphism applied in the COEFFICIENT domain,
where it is the signed permutation of pow2_cyc_rings.jl:321-329, not the index permutation the kernels use."""
import numpy as np

from oracle import spec
from tests.enc_oracle import small_residues


def rns_gadget(qs, special=False):
    """gamma[i][j] = (i == j) (crt.jl:64-77), times the special prime P = qs[-1] under ModulusRaised: its row and column are zero"""
    P = int(qs[-1]) if special else 1
    return [[(P % int(q)) if i == j else 0 for j, q in enumerate(qs)] for i in range(len(qs))]


def window_gadget(qs, w, special=False):
    """gamma[i][j] = (2^(i w) mod Q) mod q_j (rlwe_she.jl:281-283), Q the product of qs; under ModulusRaised P 2^(i w) mod Q"""
    Q = 1
    for q in qs:
        Q *= int(q)
    P = int(qs[-1]) if special else 1
    n = -(-Q.bit_length() // w)
    return [[(P * pow(2, i * w, Q) % Q) % int(q) for q in qs] for i in range(n)]


def old_rows(ref, s_ntt, galois):
    """[K][L][N]: s^ s^ where galois[k] == 0, else the NTT image of the secret under x -> x^g"""
    s1 = np.ascontiguousarray(s_ntt[None])
    out = []
    for g in galois:
        out.append(ref.pointwise("mul", s1, s1)[0] if int(g) == 0 else ref.nntt(ref.galois(int(g), ref.inntt(s1)))[0])
    return np.stack(out)


def evalkey_ref(ref, s_ntt, mask, noise, mult_e, gadget=None, old=None, galois=None):
    """s_ntt [L][N] (NTT domain); mask [K][D][L][N] canonical residues, coefficient domain; noise int [K][D][N];
    gadget [D][L] residues or None (the public-key form); old [K][L][N] (NTT domain) or None with galois [K] -> [K][D][2][L][N]"""
    qs, N = ref.qs, ref.N
    K, D, L = mask.shape[:3]
    assert L == len(qs) and noise.shape == (K, D, N)
    ah = ref.nntt(np.ascontiguousarray(mask).reshape(K * D, L, N)).reshape(K, D, L, N)
    eh = ref.nntt(small_residues(np.asarray(noise).reshape(K * D, N), mult_e, qs)).reshape(K, D, L, N)
    if gadget is not None and old is None:
        old = old_rows(ref, s_ntt, galois)
    out = np.empty((K, D, 2, L, N), dtype=np.uint64)
    s1 = np.ascontiguousarray(s_ntt[None])
    for k in range(K):
        for i in range(D):
            a, e = np.ascontiguousarray(ah[k, i][None]), np.ascontiguousarray(eh[k, i][None])
            r = ref.pointwise("neg", ref.pointwise("add", ref.pointwise("mul", a, s1), e))
            if gadget is not None:
                r = ref.pointwise("add", r, ref.scalar_mul([int(x) for x in gadget[i]], np.ascontiguousarray(old[k][None])))
            out[k, i, 0], out[k, i, 1] = a[0], r[0]
    return out


def stream_uniform(qs, N, seed, stream, poly, coeffs=None):
    """polynomial `poly` of tfhe_sample_uniform's stream: [L][len(coeffs)] (coeffs None: all N)"""
    ks = range(N) if coeffs is None else coeffs
    return np.array([[spec.sample_uniform_mod((poly << 32) | k, l, stream, seed, int(q)) for k in ks] for l, q in enumerate(qs)], dtype=np.uint64)


def stream_gauss(N, seed, stream, poly, sigma, coeffs=None):
    """polynomial `poly` of tfhe_sample_gaussian's stream as signed integers (libm against the device's: equal up to rounding ties)"""
    ks = range(N) if coeffs is None else coeffs
    return np.array([spec.sample_gauss_int((poly << 32) | k, stream, seed, sigma) for k in ks], dtype=np.int64)
