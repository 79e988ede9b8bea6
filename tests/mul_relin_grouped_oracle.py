"""The oracle's statement of tfhe_mul_relin_grouped on residues: the chain through the public entry points,

    tfhe_nntt x2 (skipped with ntt_in) -> tfhe_tensor -> tfhe_inntt -> tfhe_keyswitch_grouped(polys = 3) [-> tfhe_rescale],

from the C oracle's transforms, tensor and rescale (oracle/ref_cpu.py RefCtx.inntt / enc_mul / modswitch) and the grouped key switch
of tests/ks_grouped_oracle.py.  The forward transform is a bijection on canonical residues, so operands that arrive as NTT images are
taken back to the coefficient domain first and the product is the same one.

Operands are what the raw C ABI takes: evk [n_digits][2][Lk][N] in the NTT domain, c1 / c2 [batch][2][level][N] (the NTT images with
ntt_in), the result [batch][2][level - rescale][N] in the coefficient domain.  Shared by tests/test_gpu_mul_relin_grouped.py and
tools/bench_mul_relin_grouped.py."""
import numpy as np

from tests import ks_grouped_oracle as KO


def product_ref(ref, level, c1, c2, ntt_in=False):
    """c1 * c2 as a 3-element ciphertext [batch][3][level][N], coefficient domain (rlwe_she.jl:247-262 without expand / contract)"""
    idx = list(range(level))
    c1, c2 = (np.ascontiguousarray(c, dtype=np.uint64) for c in (c1, c2))
    assert c1.shape == c2.shape and c1.shape[1:] == (2, level, ref.N)
    if ntt_in:
        c1, c2 = (ref.inntt(c.reshape(-1, level, ref.N), idx=idx).reshape(c.shape) for c in (c1, c2))
    return ref.enc_mul(c1, c2, idx=idx)


def rescale_ref(ref, level, ct):
    """tfhe_rescale of both components: [batch][2][level][N] -> [batch][2][level - 1][N] (crt.jl:215-228)"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    return ref.modswitch(ct.reshape(-1, level, ref.N), idx=list(range(level))).reshape(ct.shape[0], 2, level - 1, ref.N)


def mul_relin_grouped_ref(ref, level, k, alpha, evk, c1, c2, ntt_in=False, rescale=False):
    """tfhe_mul_relin_grouped; `ref` is the RefCtx of the KEY ring (the special primes last).  alpha above level: one digit."""
    ks = KO.keyswitch_grouped_ref(ref, level, k, min(alpha, level), evk, product_ref(ref, level, c1, c2, ntt_in))
    return rescale_ref(ref, level, ks) if rescale else ks
