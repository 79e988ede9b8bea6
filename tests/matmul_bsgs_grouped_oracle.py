"""The oracle's statement of the product by baby and giant steps on grouped-digit keys -- tfhe_matmul_bsgs_grouped -- on residues, in the
shape of tests/matmul_oracle.matmul_bsgs_blocks_ref: every rotation is tests/ks_grouped_oracle.rotate_grouped_ref (the C oracle's
Galois map, then the grouped key switch of the rotated copy), the transforms are the C oracle's, and every sum is exact arithmetic on
Python integers, reduced once.

    inner_j = sum_m sum_{i = 0 .. n_baby} diags[m][j][i] (.) NTT(r_i(ct_m))        r_0 = identity, r_i = rotate_grouped(baby key i - 1, .)
    out     = INTT(inner_0) + sum_{j = 1 .. n_giant} rotate_grouped(giant key j - 1, INTT(inner_j))   (+ bias on component 0)

Operands are what the raw C ABI takes, except that the keys are the PLAIN (unprepared) ones -- the device gets them through
tfhe_galois_key_prepare: keys [n_digits][2][Lk][N] in the NTT domain, diagonals [n_in][n_giant + 1][n_baby + 1][level][N] in the NTT domain,
ciphertexts [batch][2][level][N] and the bias [level][N] in the coefficient domain.  `ref` is the RefCtx of the KEY ring (Lk limbs, the k
special primes last).  Shared by tests/test_matmul_bsgs_grouped_cpu.py, tests/test_gpu_matmul_bsgs_grouped.py and
tools/bench_matmul_bsgs_grouped.py."""
import numpy as np

from tests import ks_grouped_oracle as KO


def _moduli(ref, level):
    return np.array([int(q) for q in ref.qs[:level]], dtype=object).reshape(1, 1, level, 1)


def inner_sums_grouped(ref, level, k, alpha, baby_evks, baby_gs, diags, cts):
    """[n_giant + 1][batch][2][level][N], NTT domain: the exact integer sums over all inputs and baby steps, reduced once"""
    assert len(baby_evks) == len(baby_gs) and len(diags) == len(cts) >= 1
    N, idx = ref.N, range(level)
    ng1 = len(diags[0])
    total = [0] * ng1
    for m, ct in enumerate(cts):
        ct = np.ascontiguousarray(ct, dtype=np.uint64)
        assert ct.shape[1:] == (2, level, N) and np.shape(diags[m]) == (ng1, len(baby_gs) + 1, level, N)
        terms = [ct] + [KO.rotate_grouped_ref(ref, level, k, alpha, evk, int(g), ct) for evk, g in zip(baby_evks, baby_gs)]
        for i, term in enumerate(terms):
            img = ref.nntt(term.reshape(-1, level, N), idx=idx).reshape(ct.shape).astype(object)
            for j in range(ng1):
                total[j] = total[j] + img * np.asarray(diags[m][j][i]).astype(object)[None, None]
    q = _moduli(ref, level)
    return np.stack([(t % q).astype(np.uint64) for t in total])


def matmul_bsgs_blocks_grouped_ref(ref, level, k, alpha, baby_evks, baby_gs, giant_evks, giant_gs, diags, cts, bias=None):
    """tfhe_matmul_bsgs_grouped: [batch][2][level][N], coefficient domain"""
    assert len(giant_evks) == len(giant_gs) == len(diags[0]) - 1
    N, idx = ref.N, range(level)
    inner = inner_sums_grouped(ref, level, k, alpha, baby_evks, baby_gs, diags, cts)
    parts = ref.inntt(inner.reshape(-1, level, N), idx=idx).reshape(inner.shape)
    total = parts[0].astype(object)
    for j, (evk, g) in enumerate(zip(giant_evks, giant_gs)):
        total = total + KO.rotate_grouped_ref(ref, level, k, alpha, evk, int(g), parts[j + 1]).astype(object)
    if bias is not None:
        total[:, 0] = total[:, 0] + np.asarray(bias).astype(object)[None]
    return (total % _moduli(ref, level)).astype(np.uint64)
