"""The oracle's statement of the hoisted rotations and the diagonal product on grouped-digit keys -- tfhe_rotate_many_grouped and
tfhe_matmul_diag_grouped -- on residues.  Nothing is hoisted here: every rotation is tests/ks_grouped_oracle.rotate_grouped_ref (the
C oracle's Galois map, then the grouped key switch of the rotated copy), and the product adds the C oracle's forward transform and an
exact sum over Python integers, reduced once, as tests/matmul_oracle.matmul_diag_ref does for the per-limb product.

    out[r] = rotate_grouped(key_r, g_r, ct)                                                  [n_rot][batch][2][level][N], coefficient domain
    out    = diags[0] (.) NTT(ct) + sum_r diags[r + 1] (.) NTT(rotate_grouped(key_r, g_r, ct))   [batch][2][level][N], NTT domain

Operands are what the raw C ABI takes, except that the keys are the PLAIN (unprepared) ones -- the device gets them through
tfhe_galois_key_prepare: keys [n_digits][2][Lk][N] in the NTT domain, diagonals [n_rot + 1][level][N] in the NTT domain, ciphertexts
[batch][2][level][N] in the coefficient domain.  `ref` is the RefCtx of the KEY ring (Lk limbs, the k special primes last).  Shared by
tests/test_gpu_rotate_many_grouped.py and tools/bench_rotate_many_grouped.py."""
import numpy as np

from tests import ks_grouped_oracle as KO


def rotate_many_grouped_ref(ref, level, k, alpha, evks, gs, ct):
    """tfhe_rotate_many_grouped: [len(evks)][batch][2][level][N]; the same key array may appear more than once"""
    assert len(evks) == len(gs)
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    memo = {}
    out = np.empty((len(evks),) + ct.shape, dtype=np.uint64)
    for r, (evk, g) in enumerate(zip(evks, gs)):
        key = (id(evk), int(g))
        if key not in memo:
            memo[key] = KO.rotate_grouped_ref(ref, level, k, alpha, evk, int(g), ct)
        out[r] = memo[key]
    return out


def matmul_diag_grouped_ref(ref, level, k, alpha, evks, gs, diags, ct):
    """tfhe_matmul_diag_grouped: [batch][2][level][N], NTT domain"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    diags = np.asarray(diags)
    N = ref.N
    assert ct.shape[1:] == (2, level, N) and diags.shape == (len(evks) + 1, level, N)
    terms = [ct] + list(rotate_many_grouped_ref(ref, level, k, alpha, evks, gs, ct))
    total = 0
    for term, d in zip(terms, diags):
        img = ref.nntt(term.reshape(-1, level, N), idx=range(level)).reshape(ct.shape).astype(object)
        total = total + img * d.astype(object)[None, None]
    q = np.array([int(x) for x in ref.qs[:level]], dtype=object).reshape(1, 1, level, 1)
    return (total % q).astype(np.uint64)
