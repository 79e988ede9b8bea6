"""The oracle's statement of tfhe_rotate_sum_grouped and tfhe_matmul_bsgs_fold_grouped on residues, composed step by step from
tests/ks_grouped_oracle.rotate_grouped_ref and modular addition, and from tests/matmul_bsgs_grouped_oracle.py:

    F_0 = ct;   F_{t+1} = F_t + sum_{u < len(steps[t])} rotate_grouped(key_{t,u}, F_t);   rotate_sum_grouped = F_{len(steps)}
    matmul_bsgs_fold_grouped = rotate_sum_grouped( matmul_bsgs_blocks_grouped(bias = None) ) + bias on component 0

Operands as in tests/matmul_bsgs_grouped_oracle.py: PLAIN (unprepared) grouped keys [n_digits][2][Lk][N] in the NTT domain, ciphertexts
[batch][2][level][N] and the bias [level][N] in the coefficient domain; `ref` is the RefCtx of the key ring (the k special primes
last); alpha: limbs per digit.  `evk_steps` / `g_steps` are lists of lists, one list per fold step."""
import numpy as np

from tests import ks_grouped_oracle as KO
from tests import matmul_bsgs_grouped_oracle as BO


def rotate_sum_grouped_ref(ref, level, k, alpha, evk_steps, g_steps, ct):
    """tfhe_rotate_sum_grouped: [batch][2][level][N], coefficient domain"""
    assert [len(x) for x in evk_steps] == [len(x) for x in g_steps]
    q = BO._moduli(ref, level)
    f = np.ascontiguousarray(ct, dtype=np.uint64)
    for evks, gs in zip(evk_steps, g_steps):
        assert len(evks) >= 1
        total = f.astype(object)
        for evk, g in zip(evks, gs):
            total = total + KO.rotate_grouped_ref(ref, level, k, alpha, evk, g, f).astype(object)
        f = (total % q).astype(np.uint64)
    return f


def matmul_bsgs_fold_grouped_ref(ref, level, k, alpha, baby_evks, baby_gs, giant_evks, giant_gs, diags, cts, fold_evk_steps, fold_g_steps, bias=None):
    """tfhe_matmul_bsgs_fold_grouped: the bias is added after the fold"""
    f = BO.matmul_bsgs_blocks_grouped_ref(ref, level, k, alpha, baby_evks, baby_gs, giant_evks, giant_gs, diags, cts, bias=None)
    total = rotate_sum_grouped_ref(ref, level, k, alpha, fold_evk_steps, fold_g_steps, f).astype(object)
    if bias is not None:
        total[:, 0] = total[:, 0] + np.asarray(bias).astype(object)[None]
    return (total % BO._moduli(ref, level)).astype(np.uint64)
