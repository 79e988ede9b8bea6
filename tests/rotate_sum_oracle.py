"""The oracle's statement of tfhe_rotate_sum and tfhe_matmul_bsgs_fold on residues, built on tests/matmul_oracle.py (the C oracle's
Galois map and key switch, MO.rotate; MO.matmul_bsgs_blocks_ref) with exact Python-integer sums, reduced once per group:

    F_0 = ct;   F_{t+1} = F_t + sum_{u < len(groups[t])} rotate(key_{t,u}, F_t);   rotate_sum = F_{len(groups)}
    matmul_bsgs_fold = rotate_sum( matmul_bsgs_blocks(bias = None) ) + bias on component 0

Operands as in tests/matmul_oracle.py: PLAIN (unprepared) keys [n_digits][2][Lk][N] in the NTT domain, ciphertexts
[batch][2][level][N] and the bias [level][N] in the coefficient domain; `ref` is the RefCtx of the key ring.  `evk_groups` / `g_groups`
are lists of lists, one list per fold step."""
import numpy as np

from tests import matmul_oracle as MO


def rotate_sum_ref(ref, level, special, evk_groups, g_groups, ct):
    """tfhe_rotate_sum: [batch][2][level][N], coefficient domain"""
    assert [len(x) for x in evk_groups] == [len(x) for x in g_groups]
    q = MO._moduli(ref, level)
    f = np.ascontiguousarray(ct, dtype=np.uint64)
    for evks, gs in zip(evk_groups, g_groups):
        assert len(evks) >= 1
        total = f.astype(object)
        for evk, g in zip(evks, gs):
            total = total + MO.rotate(ref, level, special, evk, g, f).astype(object)
        f = (total % q).astype(np.uint64)
    return f


def matmul_bsgs_fold_ref(ref, level, special, baby_evks, baby_gs, giant_evks, giant_gs, diags, cts, fold_evk_groups, fold_g_groups, bias=None):
    """tfhe_matmul_bsgs_fold: the bias is added after the fold"""
    f = MO.matmul_bsgs_blocks_ref(ref, level, special, baby_evks, baby_gs, giant_evks, giant_gs, diags, cts, None)
    total = rotate_sum_ref(ref, level, special, fold_evk_groups, fold_g_groups, f).astype(object)
    if bias is not None:
        total[:, 0] = total[:, 0] + np.asarray(bias).astype(object)[None]
    return (total % MO._moduli(ref, level)).astype(np.uint64)
