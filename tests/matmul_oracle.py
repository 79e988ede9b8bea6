"""The oracle's statement of the three diagonal products -- tfhe_matmul_diag, tfhe_matmul_bsgs, tfhe_matmul_bsgs_blocks -- on residues:
the C oracle's Galois map, key switch and transforms (oracle/ref_cpu.py RefCtx.galois / keyswitch / nntt / inntt) and exact integer
arithmetic on Python integers for every sum (the products are summed unreduced and reduced once; RefCtx.pointwise is not used).

    inner_j = sum_m sum_{i = 0 .. n_baby} diags[m][j][i] (.) NTT(r_i(ct_m))        r_0 = identity, r_i = rotate(baby key i - 1, .)
    out     = INTT(inner_0) + sum_{j = 1 .. n_giant} rotate(giant key j - 1, INTT(inner_j))   (+ bias on component 0)

Operands are what the raw C ABI takes, except that the keys are the PLAIN (unprepared) ones -- the device gets them through
tfhe_galois_key_prepare: keys [n_digits][2][Lk][N] in the NTT domain (tests/helpers.py uniform_evk), diagonals [n_in][n_giant + 1][n_baby + 1]
[level][N] in the NTT domain, ciphertexts [batch][2][level][N] and the bias [level][N] in the coefficient domain.  `ref` is the RefCtx of the
KEY ring (Lk limbs, the special prime last).  Shared by tests/test_matmul_oracle_cpu.py (which pins it to oracle/spec.py),
tests/test_gpu_matmul_oracle.py, tests/test_gpu_chunk_seams.py and tools/fuzz_matmul.py."""
import numpy as np


def rotate(ref, level, special, evk, g, ct):
    """keyswitch(evk, galois(g, ct)): ct [batch][2][level][N] coefficient domain -> the same shape"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    return ref.keyswitch(level, special, evk, ref.galois(g, ct.reshape(-1, level, ref.N), idx=range(level)).reshape(ct.shape))


def _moduli(ref, level):
    return np.array([int(q) for q in ref.qs[:level]], dtype=object).reshape(1, 1, level, 1)


def inner_sums(ref, level, special, baby_evks, baby_gs, diags, cts):
    """[n_giant + 1][batch][2][level][N], NTT domain: the exact integer sums over all inputs and baby steps, reduced once"""
    assert len(baby_evks) == len(baby_gs) and len(diags) == len(cts) >= 1
    N, idx = ref.N, range(level)
    ng1 = len(diags[0])
    total = [0] * ng1
    for m, ct in enumerate(cts):
        ct = np.ascontiguousarray(ct, dtype=np.uint64)
        assert ct.shape[1:] == (2, level, N) and np.shape(diags[m]) == (ng1, len(baby_gs) + 1, level, N)
        terms = [ct] + [rotate(ref, level, special, evk, g, ct) for evk, g in zip(baby_evks, baby_gs)]
        for i, term in enumerate(terms):
            img = ref.nntt(term.reshape(-1, level, N), idx=idx).reshape(ct.shape).astype(object)
            for j in range(ng1):
                total[j] = total[j] + img * np.asarray(diags[m][j][i]).astype(object)[None, None]
    q = _moduli(ref, level)
    return np.stack([(t % q).astype(np.uint64) for t in total])


def matmul_bsgs_blocks_ref(ref, level, special, baby_evks, baby_gs, giant_evks, giant_gs, diags, cts, bias=None):
    """tfhe_matmul_bsgs_blocks: [batch][2][level][N], coefficient domain"""
    assert len(giant_evks) == len(giant_gs) == len(diags[0]) - 1
    N, idx = ref.N, range(level)
    inner = inner_sums(ref, level, special, baby_evks, baby_gs, diags, cts)
    parts = ref.inntt(inner.reshape(-1, level, N), idx=idx).reshape(inner.shape)
    total = parts[0].astype(object)
    for j, (evk, g) in enumerate(zip(giant_evks, giant_gs)):
        total = total + rotate(ref, level, special, evk, g, parts[j + 1]).astype(object)
    if bias is not None:
        total[:, 0] = total[:, 0] + np.asarray(bias).astype(object)[None]
    return (total % _moduli(ref, level)).astype(np.uint64)


def matmul_bsgs_ref(ref, level, special, baby_evks, baby_gs, giant_evks, giant_gs, diags, ct):
    """tfhe_matmul_bsgs: one input (diags [n_giant + 1][n_baby + 1][level][N]), no bias"""
    return matmul_bsgs_blocks_ref(ref, level, special, baby_evks, baby_gs, giant_evks, giant_gs, [diags], [ct])


def matmul_diag_ref(ref, level, special, evks, gs, diags, ct):
    """tfhe_matmul_diag: no giant step (diags [n_rot + 1][level][N]) and no closing inverse transform -- inner_0, NTT domain"""
    return inner_sums(ref, level, special, evks, gs, [np.asarray(diags)[None]], [ct])[0]
