"""The oracle's statement of tfhe_dot_plain -- dst_i = (acc_i +) sum_k T_k(a[k]_i) .* b[k]_i, T_k the forward transform or the
identity -- on residues: the C oracle's transform (oracle/ref_cpu.py) and exact integer arithmetic on Python integers (the
products are summed unreduced and reduced once).  Shared by tests/test_dot_plain_cpu.py and tests/test_gpu_dot_plain.py."""
import numpy as np


def dot_plain_ref(ref, acc, a, a_ntt, b, idx=None):
    """ref: RefCtx of the context's ring; idx: the context moduli of the buffer limbs (None: the first ones).
    acc: None or [count][limbs][N]; a: list of [count][limbs][N] (slices of packed arrays are fine); a_ntt: list of flags;
    b: list of [count][limbs][N] or [limbs][N] (one plaintext for the whole batch).  Returns [count][limbs][N] uint64."""
    assert len(a) == len(a_ntt) == len(b) and len(a) >= 1
    count, limbs, N = a[0].shape
    idx = list(range(limbs)) if idx is None else list(idx)
    assert len(idx) == limbs
    qs = np.array([ref.qs[j] for j in idx], dtype=object).reshape(1, limbs, 1)
    total = np.zeros((count, limbs, N), dtype=object) if acc is None else np.asarray(acc).astype(object)
    for x, flag, p in zip(a, a_ntt, b):
        x = np.ascontiguousarray(x, dtype=np.uint64)
        assert x.shape == (count, limbs, N)
        img = x if flag else ref.nntt(x, idx)
        p = np.asarray(p)
        total = total + img.astype(object) * (p[None] if p.ndim == 2 else p).astype(object)
    return (total % qs).astype(np.uint64)
