"""The oracle's statement of tfhe_encrypt / tfhe_decrypt_phase (rlwe_she.jl:176-216) on residues, built from the C oracle's
transforms and limb-wise products (oracle/ref_cpu.py): shared by tests/test_encrypt_cpu.py and tests/test_gpu_encrypt.py."""
import numpy as np


def small_residues(ints, mult, qs):
    """signed integers [..., N] -> residues of mult * e, [..., L, N]"""
    cols = [np.mod(ints.astype(object) * int(mult), int(q)).astype(np.uint64) for q in qs]
    return np.stack(cols, axis=ints.ndim - 1)


def _rows(ref, op, a, b):
    return ref.pointwise(op, a, np.ascontiguousarray(np.broadcast_to(b, a.shape)))


def encrypt_ref(ref, pk, rand, mult_e, msg=None):
    """pk [2][L][N] (mask, masked; NTT domain), rand int [B][3][N] (u, e1, e2), msg [B][L][N] or None -> [B][2][L][N]:
    (masked u + mult_e e1 (+ msg), mask u + mult_e e2), coefficient domain"""
    qs = ref.qs
    uh = ref.nntt(small_residues(rand[:, 0], 1, qs))
    out = np.empty((rand.shape[0], 2, len(qs), ref.N), dtype=np.uint64)
    for k in range(2):
        c = ref.inntt(_rows(ref, "mul", uh, pk[1 - k]))
        c = ref.pointwise("add", c, small_residues(rand[:, 1 + k], mult_e, qs))
        if k == 0 and msg is not None:
            c = ref.pointwise("add", c, msg)
        out[:, k] = c
    return out


def decrypt_ref(ref, s_ntt, ct, ntt_in=False):
    """s_ntt [L][N] (NTT domain), ct [B][P][L][N] -> c1 + s c2 (+ s^2 c3 ...) [B][L][N], coefficient domain"""
    B, P = ct.shape[:2]
    img = ct if ntt_in else np.stack([ref.nntt(ct[:, p]) for p in range(P)], axis=1)
    acc, spow = img[:, 0].copy(), s_ntt[None]
    for p in range(1, P):
        acc = ref.pointwise("add", acc, _rows(ref, "mul", np.ascontiguousarray(img[:, p]), spow))
        spow = ref.pointwise("mul", spow, s_ntt[None])
    return ref.inntt(acc)
