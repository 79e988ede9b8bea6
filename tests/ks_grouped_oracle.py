"""The oracle's statement of the key switch with grouped RNS digits and several special primes -- tfhe_keyswitch_grouped and
tfhe_rotate_grouped -- on residues: the C oracle's transforms, contraction and Galois map (oracle/ref_cpu.py RefCtx.nntt / inntt /
modswitch / galois) and exact arithmetic on Python integers for the CRT reconstruction, the centred lift and the key sums (summed
unreduced and reduced once; RefCtx.pointwise is not used).

    key ring: limbs 0 .. Lk-1 of `ref`, the last k of them special primes;  ciphertext ring: limbs 0 .. level-1, level <= Lk - k
    W = [0 .. level-1] + [Lk-k .. Lk-1];   digit g covers limbs [g alpha, min((g + 1) alpha, level)),  g < d = ceil(level / alpha)
    digit_g = centred(c[end] mod Q_g) reduced into every limb of W           (tie rule n > Q_g // 2  =>  n - Q_g, signedmod.jl:12-19)
    S_s     = sum_g key_{g,s} (.) NTT(digit_g) over W                        (s = 0: masked, s = 1: mask)
    out_s   = c_s + modswitch^k(INTT(S_s))                                   (the last special prime first; c_2 = 0 for a 2-element input)

Operands are what the raw C ABI takes: evk [n_digits][2][Lk][N] in the NTT domain (component 0 = mask, 1 = masked), ct
[batch][polys][level][N] and the result [batch][2][level][N] in the coefficient domain.  Shared by tests/test_ks_grouped_cpu.py
(which pins it to oracle/spec.py), tests/test_gpu_ks_grouped.py and tools/bench_keyswitch_grouped.py."""
import math

import numpy as np


def working_limbs(Lk, level, k):
    return list(range(level)) + list(range(Lk - k, Lk))


def groups(level, alpha):
    """the limb ranges of the digits at this level"""
    return [range(g * alpha, min((g + 1) * alpha, level)) for g in range(-(-level // alpha))]


def gadget_table(qs, k, alpha):
    """[d][Lk] residues of the grouped gadget at the key's own top level: row g holds P mod q_j at the limbs j of group g"""
    Lk = len(qs)
    top = Lk - k
    P = math.prod(int(q) for q in qs[top:])
    return [[P % int(qs[j]) if j in G else 0 for j in range(Lk)] for G in groups(top, alpha)]


def crt_ints(res, qs):
    """exact CRT of res [len(qs)][...] (object or uint64 arrays) into [0, prod qs), as an object array"""
    Q = math.prod(qs)
    x = 0
    for r, q in zip(res, qs):
        Qi = Q // q
        x = x + np.asarray(r).astype(object) * (Qi * pow(Qi, -1, q) % Q)
    return x % Q


def digits(qs, Lk, level, k, alpha, c_end):
    """c_end [batch][level][N] -> [batch][d][nw][N], coefficient domain"""
    W = working_limbs(Lk, level, k)
    c_end = np.asarray(c_end)
    out = np.empty((c_end.shape[0], len(groups(level, alpha)), len(W), c_end.shape[2]), dtype=np.uint64)
    for g, G in enumerate(groups(level, alpha)):
        gq = [int(qs[i]) for i in G]
        Qg = math.prod(gq)
        x = crt_ints([c_end[:, i] for i in G], gq)
        x = np.where((x > Qg // 2).astype(bool), x - Qg, x)
        for j, w in enumerate(W):
            out[:, g, j] = (x % int(qs[w])).astype(np.uint64)
    return out


def keyswitch_grouped_ref(ref, level, k, alpha, evk, ct):
    """tfhe_keyswitch_grouped; `ref` is the RefCtx of the KEY ring (the special primes last)"""
    Lk, N, qs = ref.L, ref.N, ref.qs
    W = working_limbs(Lk, level, k)
    nw = len(W)
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    evk = np.asarray(evk)
    batch, polys = ct.shape[0], ct.shape[1]
    assert polys in (2, 3) and ct.shape[2:] == (level, N) and evk.shape[1:] == (2, Lk, N)
    dig = digits(qs, Lk, level, k, alpha, ct[:, -1])
    d = dig.shape[1]
    assert evk.shape[0] >= d
    dn = ref.nntt(dig.reshape(-1, nw, N), idx=W).reshape(dig.shape).astype(object)
    qw = np.array([int(qs[w]) for w in W], dtype=object).reshape(1, nw, 1)
    S = np.empty((batch, 2, nw, N), dtype=np.uint64)
    for s in range(2):
        tot = 0
        for g in range(d):
            tot = tot + dn[:, g] * evk[g, 1 - s][W].astype(object)[None]
        S[:, s] = (tot % qw).astype(np.uint64)
    T = ref.inntt(S.reshape(-1, nw, N), idx=W)
    for t in range(k):
        T = ref.modswitch(T, idx=W[:nw - t])
    T = T.reshape(batch, 2, level, N).astype(object)
    for s in range(polys - 1):
        T[:, s] = T[:, s] + ct[:, s].astype(object)
    ql = np.array([int(q) for q in qs[:level]], dtype=object).reshape(1, 1, level, 1)
    return (T % ql).astype(np.uint64)


def rotate_grouped_ref(ref, level, k, alpha, evk, g, ct):
    """tfhe_rotate_grouped: keyswitch(evk, apply_galois_element(ct, g)), ct [batch][2][level][N]"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    rot = ref.galois(g, ct.reshape(-1, level, ref.N), idx=range(level)).reshape(ct.shape)
    return keyswitch_grouped_ref(ref, level, k, alpha, evk, rot)
