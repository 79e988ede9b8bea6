"""tests/matmul_oracle.py -- the host reference of tfhe_matmul_diag / tfhe_matmul_bsgs / tfhe_matmul_bsgs_blocks that
tests/test_gpu_matmul_oracle.py holds the device to -- pinned to oracle/spec.py: the same products built from spec.poly_nntt,
spec.keyswitch and the spec's Galois map on Python integers, word for word, at N = 16 on three small primes with and without the
special prime, 2 baby x 2 giant steps, two inputs and a bias."""
import numpy as np
import pytest

from oracle import ref_cpu, spec
from tests import helpers as H
from tests import matmul_oracle as MO

N, N_BABY, N_GIANT, N_IN, BATCH = 16, 2, 2, 2, 2


def _lists(a):
    """[L][N] words -> the spec's list of limb lists"""
    return [[int(v) for v in limb] for limb in a]


def _setup(special, seed):
    qs = H.chain(20, 3, N)                                                  # the first three primes = 1 mod 2N above 2^20
    Lk = len(qs)
    level = Lk - 1 if special else Lk
    keyring = spec.Ring(N, qs)
    ref = ref_cpu.RefCtx(N, qs)
    assert ref.psis == keyring.psis
    rng = np.random.default_rng(seed)
    pool = [pow(3, s, 2 * N) for s in range(1, N // 2)]
    baby_gs, giant_gs = pool[:N_BABY], [pool[N_BABY], 2 * N - 1]            # one step, then the conjugation
    # keys over the key ring: coefficient domain for the spec, their transforms (spec.poly_nntt) for the oracle
    keys_c = [[(_lists(H.rand_residues(rng, qs, (), N)), _lists(H.rand_residues(rng, qs, (), N))) for _ in range(Lk)]
              for _ in range(N_BABY + N_GIANT)]
    keys = [np.array([[spec.poly_nntt(m, keyring), spec.poly_nntt(md, keyring)] for m, md in k], dtype=np.uint64) for k in keys_c]
    cq = qs[:level]
    diags = H.rand_residues(rng, cq, (N_IN, N_GIANT + 1, N_BABY + 1), N)
    cts = [H.rand_residues(rng, cq, (BATCH, 2), N) for _ in range(N_IN)]
    for l, q in enumerate(cq):                                             # growth-maximising words among the uniform ones
        diags[0, 0, 0, l] = q - 1
        cts[0][0, :, l] = q - 1
    bias = H.rand_residues(rng, cq, (), N)
    return qs, level, keyring, ref, baby_gs, giant_gs, keys_c, keys, diags, cts, bias


def _spec_rotate(key_c, g, ct, cring, keyring, special):
    return spec.keyswitch(key_c, [spec.poly_galois(c, g, cring) for c in ct], cring, keyring, special)


def _spec_product(level, keyring, special, baby_gs, giant_gs, keys_c, diags, cts, bias, b):
    """ciphertext b of the block-row product from the spec's parts: [2][level][N] Python integers"""
    cring = keyring.select(range(level))
    inner = [[spec.poly_zero(cring), spec.poly_zero(cring)] for _ in range(N_GIANT + 1)]
    for m in range(len(cts)):
        ct = [_lists(cts[m][b, s]) for s in range(2)]
        terms = [ct] + [_spec_rotate(keys_c[r], g, ct, cring, keyring, special) for r, g in enumerate(baby_gs)]
        for i, term in enumerate(terms):
            img = [spec.poly_nntt(c, cring) for c in term]
            for j in range(N_GIANT + 1):
                d = _lists(diags[m][j][i])
                inner[j] = [spec.poly_add(inner[j][s], spec.poly_pointwise(d, img[s], cring), cring) for s in range(2)]
    parts = [[spec.poly_inntt(c, cring) for c in x] for x in inner]
    out = parts[0]
    for j, g in enumerate(giant_gs):
        rot = _spec_rotate(keys_c[len(baby_gs) + j], g, parts[j + 1], cring, keyring, special)
        out = [spec.poly_add(out[s], rot[s], cring) for s in range(2)]
    if bias is not None:
        out[0] = spec.poly_add(out[0], _lists(bias), cring)
    return inner, out


@pytest.mark.parametrize("special", [True, False])
def test_oracle_is_the_spec_word_for_word(special):
    qs, level, keyring, ref, baby_gs, giant_gs, keys_c, keys, diags, cts, bias = _setup(special, 16 + special)
    bk, gk = keys[:N_BABY], keys[N_BABY:]
    got = MO.matmul_bsgs_blocks_ref(ref, level, special, bk, baby_gs, gk, giant_gs, diags, cts, bias)
    inner = MO.inner_sums(ref, level, special, bk, baby_gs, diags, cts)
    one = MO.matmul_bsgs_ref(ref, level, special, bk, baby_gs, gk, giant_gs, diags[0], cts[0])
    diag = MO.matmul_diag_ref(ref, level, special, bk, baby_gs, diags[0][0], cts[0])
    assert got.dtype == np.uint64 and got.shape == (BATCH, 2, level, N)
    for b in range(BATCH):
        want_inner, want = _spec_product(level, keyring, special, baby_gs, giant_gs, keys_c, diags, cts, bias, b)
        assert got[b].tolist() == want, b
        assert [inner[j][b].tolist() for j in range(N_GIANT + 1)] == want_inner, b
        inner1, want1 = _spec_product(level, keyring, special, baby_gs, giant_gs, keys_c, diags[:1], cts[:1], None, b)
        assert one[b].tolist() == want1, b
        assert diag[b].tolist() == inner1[0], b                             # n_giant = 0 without the closing inverse transform
    # rotate is keyswitch after the Galois map, as the spec has them
    cring = keyring.select(range(level))
    rot = MO.rotate(ref, level, special, keys[0], baby_gs[0], cts[1])
    assert rot[1].tolist() == _spec_rotate(keys_c[0], baby_gs[0], [_lists(cts[1][1, s]) for s in range(2)], cring, keyring, special)


@pytest.mark.parametrize("special", [True, False])
def test_an_input_with_zero_diagonals_adds_nothing(special):
    """n_in = 2 with the second input's diagonals all zero is n_in = 1, whatever the second ciphertext; a bias moves component 0 only"""
    qs, level, keyring, ref, baby_gs, giant_gs, keys_c, keys, diags, cts, bias = _setup(special, 61 + special)
    bk, gk = keys[:N_BABY], keys[N_BABY:]
    diags = diags.copy()
    diags[1] = 0
    two = MO.matmul_bsgs_blocks_ref(ref, level, special, bk, baby_gs, gk, giant_gs, diags, cts)
    one = MO.matmul_bsgs_blocks_ref(ref, level, special, bk, baby_gs, gk, giant_gs, diags[:1], cts[:1])
    assert np.array_equal(two, one)
    assert np.array_equal(one, MO.matmul_bsgs_ref(ref, level, special, bk, baby_gs, gk, giant_gs, diags[0], cts[0]))
    with_bias = MO.matmul_bsgs_blocks_ref(ref, level, special, bk, baby_gs, gk, giant_gs, diags, cts, bias)
    assert np.array_equal(with_bias[:, 1], one[:, 1])
    q = np.array(qs[:level], dtype=object).reshape(1, level, 1)
    assert np.array_equal((with_bias[:, 0].astype(object) - one[:, 0].astype(object)) % q, np.broadcast_to(bias.astype(object)[None], one[:, 0].shape))
