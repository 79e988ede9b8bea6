"""No-GPU checks of the rectangular matrix product (tfhe_rotate_sum, tfhe_matmul_bsgs_fold, she.rect_diagonals): the two symbols are
declared, exported, bound by ctypes and by the Julia shim with one signature; she.rect_diagonals -- extended diagonals, baby / giant
regrouping and fold steps -- reproduces W @ X in a numpy model of the slots; every argument check that does not need the ring runs on
the host before any device use, in the order the header states; the body of k_md_fold (csrc/lazy_sum.h fold_term), run on the CPU with
the kernel's walk (tests/md_fold_emul/), equals exact integer sums at the edges of the 52-, 61- and 62-bit classes; the gfx950 code
objects of both instantiations use no scratch memory; and the mirror's usage errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import kernel_harness as KH
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native, she

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ctx, key_limbs, level, special, evks, galois_elements, group_sizes, n_groups, n_digits, ct, out, batch)
SUM = ("tfhe_rotate_sum", ["ptr", "int", "int", "int", "ptr", "ptr", "ptr", "int", "int", "ptr", "ptr", "i64"])
# (ctx, key_limbs, level, special, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, n_digits, diags, cts, n_in, fold_evks,
#  fold_galois, fold_group_sizes, n_fold_groups, bias, out, batch)
FOLD = ("tfhe_matmul_bsgs_fold", ["ptr", "int", "int", "int", "ptr", "ptr", "int", "ptr", "ptr", "int", "int", "ptr", "ptr", "int", "ptr", "ptr",
                                  "ptr", "int", "ptr", "ptr", "i64"])


def _err():
    return native.lib().tfhe_last_error().decode()


# ---- one signature everywhere --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,classes", [SUM, FOLD])
def test_symbols_declared_exported_and_bound_with_one_signature(name, classes):
    protos = shim.header_prototypes()
    assert name in protos, f"{name} is not declared in include/toyfhe_hip.h"
    assert protos[name] == ("int", classes)
    assert name in native.EXPORTED_SYMBOLS
    f = getattr(native.lib(), name)                      # AttributeError: not exported by the library
    assert f.restype is C.c_int and len(f.argtypes) == len(classes)
    for k, t in zip(classes, f.argtypes):
        if k == "ptr":
            assert t is C.c_void_p or hasattr(t, "contents"), t
        else:
            assert t is {"int": C.c_int, "i64": C.c_int64}[k], (k, t)
    sizes = f.argtypes[6] if name == SUM[0] else f.argtypes[16]
    assert sizes._type_ is C.c_int                       # the group sizes are a host int array
    mirror = name[len("tfhe_"):]
    assert callable(getattr(native.Context, mirror)) and callable(getattr(she, mirror))
    import toyfhe_jl_amd as tf
    assert getattr(tf, mirror) is getattr(she, mirror) and tf.rect_diagonals is she.rect_diagonals


@pytest.mark.parametrize("name,classes", [SUM, FOLD])
def test_julia_shim_binds_the_same_signature(name, classes):
    calls = [c for c in shim.shim_ccalls() if c[0] == name]
    assert len(calls) == 1, f"the shim binds {name} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == classes and nargs == len(classes)
    src = open(shim.SHIM).read()
    body = src[src.index(f"function {name[len('tfhe_'):]}("):]
    body = body[:body.index("\nend")]
    assert "GC.@preserve" in body and re.search(r"\bon\(", body) and "prepared(" in body


def test_header_states_the_composition_and_the_order_of_the_checks():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index("int tfhe_rotate_sum(")
    doc = text[text.rindex("/*", 0, i):i]
    for word in ("[batch][2][level][N]", "PREPARED", "HOST", "coefficient domain", "word for word", "tfhe_rotate_many", "tfhe_add",
                 "tfhe_ctx_set_chunk", "same bits", "TFHE_E_BADARG", "batch == 0", "[0, 64]", "out = ct", "in this order"):
        assert word in doc, word
    order = [doc.index(w) for w in ("null arrays", "n_groups\n * outside [0, 64]", "group size below 1", "more than 64 keys", "a null key",
                                    "even Galois element", "starting where ct starts", "then the context", "level / key-limb rules",
                                    "not below 2N", "overlapping ct anywhere")]
    assert order == sorted(order), order
    i = text.index("int tfhe_matmul_bsgs_fold(")
    doc = text[text.rindex("/*", 0, i):i]
    for word in ("tfhe_matmul_bsgs_blocks (bias = NULL) -> tfhe_rotate_sum -> tfhe_add", "AFTER the fold", "n_fold_groups = 0", "word for word",
                 "tfhe_ctx_set_chunk", "in this order", "W[r mod m][(r - i) mod n]"):
        assert word in doc, word
    order = [doc.index(w) for w in ("null arrays", "a null key among", "diags[m] or cts[m] among", "outside [0, 64]", "outside [1, 64]",
                                    "n_fold_groups outside [0, 64]", "fold group size below 1", "more than 64 fold keys", "a null fold key",
                                    "even Galois element", "starting where", "then the context", "level / key-limb rules", "not below 2N",
                                    "overlapping any operand anywhere")]
    assert order == sorted(order), order


# ---- rect_diagonals against W @ X ------------------------------------------------------------------------------------------

def _slot_product(D, baby, giant, folds, x):
    """matmul_bsgs_fold on slot vectors: rotation by s steps is np.roll(x, s)"""
    rots = [x] + [np.roll(x, s) for s in baby]
    inner = [sum(D[j][i] * rots[i] for i in range(len(rots))) for j in range(len(giant) + 1)]
    f = inner[0] + sum(np.roll(inner[j + 1], s) for j, s in enumerate(giant))
    for grp in folds:
        f = f + sum(np.roll(f, s) for s in grp)
    return f


@pytest.mark.parametrize("m0,n,block,n1", [(2, 8, 1, 2), (3, 8, 2, 2), (10, 64, 4, 4), (8, 8, 1, 3), (1, 4, 1, 1), (5, 16, 3, 4), (2, 8, 4, 8)])
def test_wide_rect_diagonals_give_the_matrix_product(m0, n, block, n1):
    rng = np.random.default_rng(100 * m0 + n)
    W = rng.integers(-9, 10, size=(m0, n)).astype(np.float64)
    X = rng.integers(-9, 10, size=(n, block)).astype(np.float64)
    m = 1 << (m0 - 1).bit_length()
    want = np.zeros((m, block))
    want[:m0] = W @ X
    want = np.tile(want, (n // m, 1)).reshape(-1)           # row r holds (W @ X)[r mod m]; the padding rows read 0
    outs = {}
    for radix in (2, 4):
        D, baby, giant, folds = she.rect_diagonals(W, n1, block, fold_radix=radix)
        nb1 = min(n1, m)
        assert D.shape == (-(-m // nb1), nb1, n * block)
        assert baby == [i * block for i in range(1, nb1)] and giant == [j * nb1 * block for j in range(1, -(-m // nb1))]
        lg = (n // m).bit_length() - 1
        if radix == 2:
            assert folds == [[m * block << t] for t in range(lg)]
        else:
            assert [len(g) for g in folds] == [3] * (lg // 2) + [1] * (lg % 2)
            assert all(g == [s, 2 * s, 3 * s] for g, s in zip(folds, (m * block * 4 ** t for t in range(lg // 2))))
            assert lg % 2 == 0 or folds[-1] == [m * block << (lg - 1)]
        outs[radix] = _slot_product(D, baby, giant, folds, X.reshape(-1))
        assert np.array_equal(outs[radix], want), (radix, m0, n)
    assert np.array_equal(outs[2], outs[4])
    if m == n:
        assert she.rect_diagonals(W, n1, block)[3] == []
    # the default radix is 4 (the measured choice, profiles/LOG.md)
    assert she.rect_diagonals(W, n1, block)[3] == she.rect_diagonals(W, n1, block, fold_radix=4)[3]


@pytest.mark.parametrize("m0,n,block,n1", [(16, 4, 1, 2), (8, 2, 4, 2), (16, 4, 2, 4)])
def test_tall_rect_diagonals_give_the_matrix_product_of_a_periodic_input(m0, n, block, n1):
    rng = np.random.default_rng(m0 + n)
    W = rng.integers(-9, 10, size=(m0, n)).astype(np.float64)
    X = rng.integers(-9, 10, size=(n, block)).astype(np.float64)
    D, baby, giant, folds = she.rect_diagonals(W, n1, block)
    assert folds == [] and D.shape[2] == m0 * block and D.shape[0] * D.shape[1] >= n
    x = np.tile(X, (m0 // n, 1)).reshape(-1)                # row r holds X[r mod n]
    assert np.array_equal(_slot_product(D, baby, giant, folds, x), (W @ X).reshape(-1))


def test_a_wide_layer_feeds_a_tall_one():
    """the fold leaves row r = out[r mod m]: the periodic input the tall form asks for"""
    rng = np.random.default_rng(7)
    W1, W2 = rng.integers(-5, 6, size=(2, 8)).astype(np.float64), rng.integers(-5, 6, size=(8, 2)).astype(np.float64)
    X = rng.integers(-5, 6, size=(8, 4)).astype(np.float64)
    mid = _slot_product(*she.rect_diagonals(W1, 2, 4, fold_radix=2), X.reshape(-1))
    out = _slot_product(*she.rect_diagonals(W2, 2, 4), mid)
    assert np.array_equal(out, (W2 @ (W1 @ X)).reshape(-1))


def test_rect_diagonals_refuses_shapes_it_cannot_fold():
    with pytest.raises(she.UsageError, match="power of two times"):
        she.rect_diagonals(np.zeros((3, 12)), 2)             # 12 / 4 = 3
    with pytest.raises(she.UsageError, match="power of two times"):
        she.rect_diagonals(np.zeros((5, 12)), 2)             # 8 does not divide 12
    with pytest.raises(she.UsageError, match="multiple of its column count"):
        she.rect_diagonals(np.zeros((10, 4)), 2)
    with pytest.raises(AssertionError, match="fold_radix 2 or 4"):
        she.rect_diagonals(np.zeros((2, 8)), 2, fold_radix=3)


# ---- argument validation precedes device use -------------------------------------------------------------------------------

def _arr(t, xs, fill):
    """65 valid entries behind the ones under test: a count out of range reads none that is not there"""
    return (t * 65)(*(list(xs) + [fill] * (65 - len(xs))))


def test_rotate_sum_argument_validation_precedes_device_use():
    """every status that does not need the ring, with no context and host pointers, in the header's order: each call breaks one rule
    and later ones too where it can (a null context always), and must report the earliest"""
    f = native.lib().tfhe_rotate_sum
    bufs = [np.zeros(64, dtype=np.uint64) for _ in range(4)]
    pk, pk2, pc, po = (x.ctypes.data for x in bufs)

    def call(keys=(pk, pk2, pk), gs=(3, 5, 9), sizes=(2, 1), n_groups=None, ct=pc, out=po, batch=1, drop=None):
        args = dict(keys=_arr(C.c_void_p, keys, pk), gs=_arr(C.c_uint64, gs, 3), sizes=_arr(C.c_int, sizes, 1))
        if drop:
            args[drop] = None
        return f(None, 3, 2, 1, args["keys"], args["gs"], args["sizes"], len(sizes) if n_groups is None else n_groups, 2, ct, out, batch)
    # 1. null arrays, ahead of everything behind them
    for drop in ("keys", "gs", "sizes"):
        assert call(drop=drop, n_groups=65, gs=(4,), out=pc) == native.E_BADARG and "null argument" in _err(), drop
    assert call(ct=None, n_groups=-1) == native.E_BADARG and "null argument" in _err()
    assert call(out=None, sizes=(0,)) == native.E_BADARG and "null argument" in _err()
    # 2. the group count, ahead of a bad size
    for n in (-1, 65):
        assert call(n_groups=n, sizes=(0,)) == native.E_BADARG and "n_fold_groups" in _err(), n
    # 3. a group size below 1, ahead of too many keys and a null key
    for bad in (0, -3):
        assert call(sizes=(2, bad, 64), keys=(None,)) == native.E_BADARG and "fold group 1 has size" in _err(), bad
    # 4. more than 64 keys in all (one group, or their sum), ahead of a null key
    assert call(sizes=(65,), keys=(None,)) == native.E_BADARG and "more than 64 fold keys" in _err()
    assert call(sizes=(32, 32, 1), keys=(None,)) == native.E_BADARG and "more than 64 fold keys" in _err()
    # 5. a null key among the counted ones, ahead of an even element; one beyond the count is not read
    assert call(keys=(pk, pk, None), gs=(3, 4, 5)) == native.E_BADARG and "null fold key 2" in _err()
    assert call(keys=(pk, pk, pk, None)) == native.E_BADARG and "null context" in _err()
    # 6. an even Galois element, ahead of out on ct
    assert call(gs=(3, 5, 4), out=pc) == native.E_BADARG and "galois element must be odd" in _err()
    assert call(gs=(3, 5, 9, 4)) == native.E_BADARG and "null context" in _err()
    # 7. out starting where ct starts
    assert call(out=pc) == native.E_BADARG and "out overlaps an operand" in _err()
    # 8. the context is next: the limits themselves, no group at all, an empty batch
    assert call() == native.E_BADARG and "null context" in _err()
    assert call(sizes=(64,)) == native.E_BADARG and "null context" in _err()
    assert call(sizes=(1,) * 64) == native.E_BADARG and "null context" in _err()
    assert call(sizes=()) == native.E_BADARG and "null context" in _err()
    assert call(batch=0) == native.E_BADARG and "null context" in _err()
    with pytest.raises(AssertionError):
        native.check(call(sizes=(0,)))


def test_matmul_bsgs_fold_argument_validation_precedes_device_use():
    """tfhe_matmul_bsgs_blocks' checks in its order, the fold's among them"""
    f = native.lib().tfhe_matmul_bsgs_fold
    bufs = [np.zeros(64, dtype=np.uint64) for _ in range(9)]
    pk, pk2, pd, pd2, pc, pc2, pb, po, pf = (x.ctypes.data for x in bufs)

    def call(baby=(pk, pk2), bg=(3, 5), giant=(pk,), gg=(9,), n_baby=None, n_giant=None, diags=(pd, pd2), cts=(pc, pc2), n_in=None,
             fold=(pf, pf), fg=(7, 11), sizes=(1, 1), n_fold=None, bias=pb, out=po, batch=1, drop=None):
        args = dict(baby=_arr(C.c_void_p, baby, pk), bg=_arr(C.c_uint64, bg, 3), giant=_arr(C.c_void_p, giant, pk), gg=_arr(C.c_uint64, gg, 3),
                    diags=_arr(C.c_void_p, diags, pd), cts=_arr(C.c_void_p, cts, pc), fold=_arr(C.c_void_p, fold, pf),
                    fg=_arr(C.c_uint64, fg, 3), sizes=_arr(C.c_int, sizes, 1))
        if drop:
            args[drop] = None
        return f(None, 3, 2, 1, args["baby"], args["bg"], len(baby) if n_baby is None else n_baby, args["giant"], args["gg"],
                 len(giant) if n_giant is None else n_giant, 2, args["diags"], args["cts"], len(cts) if n_in is None else n_in,
                 args["fold"], args["fg"], args["sizes"], len(sizes) if n_fold is None else n_fold, bias, out, batch)
    # 1. nulls: the arrays, the fold's three among them ...
    for drop in ("baby", "bg", "giant", "gg", "diags", "cts", "fold", "fg", "sizes"):
        assert call(drop=drop, n_in=0, gg=(4,), out=pb, n_fold=65) == native.E_BADARG and "null argument" in _err(), drop
    assert call(out=None) == native.E_BADARG and "null argument" in _err()
    # ... a null key, a null entry per input, each ahead of a count out of range
    assert call(baby=(pk, None), n_in=0) == native.E_BADARG and "null baby key 1" in _err()
    assert call(giant=(None,), n_baby=-1) == native.E_BADARG and "null giant key 0" in _err()
    assert call(diags=(pd, None), n_giant=65, n_fold=-1) == native.E_BADARG and "null diagonals of input 1" in _err()
    assert call(cts=(None, pc2), n_baby=65) == native.E_BADARG and "null ciphertext of input 0" in _err()
    # 2. the counts of the product, ahead of the fold's
    for n in (-1, 65):
        assert call(n_baby=n, n_fold=65) == native.E_BADARG and "n_baby" in _err(), n
        assert call(n_giant=n, sizes=(0,)) == native.E_BADARG and "n_giant" in _err(), n
    for n in (0, -1, 65):
        assert call(n_in=n, n_fold=-1) == native.E_BADARG and "n_in" in _err(), n
    # 3. the fold's: group count, a size below 1, more than 64 keys, a null key -- each ahead of the next and of an even element
    for n in (-1, 65):
        assert call(n_fold=n, sizes=(0,)) == native.E_BADARG and "n_fold_groups" in _err(), n
    assert call(sizes=(1, 0, 65)) == native.E_BADARG and "fold group 1 has size 0" in _err()
    assert call(sizes=(65,), fold=(None,)) == native.E_BADARG and "more than 64 fold keys" in _err()
    assert call(sizes=(60, 5), fold=(None,)) == native.E_BADARG and "more than 64 fold keys" in _err()
    assert call(fold=(pf, None), gg=(4,)) == native.E_BADARG and "null fold key 1" in _err()
    assert call(fold=(pf, pf, None)) == native.E_BADARG and "null context" in _err()           # beyond its count: not read
    # 4. an even Galois element of any of the three sets, ahead of out on an operand
    assert call(bg=(3, 4), out=pc) == native.E_BADARG and "galois element must be odd" in _err()
    assert call(gg=(0,), out=pb) == native.E_BADARG and "galois element must be odd" in _err()
    assert call(fg=(7, 6), out=pd) == native.E_BADARG and "galois element must be odd" in _err()
    # 5. out starting where an operand starts
    for o in (pc, pc2, pd, pd2, pb):
        assert call(out=o) == native.E_BADARG and "out overlaps an operand" in _err()
    # 6. the context is next: with and without a bias, without fold steps, an empty batch
    assert call() == native.E_BADARG and "null context" in _err()
    assert call(bias=None) == native.E_BADARG and "null context" in _err()
    assert call(sizes=()) == native.E_BADARG and "null context" in _err()
    assert call(sizes=(3, 61), fold=(pf,) * 64, fg=(3,) * 64) == native.E_BADARG and "null context" in _err()
    assert call(batch=0) == native.E_BADARG and "null context" in _err()
    with pytest.raises(AssertionError):
        native.check(call(n_in=0))


# ---- the body of k_md_fold on the CPU ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = KH.build_emul("md_fold_emul/md_fold_emul.cpp", tmp_path_factory.mktemp("md_fold_emul"))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.md_fold_emul.argtypes, L.md_fold_emul.restype = [u64, C.c_int, u64, u32, u32, u32] + [vp] * 8, C.c_long
    return L


def _fold_moduli():
    """the smallest and the largest prime of 52, 61 and 62 bits (q = 1 mod 2^12)"""
    N = 1 << 11
    out = []
    for bits in (52, 61, 62):
        out += [H.primes_above(1 << (bits - 1), 1, N)[0], H.primes_below(1 << bits, 1, N)[0]]
        assert [q.bit_length() for q in out[-2:]] == [bits, bits]
    return out


@pytest.mark.parametrize("q", _fold_moduli())
@pytest.mark.parametrize("edge", [False, True])
def test_fold_body_matches_exact_sums(emul, q, edge):
    """S = X + sum_r (V[pi_r k] - U[k] (pinv)) for r = 1, 3 and 64 rotations, both USCALE forms, at n = 16 (every lane but the first
    clamped), n = 2^11 (one workgroup of a team, no clamped lane) and n = 2^13 (four workgroups per team), with uniform words and with
    every word of X, V and U equal to q - 1; every coefficient is stored exactly once"""
    rng = np.random.default_rng(q % 1000 + edge)
    pinv = int(rng.integers(1, 1 << 29)) % q or 1
    for n, rots in ((16, (1, 3, 64)), (1 << 11, (1, 3, 64)), (1 << 13, (3,))):
        for nrot in rots:
            x = H.words_mod(rng, q, (2, n), edge)
            v = H.words_mod(rng, q, (nrot, n, 2), edge)
            u = H.words_mod(rng, q, (2, nrot, n), edge)
            gs = np.array([(2 * int(t) + 3) % (2 * n) | 1 for t in rng.integers(0, n, nrot)], dtype=np.uint64)
            for uscale in (0, 1):
                s = np.full((2, n), q - 1, dtype=np.uint64) if not edge else np.zeros((2, n), dtype=np.uint64)
                stored = emul.md_fold_emul(q, uscale, pinv, n, nrot, 32, x[0].ctypes.data, x[1].ctypes.data, v.ctypes.data, u[0].ctypes.data,
                                           u[1].ctypes.data, gs.ctypes.data, s[0].ctypes.data, s[1].ctypes.data)
                assert stored == n, (n, nrot, stored)
                for c in (0, 1):
                    want = x[c].astype(object)
                    for t in range(nrot):
                        uu = u[c][t].astype(object) * (pinv if uscale else 1) % q
                        want = want + (v[t][H.galois_pos(n, int(gs[t])), c].astype(object) - uu) % q
                    assert np.array_equal(s[c].astype(object), want % q), (q, n, nrot, uscale, c)
    assert emul.md_fold_emul(q, 0, pinv, 16, 0, 32, *([None] * 8)) == -1


# ---- resources of the gfx950 code objects ------------------------------------------------------------------------------------

@KH.needs_hipcc
def test_fold_kernels_use_no_scratch(tmp_path):
    """compiler-reported scratch is 0 for both instantiations of k_md_fold (32 running words and the 32 gathered words of the next
    rotation per thread)"""
    kernels = KH.kernel_resources("md_fold_emul/resource_probe.hip", tmp_path)
    fold = [k for k in kernels if re.match(r"_Z\d+k_md_foldILb[01]EE", k["name"])]
    assert len(fold) == 2, [k["name"] for k in kernels]
    for k in fold:
        print(f"{k['name']}: {k['vgprs']} VGPRs, {k['agprs']} AGPRs, scratch {k['scratch']}")
        assert k["scratch"] == 0, (k["name"], k["scratch"])


def test_fold_goes_through_the_launch_helper_and_the_split_rotation_phase():
    """csrc/md_api.inc: both forms of the fold kernel are launched, the plain route adds the coefficient-domain rows without a
    transform, and md_rotations still ends in the forward transforms its two product callers need"""
    src = open(os.path.join(ROOT, "toyfhe.jl_amd", "csrc", "md_api.inc")).read()
    run = src[src.index("static int md_fold_run("):src.index("// the output tile")]
    assert "scaled ? k_md_fold<false> : k_md_fold<true>" in run and "launch(c, fold," in run
    plain = run[run.index("} else {"):]
    assert "md_rotations_coeff(" in plain and "k_bsgs_sum" in plain and "run_ntt" not in plain
    rot = src[src.index("static int md_rotations("):src.index("// ---- diagonal matrix-vector product")]
    assert "md_rotations_coeff(c, P, evks, cin, nb, B)" in rot and "run_ntt(c, false, B.ROT, B.ROT" in rot


# ---- the mirror's usage errors ---------------------------------------------------------------------------------------------

def test_mirror_usage_errors():
    from tests.test_matmul_bsgs_blocks_cpu import _Stub
    c = _Stub()
    with pytest.raises(she.UsageError, match="a fold step without a key"):
        she.rotate_sum([[]], c)
    with pytest.raises(she.UsageError, match="at most 64 fold steps and 64 fold keys"):
        she.rotate_sum([[None]] * 65, c)
    with pytest.raises(she.UsageError, match="at most 64 fold steps and 64 fold keys"):
        she.rotate_sum([[None] * 33, [None] * 32], c)
    with pytest.raises(AssertionError, match="2-element"):
        she.rotate_sum([[None]], _Stub(n=3))
    assert she.rotate_sum([], c) is c
    # matmul_bsgs_fold: the fold's own, then those of matmul_bsgs_blocks
    f = she.matmul_bsgs_fold
    with pytest.raises(she.UsageError, match="a fold step without a key"):
        f([], [], [[[None]]], [c], [[None], []])
    with pytest.raises(she.UsageError, match="one set of diagonals per input"):
        f([], [], [[[None]]], [c, c], [])
    with pytest.raises(she.UsageError, match="at most 64 inputs"):
        f([], [], [[[None]]] * 65, [c] * 65, [])
    with pytest.raises(she.UsageError, match="one ring, level, scale and batch"):
        f([], [], [[[None]]] * 2, [c, _Stub(scale=2**21)], [])
    with pytest.raises(she.UsageError, match="at most 64 baby and 64 giant"):
        f([None] * 65, [], [[[None]]], [c], [])
    with pytest.raises(she.UsageError, match="single plaintext elements"):
        f([], [], [[[None]]], [c], [])
