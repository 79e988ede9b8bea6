"""No-GPU checks of the rotate-and-sum fold and the rectangular product on grouped-digit keys (tfhe_rotate_sum_grouped,
tfhe_matmul_bsgs_fold_grouped): both symbols are declared, exported, bound by ctypes and by the Julia shim with one signature; the oracle
(tests/rotate_sum_grouped_oracle.py) against tests/rotate_sum_oracle.py in the two degenerate cases; the bodies of the two kernels of an
evaluation-domain fold step -- the gather's sum over the kernel's layouts and csrc/ks_group_core.h mdg_fold_finish_coeff --, run on the CPU
over whole rows (tests/mdg_fold_emul/), against Python integers and against the coefficient route -- the tail of every rotation, then the sum; the host
checks in the header's order, on plain numbers; the gfx950 code objects' scratch; and the mirror's argument rules."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest

from oracle import ref_cpu
from tests import helpers as H
from tests import kernel_harness as KH
from tests import rotate_sum_grouped_oracle as FO
from tests import rotate_sum_oracle as RO
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native, she

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLD, PRODUCT = "tfhe_rotate_sum_grouped", "tfhe_matmul_bsgs_fold_grouped"
CLASSES = {
    # (ctx, key_limbs, level, n_special, group, evks, galois_elements, group_sizes, n_groups, n_digits, ct, out, batch)
    FOLD: ["ptr", "int", "int", "int", "int", "ptr", "ptr", "ptr", "int", "int", "ptr", "ptr", "i64"],
    # (ctx, key_limbs, level, n_special, group, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, n_digits, diags, cts, n_in,
    #  fold_evks, fold_galois, fold_group_sizes, n_fold_groups, bias, out, batch)
    PRODUCT: ["ptr", "int", "int", "int", "int", "ptr", "ptr", "int", "ptr", "ptr", "int", "int", "ptr", "ptr", "int", "ptr", "ptr", "ptr", "int",
              "ptr", "ptr", "i64"],
}
POISON = 0xA5A5A5A5A5A5A5A5


# ---- one signature everywhere --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [FOLD, PRODUCT])
def test_symbol_declared_exported_and_bound_with_one_signature(name):
    protos = shim.header_prototypes()
    assert name in protos, f"{name} is not declared in include/toyfhe_hip.h"
    assert protos[name] == ("int", CLASSES[name])
    assert name in native.EXPORTED_SYMBOLS
    f = getattr(native.lib(), name)                      # AttributeError: not exported by the library
    assert f.restype is C.c_int and len(f.argtypes) == len(CLASSES[name])
    for k, t in zip(CLASSES[name], f.argtypes):
        if k == "ptr":
            assert t is C.c_void_p or issubclass(t, C._Pointer), (k, t)
        else:
            assert t is {"int": C.c_int, "i64": C.c_int64}[k], (k, t)
    assert callable(native.Context.rotate_sum_grouped) and callable(native.Context.matmul_bsgs_fold_grouped)
    import toyfhe_jl_amd as tf
    assert callable(tf.rotate_sum_grouped) and callable(tf.matmul_bsgs_fold_grouped)
    calls = [c for c in shim.shim_ccalls() if c[0] == name]
    assert len(calls) == 1, f"the shim binds {name} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == CLASSES[name] and nargs == len(CLASSES[name])


def test_header_states_the_contract_and_what_is_still_refused():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index(f"int {FOLD}(")
    doc = text[text.rindex("/*", 0, i):i]
    for word in ("tfhe_galois_key_prepare", "HOST array", "word for word", "tfhe_rotate_many_grouped", "tfhe_rotate_grouped", "TFHE_MD_COEFF",
                 "TFHE_MDG_FOLD_EVAL", "in this order", "batch == 0", "untouched", "tfhe_matmul_bsgs_grouped", "fold step", "n_groups = 0", "tfhe_add"):
        assert word in doc, word
    order = [doc.index(w) for w in ("a null ctx or array", "n_groups outside", "null-key and count rules", "shape checks", "overlapping anywhere")]
    assert order == sorted(order), order
    still = text[text.index("Still refused on grouped keys"):text.index("int tfhe_rotate_many_grouped(")]
    for word in ("tfhe_rotate_sum", "tfhe_matmul_bsgs_fold", "fused N <= 2^14 key switch", FOLD, PRODUCT):
        assert word in still, word
    assert "has no grouped form" not in text


def test_a_null_argument_is_refused_by_the_library_before_any_device_use():
    lib = native.lib()
    buf = np.zeros(8, dtype=np.uint64).ctypes.data
    keys = (C.c_void_p * 2)(buf, None)
    gs = (C.c_uint64 * 2)(4, 3)
    sizes = (C.c_int * 2)(0, 99)
    rc = lib.tfhe_rotate_sum_grouped(None, 0, 0, 9, 0, keys, gs, sizes, 70, 0, buf, buf, -1)
    assert rc == native.E_BADARG and "null argument" in lib.tfhe_last_error().decode()
    rc = lib.tfhe_matmul_bsgs_fold_grouped(None, 0, 0, 9, 0, keys, gs, 70, keys, gs, -1, 0, keys, keys, 0, keys, gs, sizes, 70, None, buf, -1)
    assert rc == native.E_BADARG and "null argument" in lib.tfhe_last_error().decode()


# ---- the oracle in the two degenerate cases --------------------------------------------------------------------------------

@pytest.mark.parametrize("special", [1, 0])
def test_oracle_with_one_limb_per_digit_is_the_per_limb_oracle(special):
    """(k, alpha) = (1, 1) is ModulusRaised with one special prime, (0, 1) the plain RNS gadget: the words of rotate_sum_ref and
    matmul_bsgs_fold_ref"""
    N, Lk = 16, 4
    qs = H.chain(30, Lk, N)
    ref = ref_cpu.RefCtx(N, qs)
    level = Lk - special
    rng = np.random.default_rng(special)
    nb, ng, nin, batch = 1, 1, 2, 2
    bgs, ggs, fgs = [3], [9], [[5, 2 * N - 1], [25]]
    bk = [H.uniform_evk(rng, qs, level, N) for _ in bgs]
    gk = [H.uniform_evk(rng, qs, level, N) for _ in ggs]
    fk = [[H.uniform_evk(rng, qs, level, N) for _ in st] for st in fgs]
    diags = [H.rand_residues(rng, qs[:level], (ng + 1, nb + 1), N) for _ in range(nin)]
    cts = [H.rand_residues(rng, qs[:level], (batch, 2), N) for _ in range(nin)]
    bias = H.rand_residues(rng, qs[:level], (), N)
    assert np.array_equal(FO.rotate_sum_grouped_ref(ref, level, special, 1, fk, fgs, cts[0]), RO.rotate_sum_ref(ref, level, special, fk, fgs, cts[0]))
    for b in (None, bias):
        want = RO.matmul_bsgs_fold_ref(ref, level, special, bk, bgs, gk, ggs, diags, cts, fk, fgs, bias=b)
        got = FO.matmul_bsgs_fold_grouped_ref(ref, level, special, 1, bk, bgs, gk, ggs, diags, cts, fk, fgs, bias=b)
        assert np.array_equal(got, want), (special, b is not None)


# ---- the emulation ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = KH.build_emul("mdg_fold_emul/mdg_fold_emul.cpp", tmp_path_factory.mktemp("mdg_fold_emul"))
    vp, i32, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    L.mdg_fold_emul_jb.argtypes, L.mdg_fold_emul_jb.restype = [], i32
    L.mdg_fold_emul_gather.argtypes, L.mdg_fold_emul_gather.restype = [vp, C.c_long, i32, i32, i32, i32, vp, vp, vp, vp], i32
    L.mdg_fold_emul_finish.argtypes, L.mdg_fold_emul_finish.restype = [i32, i32, i32, vp, C.c_long, i32, vp, vp, vp, vp, vp], i32
    L.mdg_fold_emul_check.argtypes = [i32, i32, i32, i64, i32, i32, i32, i32, i32, i64, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, u64, u64,
                                      vp, C.c_char_p, C.c_size_t]
    L.mdg_fold_emul_check.restype = i32
    return L


@pytest.fixture(scope="module")
def rot_emul(tmp_path_factory):
    L = KH.build_emul("ks_group_rot_emul/ks_group_rot_emul.cpp", tmp_path_factory.mktemp("ks_group_rot_emul_for_mdg_fold"))
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    L.ks_group_rot_emul_tail.argtypes, L.ks_group_rot_emul_tail.restype = [i32, i32, vp, C.c_long, u64, vp, vp, vp], i32
    return L


def _mixed_ring(K, N):
    """level = 3 ciphertext limbs of 30, 50 and 61 bits, then K special primes of 61, 30, 50 and 61 bits: every size on both sides"""
    p30, p50, p61 = H.chain(30, 2, N), H.chain(50, 2, N), H.chain(61, 3, N)
    return [p30[0], p50[0], p61[0]] + [p61[1], p30[1], p50[1], p61[2]][:K]


def _finish(emul, K, jb, level, w, pb, e, bias):
    """pb [R][K][N], e [level][N] -> dst [level][N], Pinv"""
    R, N = pb.shape[0], pb.shape[2]
    wa = np.array(w, dtype=np.uint64)
    pb, e = np.ascontiguousarray(pb, dtype=np.uint64), np.ascontiguousarray(e, dtype=np.uint64)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.uint64)
    dst = np.full((level, N), POISON, dtype=np.uint64)
    pinv = np.zeros(level, dtype=np.uint64)
    assert emul.mdg_fold_emul_finish(K, jb, level, wa.ctypes.data, N, R, pb.ctypes.data, e.ctypes.data, None if b is None else b.ctypes.data,
                                     dst.ctypes.data, pinv.ctypes.data) == 0
    assert (dst < wa[:level].reshape(level, 1)).all()
    return dst, [int(x) for x in pinv]


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_finish_body_is_the_sum_of_the_floors_on_python_integers(emul, K, R):
    """for integers x_r in [0, Q P) given by their residues: with e_j = sum_r x_r Pinv_j (what the inverse transform of the gathered sum
    holds when nothing else is added) the finish leaves sum_r floor(x_r / P) mod q_j, plus the bias.  x = 0, P - 1, P, Q P - 1 (every
    residue q - 1), a multiple of P, random ones; both block sizes give the same words"""
    N, level = 64, 3
    w = _mixed_ring(K, N)
    Q, P = math.prod(w[:level]), math.prod(w[level:])
    rng = np.random.default_rng(10 * K + R)
    xs = []
    for r in range(R):
        row = [0, P - 1, P, Q * P - 1, P * int(rng.integers(1, 1 << 60)) % (Q * P)]
        row = row[r:] + row[:r]                                        # the edge values meet different partners in every rotation
        xs.append(row + [int.from_bytes(rng.bytes(48), "little") % (Q * P) for _ in range(N - len(row))])
    pb = np.array([[[x % p for x in xs[r]] for p in w[level:]] for r in range(R)], dtype=np.uint64)
    pinv = [pow(P, -1, q) for q in w[:level]]
    e = np.array([[sum(xs[r][i] % q * pinv[j] for r in range(R)) % q for i in range(N)] for j, q in enumerate(w[:level])], dtype=np.uint64)
    bias = H.rand_residues(rng, w[:level], (), N).reshape(level, N)
    for b in (None, bias):
        got, got_pinv = _finish(emul, K, emul.mdg_fold_emul_jb(), level, w, pb, e, b)
        assert got_pinv == pinv
        for j, q in enumerate(w[:level]):
            for i in range(N):
                assert int(got[j, i]) == (sum(xs[r][i] // P for r in range(R)) + (0 if b is None else int(b[j, i]))) % q, (K, R, j, i)
        assert np.array_equal(_finish(emul, K, 2, level, w, pb, e, b)[0], got)      # blocks of 2 + 1 limbs


def _fold_step_both_ways(emul, rot_emul, K, N, level, w, gs, T, F, bias):
    """One ciphertext (both components) through a fold step.  T [R][2][nw][N]: any canonical coefficient-domain key sums; F [2][level][N]:
    the running value.  Coefficient route: the tail of every rotation (with sigma_g(F_0) as its addend for s = 0 -- component 1's own
    rotation comes out of its key sum alone), then F + the sum, the bias onto component 0.  Evaluation route: V = NTT(T) Pinv + NTT(F_0)
    [s = 0] in the EPI layout, the gather over the chunk, one inverse transform, the finish on sigma_g of the special rows."""
    R, nw = len(gs), level + K
    ref = ref_cpu.RefCtx(N, w)
    wa = np.array(w, dtype=np.uint64)
    ql = np.array([int(q) for q in w[:level]], dtype=object).reshape(level, 1)
    # coefficient route
    want = []
    for s in (0, 1):
        total = F[s].astype(object)
        for r, g in enumerate(gs):
            rot = np.full((level, N), POISON, dtype=np.uint64)
            t, c = np.ascontiguousarray(T[r, s]), np.ascontiguousarray(F[0])
            assert rot_emul.ks_group_rot_emul_tail(K, level, wa.ctypes.data, N, g, t.ctypes.data, c.ctypes.data if s == 0 else None, rot.ctypes.data) == 0
            total = total + rot.astype(object)
        if bias is not None and s == 0:
            total = total + bias.astype(object)
        want.append((total % ql).astype(np.uint64))
    # evaluation route
    pinv = np.array([pow(math.prod(w[level:]), -1, int(q)) for q in w[:level]], dtype=object).reshape(level, 1)
    X = np.ascontiguousarray(ref.nntt(F.reshape(2, level, N), idx=range(level)).reshape(1, 2, level, N))
    Sn = ref.nntt(np.ascontiguousarray(T[:, :, :level]).reshape(R * 2, level, N), idx=range(level)).reshape(R, 2, level, N)
    V = np.full((R, nw, N, 2), POISON, dtype=np.uint64)                  # ci = r (batch 1); the special limbs' rows are not the gather's
    for r in range(R):
        V[r, :level, :, 0] = ((Sn[r, 0].astype(object) * pinv + X[0, 0].astype(object)) % ql).astype(np.uint64)
        V[r, :level, :, 1] = ((Sn[r, 1].astype(object) * pinv) % ql).astype(np.uint64)
    E = np.full((1, 2, level, N), POISON, dtype=np.uint64)
    ga, qa = np.array(gs, dtype=np.uint64), np.array(w[:level], dtype=np.uint64)
    assert emul.mdg_fold_emul_gather(qa.ctypes.data, N, R, 1, level, nw, ga.ctypes.data, X.ctypes.data, V.ctypes.data, E.ctypes.data) == 0
    Ec = ref.inntt(E.reshape(2, level, N), idx=range(level)).reshape(2, level, N)
    sp = range(level, nw)
    for s in (0, 1):
        pb = np.stack([ref.galois(g, np.ascontiguousarray(T[r, s, level:]).reshape(1, K, N), idx=sp).reshape(K, N) for r, g in enumerate(gs)])
        b = bias if s == 0 else None
        got, _ = _finish(emul, K, emul.mdg_fold_emul_jb(), level, w, pb, Ec[s], b)
        assert np.array_equal(got, want[s]), (K, N, R, s, int((got != want[s]).sum()))
        assert np.array_equal(_finish(emul, K, 2, level, w, pb, Ec[s], b)[0], want[s])


@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_evaluation_route_gives_the_words_of_the_coefficient_route(emul, rot_emul, K, N):
    """whole rows of both components, R = 1 and 3 rotations (no sign flip, every sign but one, many wraps), with and without the bias;
    random words, every word q - 1 and every word 0"""
    level = 3
    w = _mixed_ring(K, N)
    nw = level + K
    rng = np.random.default_rng(100 * K + N)
    wa = np.array(w, dtype=np.uint64).reshape(nw, 1)
    for gs in ([5], [1, 2 * N - 1, pow(3, N // 2 + 3, 2 * N)]):
        R = len(gs)
        rand = H.rand_residues(rng, w, (R, 2), N).reshape(R, 2, nw, N)
        edge = np.broadcast_to(wa - np.uint64(1), (R, 2, nw, N)).copy()
        zero = np.zeros((R, 2, nw, N), dtype=np.uint64)
        F = H.rand_residues(rng, w[:level], (2,), N).reshape(2, level, N)
        Fe = np.broadcast_to(wa[:level] - np.uint64(1), (2, level, N)).copy()
        bias = H.rand_residues(rng, w[:level], (), N).reshape(level, N)
        for T, f, b in ((rand, F, None), (rand, F, bias), (edge, Fe, Fe[0]), (zero, np.zeros_like(F), None), (edge, np.zeros_like(F), None)):
            _fold_step_both_ways(emul, rot_emul, K, N, level, w, gs, T, f, b)


def test_ragged_last_digit_oracle_step_is_rotations_then_sum():
    """level 3 in digits of two limbs (the last digit ragged), K = 2, N = 16: one step of three keys and one of one, against the
    rotations added one by one"""
    N, level, k, alpha = 16, 3, 2, 2
    qs = H.chain(30, level + k, N)
    ref = ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(7)
    gs = [[3, 2 * N - 1, 5], [9]]
    ks = [[H.uniform_evk(rng, qs, 2, N) for _ in st] for st in gs]
    ct = H.rand_residues(rng, qs[:level], (2, 2), N)
    got = FO.rotate_sum_grouped_ref(ref, level, k, alpha, ks, gs, ct)
    from tests import ks_grouped_oracle as KO
    q = np.array(qs[:level], dtype=object).reshape(1, 1, level, 1)
    f = ct
    for evks, st in zip(ks, gs):
        t = f.astype(object)
        for e, g in zip(evks, st):
            t = (t + KO.rotate_grouped_ref(ref, level, k, alpha, e, g, f).astype(object)) % q
        f = t.astype(np.uint64)
    assert np.array_equal(got, f)


# ---- the host checks ----------------------------------------------------------------------------------------------------------

def test_every_host_check_in_the_headers_order(emul):
    """ks_group_fold_check (csrc/ks_group_core.h), the function both entry points run first, on a ring of L = 8 limbs and N = 64: every
    call breaks one rule and later ones too where it can, and must report the earliest"""
    msg = C.create_string_buffer(200)
    N = 64
    ct_bytes = 2 * 4 * N * 8          # batch 1, level 4
    CT, DG, OUT, BIAS = 1 << 20, 1 << 24, 1 << 28, 1 << 30

    def call(product=1, null=0, Lk=6, level=4, k=2, group=2, nd=2, batch=1, baby=(0, 0), bgs=(3, 5), giant=(0,), ggs=(127,), n_baby=None, n_giant=None,
             diags=(DG,), cts=(CT,), n_in=None, fold=(), fgs=(9, 11, 13), sizes=(2, 1), n_steps=None, bias=0, out=OUT):
        n_baby = len(baby) if n_baby is None else n_baby
        n_giant = len(giant) if n_giant is None else n_giant
        n_in = len(cts) if n_in is None else n_in
        n_steps = len(sizes) if n_steps is None else n_steps
        arr = lambda t, xs: (t * max(1, len(xs)))(*xs)
        ba, ga = arr(C.c_int, baby), arr(C.c_int, giant)
        bg, gg = arr(C.c_uint64, bgs), arr(C.c_uint64, ggs)
        da, ca = arr(C.c_uint64, diags), arr(C.c_uint64, cts)
        fa = (C.c_int * 64)(*fold)
        fg = (C.c_uint64 * 64)(*(list(fgs) + [3] * (64 - len(fgs))))
        fs = arr(C.c_int, sizes)
        nothing = C.c_int(-1)
        rc = emul.mdg_fold_emul_check(product, null, 8, N, Lk, level, k, group, nd, batch, C.addressof(ba), C.addressof(bg), n_baby, C.addressof(ga),
                                      C.addressof(gg), n_giant, C.addressof(da), C.addressof(ca), n_in, C.addressof(fa), C.addressof(fg),
                                      C.addressof(fs), n_steps, bias, out, C.addressof(nothing), msg, len(msg))
        return rc, msg.value.decode(), nothing.value
    for product in (1, 0):
        assert call(product=product) == (native.OK, "", 0)
        # 1. a null array or operand, ahead of everything
        assert call(product=product, null=1, n_steps=70, Lk=0, batch=-1, n_giant=70)[:2] == (native.E_BADARG, "null argument")
        # 2. the fold's host rules, ahead of the product's and of the shapes
        for kw, word in ((dict(n_steps=-1), "n_fold_groups=-1 outside"), (dict(sizes=(1,) * 65), "n_fold_groups=65 outside"),
                         (dict(sizes=(2, 0)), "fold group 1 has size 0, below 1"), (dict(sizes=(60, 5)), "more than 64 fold keys"),
                         (dict(sizes=(65,)), "more than 64 fold keys"), (dict(fold=(0, 0, 1)), "null fold key 2")):
            rc, m, _ = call(product=product, Lk=0, baby=(1, 0), n_in=0, **kw)
            assert rc == native.E_BADARG and word in m, (kw, m)
        assert call(product=product, sizes=(64,))[0] == native.OK and call(product=product, sizes=(1,) * 64)[0] == native.OK
        assert call(product=product, fold=(0, 0, 0, 1))[0] == native.OK                # a null pointer past the keys in use is not read
    # 3. the product's null keys and counts, ahead of the shapes
    rc, m, _ = call(baby=(0, 1), n_giant=70, Lk=0)
    assert rc == native.E_BADARG and "null baby key 1" in m
    rc, m, _ = call(giant=(1,), n_in=0, Lk=0)
    assert rc == native.E_BADARG and "null giant key 0" in m
    rc, m, _ = call(diags=(DG, 0), cts=(CT, 0), n_baby=-1)
    assert rc == native.E_BADARG and "null diagonals of input 1" in m
    rc, m, _ = call(diags=(DG, DG), cts=(CT, 0), n_baby=-1)
    assert rc == native.E_BADARG and "null ciphertext of input 1" in m
    for kw, word in ((dict(n_baby=-1), "n_baby"), (dict(baby=(0,) * 65, bgs=(3,) * 65), "n_baby"), (dict(n_giant=-1), "n_giant"),
                     (dict(giant=(0,) * 65, ggs=(3,) * 65), "n_giant"), (dict(n_in=0), "n_in"), (dict(diags=(DG,) * 65, cts=(CT,) * 65), "n_in")):
        rc, m, _ = call(Lk=0, **kw)
        assert rc == native.E_BADARG and word in m and "outside" in m, (kw, m)
    assert call(product=0, baby=(1,), n_baby=-1, n_giant=70, n_in=0)[0] == native.OK    # the fold alone looks at none of them
    # 4. per key in turn (baby, giant, fold) the shape checks of tfhe_rotate_grouped in its order
    for product in (1, 0):
        rc, m, _ = call(product=product, Lk=0, fgs=(4, 4, 4))
        assert rc == native.E_BADARG and "key_limbs" in m
        rc, m, _ = call(product=product, k=5, group=0, level=0, nd=0, batch=-1, fgs=(4, 4, 4))
        assert rc == native.E_BADARG and "n_special" in m
        rc, m, _ = call(product=product, group=0, level=0, nd=0, batch=-1)
        assert rc == native.E_BADARG and "group" in m
        rc, m, _ = call(product=product, level=5, nd=0, batch=-1)
        assert rc == native.E_LEVEL and "level" in m
        rc, m, _ = call(product=product, nd=1, batch=-1, fgs=(4, 4, 4))
        assert rc == native.E_PARAMS and "components" in m
        rc, m, _ = call(product=product, batch=-1, fgs=(4, 4, 4))
        assert rc == native.E_BADARG and "negative batch" in m
        for g in (0, 4, 2 * N, 2 * N + 1):
            rc, m, _ = call(product=product, out=CT, fgs=(9, 11, g))
            assert rc == native.E_BADARG and "odd and below 2N" in m, (product, g)     # ahead of the overlap
        rc, m, _ = call(product=product, baby=(), bgs=(), giant=(), ggs=(), sizes=(), level=5)
        assert rc == native.E_LEVEL and "level" in m                                   # no key at all: the shape checks run once
    for g in (0, 4, 2 * N):
        for kw in (dict(bgs=(3, g)), dict(ggs=(g,))):
            rc, m, _ = call(out=CT, **kw)
            assert rc == native.E_BADARG and "odd and below 2N" in m, (g, kw)
    assert call(product=0, bgs=(4, 4), ggs=(4,))[0] == native.OK
    # 5. out against every operand: anywhere, the last word included
    d_bytes = 2 * 3 * 4 * N * 8       # [n_giant + 1][n_baby + 1][level][N]
    for product in (1, 0):
        for out in (CT, CT + ct_bytes - 8, CT - ct_bytes + 8):
            rc, m, _ = call(product=product, out=out)
            assert rc == native.E_BADARG and "overlaps" in m, out
        assert call(product=product, out=CT + ct_bytes)[0] == native.OK
    for out in (DG, DG + d_bytes - 8, DG - ct_bytes + 8):
        rc, m, _ = call(out=out)
        assert rc == native.E_BADARG and "overlaps" in m, out
    assert call(product=0, out=DG)[0] == native.OK
    for out in (BIAS, BIAS + 4 * N * 8 - 8, BIAS - ct_bytes + 8):
        rc, m, _ = call(out=out, bias=BIAS)
        assert rc == native.E_BADARG and "overlaps" in m, out
    rc, m, _ = call(diags=(DG, DG + d_bytes), cts=(CT, CT), out=DG + 2 * d_bytes - 8)
    assert rc == native.E_BADARG and "overlaps" in m                                   # the second input's diagonals
    assert call(out=DG + d_bytes)[0] == native.OK and call(out=BIAS - ct_bytes, bias=BIAS)[0] == native.OK
    # accepted: no fold step, no baby or giant step, a repeated input
    assert call(sizes=()) == (native.OK, "", 0)
    assert call(baby=(), bgs=(), giant=(), ggs=()) == (native.OK, "", 0)
    assert call(baby=(), bgs=(), giant=(), ggs=(), sizes=()) == (native.OK, "", 0)
    assert call(diags=(DG, DG), cts=(CT, CT)) == (native.OK, "", 0)
    # an empty batch: every check, then nothing to do
    for product in (1, 0):
        assert call(product=product, batch=0) == (native.OK, "", 1)
        assert call(product=product, batch=0, fgs=(4,))[0] == native.E_BADARG
        assert call(product=product, batch=0, out=CT)[0] == native.E_BADARG


# ---- the code objects -----------------------------------------------------------------------------------------------------------

@KH.needs_hipcc
def test_gfx950_code_objects_use_no_scratch(tmp_path):
    """k_mdg_fold_finish<1..4, 1..2> keeps a block of TFHE_MDG_FOLD_JB limbs and K special words per coefficient in registers and its
    constants in static LDS; k_mdg_fold_gather is k_md_fold without a stream.  No scratch in any of them; the register and LDS counts
    are printed for the record, without a threshold"""
    found = KH.probe_all("mdg_fold_emul/resource_probe.hip", tmp_path, [(f"PROBE_K={K}",) for K in (1, 2, 3, 4)])
    recs = [r for kernels in found for r in kernels]
    finish = {r["name"]: r for r in recs if "k_mdg_fold_finishILi" in r["name"]}
    gather = [r for r in recs if "k_mdg_fold_gather" in r["name"]]
    assert len(finish) == 8 and len(gather) == 4, sorted(r["name"] for r in recs if "mdg_fold" in r["name"])
    for r in list(finish.values()) + gather[:1]:
        print(r["name"], r)
        assert r["scratch"] == 0, r
    assert all(r["static_lds"] > 0 for r in finish.values())


# ---- the mirror -------------------------------------------------------------------------------------------------------------------

def test_mirror_argument_rules():
    qs = H.chain(30, 6, 64)
    ring = types.SimpleNamespace(L=len(qs), moduli=list(qs), N=64)
    inner = types.SimpleNamespace(relin_window=0, sigma=3.2, scheme_name="CKKS", R_key=lambda: ring, R_cipher=lambda: ring)
    gp = she.GroupedRaised(inner, 2, 2)
    gk = she.GaloisKey(3, types.SimpleNamespace(params=gp, key=[None]))
    plain = she.GaloisKey(3, types.SimpleNamespace(params=inner, key=[None]))
    for call in (lambda: she.rotate_sum_grouped([[plain]], [0, 0]), lambda: she.rotate_sum_grouped([[gk], [plain]], [0, 0]),
                 lambda: she.matmul_bsgs_fold_grouped([gk], [], [[[0, 0]]], [[0, 0]], [[plain]]),
                 lambda: she.matmul_bsgs_fold_grouped([plain], [], [[[0, 0]]], [[0, 0]], [[gk]])):
        with pytest.raises(she.UsageError, match="one parameter set with grouped digits"):
            call()
    with pytest.raises(she.UsageError, match="no Galois key at all"):
        she.matmul_bsgs_fold_grouped([], [], [[0]], [[0, 0]], [])
    with pytest.raises(she.UsageError, match="a fold step without a key"):
        she.rotate_sum_grouped([[gk], []], [0, 0])
    with pytest.raises(she.UsageError, match="a fold step without a key"):
        she.matmul_bsgs_fold_grouped([gk], [], [[[0, 0]]], [[0, 0]], [[]])
    with pytest.raises(she.UsageError, match="at most 64 fold steps"):
        she.rotate_sum_grouped([[gk]] * 65, [0, 0])
    # the per-limb mirror functions still refuse grouped keys
    for call in (lambda: she.rotate_sum([[gk]], [0, 0]), lambda: she.matmul_bsgs_fold([], [], [[[0]]], [[0, 0]], [[gk]])):
        with pytest.raises(she.UsageError, match="grouped digits"):
            call()
