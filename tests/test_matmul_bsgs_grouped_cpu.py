"""No-GPU checks of the product by baby and giant steps on grouped-digit keys (tfhe_matmul_bsgs_grouped) and of the evaluation-domain
rotation phase under it: the symbol is declared, exported, bound by ctypes and by the Julia shim with one signature; the oracle
(tests/matmul_bsgs_grouped_oracle.py) against tests/matmul_oracle.matmul_bsgs_blocks_ref in the two degenerate cases; the
per-coefficient body of k_mdg_lift<K, V> (csrc/ks_group_core.h mdg_lift_coeff), run on the CPU over whole rows (tests/mdg_lift_emul/),
against Python integers and against the coefficient-domain tail it replaces; the host checks in the header's order, on plain numbers;
the gfx950 code objects' scratch; and the mirror's argument rules."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest

from oracle import ref_cpu
from tests import helpers as H
from tests import kernel_harness as KH
from tests import matmul_bsgs_grouped_oracle as BO
from tests import matmul_oracle as MO
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native, she

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfhe_matmul_bsgs_grouped"
# (ctx, key_limbs, level, n_special, group, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, n_digits, diags, cts, n_in, bias, out, batch)
CLASSES = ["ptr", "int", "int", "int", "int", "ptr", "ptr", "int", "ptr", "ptr", "int", "int", "ptr", "ptr", "int", "ptr", "ptr", "i64"]


# ---- one signature everywhere --------------------------------------------------------------------------------------------

def test_symbol_declared_exported_and_bound_with_one_signature():
    protos = shim.header_prototypes()
    assert NAME in protos, f"{NAME} is not declared in include/toyfhe_hip.h"
    assert protos[NAME] == ("int", CLASSES)
    assert NAME in native.EXPORTED_SYMBOLS
    f = getattr(native.lib(), NAME)                      # AttributeError: not exported by the library
    assert f.restype is C.c_int and len(f.argtypes) == len(CLASSES)
    for k, t in zip(CLASSES, f.argtypes):
        if k == "ptr":
            assert t is C.c_void_p or issubclass(t, C._Pointer), (k, t)
        else:
            assert t is {"int": C.c_int, "i64": C.c_int64}[k], (k, t)
    assert callable(native.Context.matmul_bsgs_grouped)
    import toyfhe_jl_amd as tf
    assert callable(tf.matmul_bsgs_grouped) and callable(tf.matmul_bsgs_blocks_grouped)
    calls = [c for c in shim.shim_ccalls() if c[0] == NAME]
    assert len(calls) == 1, f"the shim binds {NAME} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == CLASSES and nargs == len(CLASSES)


def test_header_states_the_contract_and_what_is_still_refused():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index(f"int {NAME}(")
    doc = text[text.rindex("/*", 0, i):i]
    for word in ("tfhe_galois_key_prepare", "HOST array", "word for word", "tfhe_rotate_many_grouped", "tfhe_rotate_grouped", "TFHE_MD_COEFF",
                 "in this order", "batch == 0", "untouched", "tfhe_matmul_bsgs_blocks", "tfhe_matmul_diag_grouped"):
        assert word in doc, word
    order = [doc.index(w) for w in ("a null ctx", "a null key among", "outside", "shape checks", "overlapping anywhere")]
    assert order == sorted(order), order
    for word in ("tfhe_rotate_sum", "tfhe_matmul_bsgs_fold", "fused N <= 2^14 key switch"):
        assert word in text[text.index("Still refused on grouped keys"):i], word


def test_a_null_argument_is_refused_by_the_library_before_any_device_use():
    lib = native.lib()
    buf = np.zeros(8, dtype=np.uint64).ctypes.data
    keys = (C.c_void_p * 2)(buf, None)
    gs = (C.c_uint64 * 2)(4, 3)
    rc = lib.tfhe_matmul_bsgs_grouped(None, 0, 0, 9, 0, keys, gs, 70, keys, gs, -1, 0, keys, keys, 0, None, buf, -1)
    assert rc == native.E_BADARG and "null argument" in lib.tfhe_last_error().decode()


# ---- the oracle in the two degenerate cases --------------------------------------------------------------------------------

@pytest.mark.parametrize("special", [1, 0])
def test_oracle_with_one_limb_per_digit_is_the_per_limb_oracle(special):
    """(k, alpha) = (1, 1) is ModulusRaised with one special prime, (0, 1) the plain RNS gadget: the words of matmul_bsgs_blocks_ref"""
    N, Lk = 16, 4
    qs = H.chain(30, Lk, N)
    ref = ref_cpu.RefCtx(N, qs)
    level = Lk - special
    rng = np.random.default_rng(special)
    nb, ng, nin, batch = 2, 2, 2, 2
    bgs, ggs = [3, 2 * N - 1], [5, 9]
    bk = [H.uniform_evk(rng, qs, level, N) for _ in bgs]
    gk = [H.uniform_evk(rng, qs, level, N) for _ in ggs]
    diags = [H.rand_residues(rng, qs[:level], (ng + 1, nb + 1), N) for _ in range(nin)]
    cts = [H.rand_residues(rng, qs[:level], (batch, 2), N) for _ in range(nin)]
    bias = H.rand_residues(rng, qs[:level], (), N)
    for b in (None, bias):
        want = MO.matmul_bsgs_blocks_ref(ref, level, special, bk, bgs, gk, ggs, diags, cts, bias=b)
        got = BO.matmul_bsgs_blocks_grouped_ref(ref, level, special, 1, bk, bgs, gk, ggs, diags, cts, bias=b)
        assert np.array_equal(got, want), (special, b is not None)


# ---- the emulation ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = KH.build_emul("mdg_lift_emul/mdg_lift_emul.cpp", tmp_path_factory.mktemp("mdg_lift_emul"))
    vp, i32, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    L.mdg_lift_emul_rows.argtypes, L.mdg_lift_emul_rows.restype = [i32, i32, vp, C.c_long, vp, vp, vp], i32
    L.mdg_lift_emul_check.argtypes = [i32, i32, i64, i32, i32, i32, i32, i32, i64, vp, vp, i32, vp, vp, i32, vp, vp, i32, u64, u64, vp, C.c_char_p,
                                      C.c_size_t]
    L.mdg_lift_emul_check.restype = i32
    return L


@pytest.fixture(scope="module")
def rot_emul(tmp_path_factory):
    L = KH.build_emul("ks_group_rot_emul/ks_group_rot_emul.cpp", tmp_path_factory.mktemp("ks_group_rot_emul_for_mdg"))
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    L.ks_group_rot_emul_tail.argtypes, L.ks_group_rot_emul_tail.restype = [i32, i32, vp, C.c_long, u64, vp, vp, vp], i32
    return L


def _mixed_ring(K, N):
    """level = 3 ciphertext limbs of 30, 50 and 61 bits, then K special primes of 61, 30, 50 and 61 bits: every size on both sides"""
    p30, p50, p61 = H.chain(30, 2, N), H.chain(50, 2, N), H.chain(61, 3, N)
    return [p30[0], p50[0], p61[0]] + [p61[1], p30[1], p50[1], p61[2]][:K]


def _lift(emul, K, level, w, special_rows):
    N = special_rows.shape[1]
    wa = np.array(w, dtype=np.uint64)
    sp = np.ascontiguousarray(special_rows, dtype=np.uint64)
    u = np.full((level, N), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    pinv = np.zeros(level, dtype=np.uint64)
    assert emul.mdg_lift_emul_rows(K, level, wa.ctypes.data, N, sp.ctypes.data, u.ctypes.data, pinv.ctypes.data) == 0
    assert (u < wa[:level].reshape(level, 1)).all()
    return u, [int(x) for x in pinv]


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_lift_body_is_the_floor_by_the_special_primes_on_python_integers(emul, K):
    """for an integer x in [0, Q P) given by its residues over the working limbs: x_j Pinv_j - U_j = floor(x / P) mod q_j.  x = 0, P - 1,
    P, Q P - 1, the integer with every residue q - 1, a multiple of P (every special residue 0), and random ones, over whole rows"""
    N, level = 64, 3
    w = _mixed_ring(K, N)
    Q, P = math.prod(w[:level]), math.prod(w[level:])
    rng = np.random.default_rng(K)
    minus1 = (Q * P - 1)                                                     # -1 mod every limb: every residue q - 1
    xs = [0, P - 1, P, Q * P - 1, minus1, P * int(rng.integers(1, 1 << 60)) % (Q * P)]
    xs += [int.from_bytes(rng.bytes(48), "little") % (Q * P) for _ in range(N - len(xs))]
    assert all(minus1 % q == q - 1 for q in w) and all(xs[5] % p == 0 for p in w[level:])
    sp = np.array([[x % p for x in xs] for p in w[level:]], dtype=np.uint64)
    u, pinv = _lift(emul, K, level, w, sp)
    for j in range(level):
        q = w[j]
        assert pinv[j] == pow(P, -1, q)
        for i, x in enumerate(xs):
            assert ((x % q) * pinv[j] - int(u[j, i])) % q == (x // P) % q, (K, j, i)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_lift_body_gives_the_words_of_the_coefficient_tail(emul, rot_emul, K):
    """ks_group_rot_tail_coeff<K> at g = 1 (no permutation, no sign, no addend) is tail_j(t_j) on ANY canonical words, consistent with
    one integer or not: t_j Pinv_j - U_j, word for word.  Random rows, every word q - 1, and every special word 0"""
    N, level = 64, 3
    w = _mixed_ring(K, N)
    nw = level + K
    wa = np.array(w, dtype=np.uint64)
    rng = np.random.default_rng(10 + K)
    edge = np.broadcast_to(wa.reshape(nw, 1) - np.uint64(1), (nw, N)).copy()
    zero_special = H.rand_residues(rng, w, (), N).reshape(nw, N)
    zero_special[level:] = 0
    for t in (H.rand_residues(rng, w, (), N).reshape(nw, N), edge, zero_special):
        t = np.ascontiguousarray(t)
        want = np.full((level, N), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        assert rot_emul.ks_group_rot_emul_tail(K, level, wa.ctypes.data, N, 1, t.ctypes.data, None, want.ctypes.data) == 0
        u, pinv = _lift(emul, K, level, w, t[level:])
        for j in range(level):
            got = (t[j].astype(object) * pinv[j] - u[j].astype(object)) % w[j]
            assert np.array_equal(got.astype(np.uint64), want[j]), (K, j)


# ---- the host checks ----------------------------------------------------------------------------------------------------------

def test_every_host_check_in_the_headers_order(emul):
    """ks_group_bsgs_check (csrc/ks_group_core.h), the function the entry point runs first, on a ring of L = 8 limbs and N = 64: every
    call breaks one rule and later ones too where it can, and must report the earliest"""
    msg = C.create_string_buffer(200)
    N = 64
    ct_bytes = 2 * 4 * N * 8          # batch 1, level 4
    CT, DG, OUT, BIAS = 1 << 20, 1 << 24, 1 << 28, 1 << 30

    def call(null=0, Lk=6, level=4, k=2, group=2, nd=2, batch=1, baby=(0, 0), bgs=(3, 5), giant=(0,), ggs=(127,), n_baby=None, n_giant=None,
             diags=(DG,), cts=(CT,), n_in=None, bias=0, out=OUT):
        n_baby = len(baby) if n_baby is None else n_baby
        n_giant = len(giant) if n_giant is None else n_giant
        n_in = len(cts) if n_in is None else n_in
        arr = lambda t, xs: (t * max(1, len(xs)))(*xs)
        ba, ga = arr(C.c_int, baby), arr(C.c_int, giant)
        bg, gg = arr(C.c_uint64, bgs), arr(C.c_uint64, ggs)
        da, ca = arr(C.c_uint64, diags), arr(C.c_uint64, cts)
        nothing = C.c_int(-1)
        rc = emul.mdg_lift_emul_check(null, 8, N, Lk, level, k, group, nd, batch, C.addressof(ba), C.addressof(bg), n_baby, C.addressof(ga),
                                      C.addressof(gg), n_giant, C.addressof(da), C.addressof(ca), n_in, bias, out, C.addressof(nothing), msg, len(msg))
        return rc, msg.value.decode(), nothing.value
    assert call() == (native.OK, "", 0)
    # 1. a null array or operand, ahead of everything
    assert call(null=1, baby=(1, 0), bgs=(4, 3), Lk=0, batch=-1, n_giant=70)[:2] == (native.E_BADARG, "null argument")
    # 2. a null key / operand among the first valid count, ahead of the counts and the shapes
    rc, m, _ = call(baby=(0, 1), n_giant=70, Lk=0)
    assert rc == native.E_BADARG and "null baby key 1" in m
    rc, m, _ = call(giant=(1,), n_in=0, Lk=0)
    assert rc == native.E_BADARG and "null giant key 0" in m
    rc, m, _ = call(diags=(DG, 0), cts=(CT, 0), n_baby=-1)
    assert rc == native.E_BADARG and "null diagonals of input 1" in m
    rc, m, _ = call(diags=(DG, DG), cts=(CT, 0), n_baby=-1)
    assert rc == native.E_BADARG and "null ciphertext of input 1" in m
    # 3. the counts
    for kw, word in ((dict(n_baby=-1), "n_baby"), (dict(baby=(0,) * 65, bgs=(3,) * 65), "n_baby"), (dict(n_giant=-1), "n_giant"),
                     (dict(giant=(0,) * 65, ggs=(3,) * 65), "n_giant"), (dict(n_in=0), "n_in"), (dict(diags=(DG,) * 65, cts=(CT,) * 65), "n_in")):
        rc, m, _ = call(Lk=0, **kw)
        assert rc == native.E_BADARG and word in m and "outside" in m, (kw, m)
    assert call(baby=(0,) * 64, bgs=(3,) * 64, giant=(0,) * 64, ggs=(5,) * 64, diags=(DG,) * 64, cts=(CT,) * 64)[0] == native.OK
    # 4. per key in turn (baby, then giant) the shape checks of tfhe_rotate_grouped in its order
    rc, m, _ = call(Lk=0, bgs=(4, 4))
    assert rc == native.E_BADARG and "key_limbs" in m
    rc, m, _ = call(k=5, group=0, level=0, nd=0, batch=-1, bgs=(4, 4))
    assert rc == native.E_BADARG and "n_special" in m
    rc, m, _ = call(group=0, level=0, nd=0, batch=-1)
    assert rc == native.E_BADARG and "group" in m
    rc, m, _ = call(level=5, nd=0, batch=-1)
    assert rc == native.E_LEVEL and "level" in m
    rc, m, _ = call(nd=1, batch=-1, bgs=(4, 4))
    assert rc == native.E_PARAMS and "components" in m
    rc, m, _ = call(batch=-1, bgs=(4, 4))
    assert rc == native.E_BADARG and "negative batch" in m
    for g in (0, 4, 2 * N, 2 * N + 1):
        for kw in (dict(bgs=(3, g)), dict(ggs=(g,))):
            rc, m, _ = call(out=CT, **kw)
            assert rc == native.E_BADARG and "odd and below 2N" in m, (g, kw)          # ahead of the overlap
    rc, m, _ = call(baby=(), bgs=(), giant=(), ggs=(), level=5)
    assert rc == native.E_LEVEL and "level" in m                                       # no key at all: the shape checks run once
    # 5. out against every operand: anywhere, the last word included
    d_bytes = 2 * 3 * 4 * N * 8       # [n_giant + 1][n_baby + 1][level][N]
    for out in (CT, CT + ct_bytes - 8, CT - ct_bytes + 8, DG, DG + d_bytes - 8, DG - ct_bytes + 8):
        rc, m, _ = call(out=out)
        assert rc == native.E_BADARG and "overlaps" in m, out
    for out in (BIAS, BIAS + 4 * N * 8 - 8, BIAS - ct_bytes + 8):
        rc, m, _ = call(out=out, bias=BIAS)
        assert rc == native.E_BADARG and "overlaps" in m, out
    rc, m, _ = call(diags=(DG, DG + d_bytes), cts=(CT, CT), out=DG + 2 * d_bytes - 8)
    assert rc == native.E_BADARG and "overlaps" in m                                   # the second input's diagonals
    assert call(out=CT + ct_bytes)[0] == native.OK and call(out=DG + d_bytes)[0] == native.OK and call(out=BIAS - ct_bytes, bias=BIAS)[0] == native.OK
    # accepted: no giant step, no baby step, a repeated key (the flags only say "not null"), a repeated input
    assert call(giant=(), ggs=()) == (native.OK, "", 0)
    assert call(baby=(), bgs=()) == (native.OK, "", 0)
    assert call(baby=(), bgs=(), giant=(), ggs=()) == (native.OK, "", 0)
    assert call(diags=(DG, DG), cts=(CT, CT)) == (native.OK, "", 0)
    # an empty batch: every check, then nothing to do
    assert call(batch=0) == (native.OK, "", 1)
    assert call(batch=0, ggs=(4,))[0] == native.E_BADARG
    assert call(batch=0, out=CT)[0] == native.E_BADARG


# ---- the code objects -----------------------------------------------------------------------------------------------------------

@KH.needs_hipcc
def test_gfx950_code_objects_use_no_scratch(tmp_path):
    """k_mdg_lift<1..4, 1..2> keeps K words per coefficient in registers and its constants in static LDS; k_mdg_special_perm is a gather.
    No scratch in any of them; the register counts are printed for the record, without a threshold"""
    recs = KH.kernel_resources("mdg_lift_emul/resource_probe.hip", tmp_path)
    lift = {r["name"]: r for r in recs if "k_mdg_liftILi" in r["name"]}
    perm = [r for r in recs if "k_mdg_special_perm" in r["name"]]
    assert len(lift) == 8 and len(perm) == 1, sorted(r["name"] for r in recs if "mdg" in r["name"])
    for r in list(lift.values()) + perm:
        print(r["name"], r)
        assert r["scratch"] == 0, r
    assert all(r["static_lds"] > 0 for r in lift.values())


# ---- the mirror -------------------------------------------------------------------------------------------------------------------

def test_mirror_argument_rules():
    qs = H.chain(30, 6, 64)
    ring = types.SimpleNamespace(L=len(qs), moduli=list(qs), N=64)
    inner = types.SimpleNamespace(relin_window=0, sigma=3.2, scheme_name="CKKS", R_key=lambda: ring, R_cipher=lambda: ring)
    gp = she.GroupedRaised(inner, 2, 2)
    gk = she.GaloisKey(3, types.SimpleNamespace(params=gp, key=[None]))
    plain = she.GaloisKey(3, types.SimpleNamespace(params=inner, key=[None]))
    for call in (lambda: she.matmul_bsgs_grouped([plain], [], [[0, 0]], [0, 0]), lambda: she.matmul_bsgs_blocks_grouped([gk], [plain], [[[0, 0]] * 2], [[0, 0]])):
        with pytest.raises(she.UsageError, match="one parameter set with grouped digits"):
            call()
    with pytest.raises(she.UsageError, match="no Galois key at all"):
        she.matmul_bsgs_grouped([], [], [[0]], [0, 0])
