"""No-GPU checks of the hoisted rotations and the diagonal product on grouped-digit keys (tfhe_rotate_many_grouped,
tfhe_matmul_diag_grouped): the two symbols are declared, exported, bound by ctypes and by the Julia shim with one signature; the
per-coefficient body of k_ks_group_rot_tail<K> (csrc/ks_group_core.h), run on the CPU over whole rows (tests/ks_group_rot_emul/),
against galois -> modswitch^K -> + galois(c) of the C oracle; the identity the hoisting rests on -- the grouped digits commute with the
automorphism -- on the emulated digit bodies; the host checks of both entry points in the header's order, on plain numbers; the
gfx950 code objects' registers, scratch and LDS; and the mirror's argument rules."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest

from oracle import ref_cpu
from tests import helpers as H
from tests import kernel_harness as KH
from tests import ks_grouped_oracle as KO
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native, she

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ctx, key_limbs, level, n_special, group, evks, n_digits, galois_elements, n_rot, ct, out, batch)
MANY = ("tfhe_rotate_many_grouped", ["ptr", "int", "int", "int", "int", "ptr", "int", "ptr", "int", "ptr", "ptr", "i64"])
# (ctx, key_limbs, level, n_special, group, evks, n_digits, galois_elements, n_rot, diags, ct, out, batch)
DIAG = ("tfhe_matmul_diag_grouped", ["ptr", "int", "int", "int", "int", "ptr", "int", "ptr", "int", "ptr", "ptr", "ptr", "i64"])


# ---- one signature everywhere --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,classes", [MANY, DIAG])
def test_symbols_declared_exported_and_bound_with_one_signature(name, classes):
    protos = shim.header_prototypes()
    assert name in protos, f"{name} is not declared in include/toyfhe_hip.h"
    assert protos[name] == ("int", classes)
    assert name in native.EXPORTED_SYMBOLS
    f = getattr(native.lib(), name)                      # AttributeError: not exported by the library
    assert f.restype is C.c_int and len(f.argtypes) == len(classes)
    for k, t in zip(classes, f.argtypes):
        if k == "ptr":
            assert t is C.c_void_p or issubclass(t, C._Pointer), (k, t)
        else:
            assert t is {"int": C.c_int, "i64": C.c_int64}[k], (k, t)
    assert callable(getattr(native.Context, name[len("tfhe_"):]))
    import toyfhe_jl_amd as tf
    assert callable(getattr(tf, name[len("tfhe_"):])) and callable(she.GaloisKey.prepared_grouped)


@pytest.mark.parametrize("name,classes", [MANY, DIAG])
def test_julia_shim_binds_the_same_signature(name, classes):
    calls = [c for c in shim.shim_ccalls() if c[0] == name]
    assert len(calls) == 1, f"the shim binds {name} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == classes and nargs == len(classes)
    src = open(shim.SHIM).read()
    body = src[src.index(f"function {name[len('tfhe_'):]}("):]
    body = body[:body.index("\nend")]
    assert "GC.@preserve" in body and "on(ctx" in body and "batchsize(c)" in body and "prepared(gk)" in body


def test_header_states_the_contract_and_the_order_of_the_checks():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index("int tfhe_rotate_many_grouped(")
    doc = text[text.rindex("/*", 0, i):i]
    for word in ("tfhe_galois_key_prepare", "HOST array", "[n_rot][batch][2][level][N]", "[n_rot + 1][level][N]", "word for word", "tiles of 64",
                 "BEFORE", "tfhe_rotate_many_grouped ->", "tfhe_nntt -> tfhe_dot", "in this order", "batch == 0", "tfhe_matmul_bsgs*", "tfhe_rotate_sum",
                 "tfhe_mul_relin"):
        assert word in doc, word
    order = [doc.index(w) for w in ("a null ctx", "n_rot > 64", "for r = 0, 1, .. in turn", "overlapping")]
    assert order == sorted(order), order
    assert text.index("int tfhe_matmul_diag_grouped(") > i > text.index("int tfhe_rotate_grouped(")


def test_a_null_argument_is_refused_by_the_library_before_any_device_use():
    """no context and host pointers: each call also breaks later rules and must report the first"""
    lib = native.lib()
    buf = np.zeros(8, dtype=np.uint64).ctypes.data
    keys = (C.c_void_p * 2)(buf, None)
    gs = (C.c_uint64 * 2)(4, 3)
    err = lambda: lib.tfhe_last_error().decode()
    for args in ((None, 3, 2, 1, 1, keys, 2, gs, 2, buf, buf, 1), (None, 0, 0, 9, 0, keys, 0, gs, -1, buf, buf, -1)):
        assert lib.tfhe_rotate_many_grouped(*args) == native.E_BADARG and "null argument" in err()
    assert lib.tfhe_matmul_diag_grouped(None, 3, 2, 1, 1, keys, 2, gs, 65, buf, buf, buf, 1) == native.E_BADARG and "null argument" in err()


# ---- the emulation ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = KH.build_emul("ks_group_rot_emul/ks_group_rot_emul.cpp", tmp_path_factory.mktemp("ks_group_rot_emul"))
    vp, i32, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    L.ks_group_rot_emul_tail.argtypes, L.ks_group_rot_emul_tail.restype = [i32, i32, vp, C.c_long, u64, vp, vp, vp], i32
    L.ks_group_rot_emul_digits.argtypes, L.ks_group_rot_emul_digits.restype = [i32, i32, vp, i32, vp, C.c_long, vp, vp], i32
    L.ks_group_rot_emul_check.argtypes = [i32, i32, i32, i64, i32, i32, i32, i32, i32, i64, vp, vp, i32, u64, u64, u64, vp, C.c_char_p, C.c_size_t]
    L.ks_group_rot_emul_check.restype = i32
    return L


def _galois_elements(N):
    return [1, 2 * N - 1, 5, pow(3, N // 2 + 3, 2 * N)]


# ---- the tail body --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("ct_bits,sp_bits", [(40, 30), (30, 50), (61, 30)])
def test_tail_body_is_galois_then_k_modswitch_steps_then_the_rotated_addend(emul, K, ct_bits, sp_bits):
    """special primes below and above the ciphertext limbs; g = 1 flips no sign, g = 2N - 1 every one but index 0; random words and
    every word q - 1; with the addend (component 0) and without (component 1)"""
    N, level = 64, 3
    w = H.chain(ct_bits, level, N) + H.chain(sp_bits, K, N)
    nw = level + K
    ref = ref_cpu.RefCtx(N, w)
    rng = np.random.default_rng(10 * K + ct_bits)
    wa = np.array(w, dtype=np.uint64)
    ql = np.array(w[:level], dtype=object).reshape(level, 1)
    for edge in (False, True):
        if edge:
            t = np.broadcast_to(wa.reshape(nw, 1) - np.uint64(1), (nw, N)).copy()
            c = t[:level].copy()
        else:
            t, c = H.rand_residues(rng, w, (), N).reshape(nw, N), H.rand_residues(rng, w[:level], (), N).reshape(level, N)
        for g in _galois_elements(N):
            x = ref.galois(g, t[None], idx=range(nw))
            for step in range(K):                          # modswitch, the last special prime first
                x = ref.modswitch(x, idx=range(nw - step))
            bare = x[0]
            full = ((bare.astype(object) + ref.galois(g, c[None], idx=range(level))[0].astype(object)) % ql).astype(np.uint64)
            for addend, want in ((None, bare), (c, full)):
                out = np.full((level, N), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
                rc = emul.ks_group_rot_emul_tail(K, level, wa.ctypes.data, N, g, t.ctypes.data, None if addend is None else addend.ctypes.data,
                                                 out.ctypes.data)
                assert rc == 0
                assert np.array_equal(out, want), (K, ct_bits, sp_bits, edge, g, addend is not None)


# ---- the digits commute with the automorphism ----------------------------------------------------------------------------------

def _emul_digits(emul, qs, Lk, level, k, alpha, c_end):
    """digits of c_end [level][N] over W, [d][nw][N], through the emulated ks_group_prepare / ks_group_eval"""
    W = KO.working_limbs(Lk, level, k)
    tq = np.array([qs[j] for j in W], dtype=np.uint64)
    out = np.zeros((len(KO.groups(level, alpha)), len(W), c_end.shape[1]), dtype=np.uint64)
    for gi, G in enumerate(KO.groups(level, alpha)):
        a = np.array([qs[i] for i in G], dtype=np.uint64)
        x = np.ascontiguousarray(c_end[list(G)])
        Gt = min(alpha, level) if min(alpha, level) <= 4 else 0   # the instantiation the entry points dispatch to (ksg_digits_fwd)
        assert emul.ks_group_rot_emul_digits(Gt, len(a), a.ctypes.data, len(tq), tq.ctypes.data, x.shape[1], x.ctypes.data, out[gi].ctypes.data) == 0
    return out


@pytest.mark.parametrize("Lk,k,alpha,level", [(8, 2, 2, 6), (10, 3, 3, 7), (6, 0, 4, 6), (7, 1, 6, 6)])
def test_grouped_digits_commute_with_the_automorphism(emul, Lk, k, alpha, level):
    """digits(sigma_g(c)) = sigma_g(digits(c)) in every working limb, word for word: the centred representative modulo the odd Q_g has
    no tie and centred(-x) = -centred(x).  0, 1, Q_g - 1, Q_g // 2 and Q_g // 2 + 1 planted in every group, the rest uniform; the
    emulated digits are also the oracle's."""
    N = 64
    qs = H.chain(30, Lk, N)
    ref = ref_cpu.RefCtx(N, qs)
    W = KO.working_limbs(Lk, level, k)
    rng = np.random.default_rng(Lk + alpha)
    c = H.rand_residues(rng, qs[:level], (), N).reshape(level, N)
    for G in KO.groups(level, alpha):
        Qg = math.prod(qs[i] for i in G)
        for pos, v in enumerate((0, 1, Qg - 1, Qg // 2, Qg // 2 + 1)):
            for i in G:
                c[i, pos] = v % qs[i]
    dig = _emul_digits(emul, qs, Lk, level, k, alpha, c)
    assert np.array_equal(dig, KO.digits(qs, Lk, level, k, alpha, c[None])[0])
    for g in (1, 3, 5, 2 * N - 1, pow(3, N // 2 + 3, 2 * N)):
        rotated = ref.galois(g, c[None], idx=range(level))[0]
        lhs = _emul_digits(emul, qs, Lk, level, k, alpha, rotated)
        rhs = ref.galois(g, dig, idx=W)
        assert np.array_equal(lhs, rhs), (Lk, k, alpha, level, g)


# ---- the host checks ----------------------------------------------------------------------------------------------------------

def test_every_host_check_in_the_headers_order(emul):
    """ks_group_many_check (csrc/ks_group_core.h), the function both entry points run first, on a ring of L = 8 limbs and N = 64:
    every call breaks one rule and later ones too where it can, and must report the earliest"""
    msg = C.create_string_buffer(200)
    N = 64
    ct_bytes = 2 * 4 * N * 8          # batch 1, level 4

    def call(product=0, null=0, Lk=6, level=4, k=2, group=2, nd=2, batch=1, keys=(0, 0, 0), gs=(3, 5, 127), n_rot=None, ct=1 << 20, out=1 << 24,
             diags=1 << 28):
        n_rot = len(keys) if n_rot is None else n_rot
        ka = (C.c_int * max(1, len(keys)))(*keys)
        ga = (C.c_uint64 * max(1, len(gs)))(*gs)
        nothing = C.c_int(-1)
        rc = emul.ks_group_rot_emul_check(product, null, 8, N, Lk, level, k, group, nd, batch, C.addressof(ka), C.addressof(ga), n_rot, ct, out, diags,
                                          C.addressof(nothing), msg, len(msg))
        return rc, msg.value.decode(), nothing.value
    for product in (0, 1):
        assert call(product) == (native.OK, "", 0)
        # 1. a null array or operand or a negative count, ahead of everything
        assert call(product, null=1, keys=(1, 0, 0), gs=(4, 3, 3), Lk=0, batch=-1, n_rot=70)[:2] == (native.E_BADARG, "null argument")
        assert call(product, n_rot=-1, keys=(), gs=(), Lk=0)[:2] == (native.E_BADARG, "null argument")
        # 3. per key in turn, the checks of tfhe_rotate_grouped in its order: the FIRST key that breaks a rule reports, and its earliest rule
        rc, m, _ = call(product, keys=(0, 1, 0), gs=(3, 3, 4), Lk=0)
        assert rc == native.E_BADARG and "key_limbs" in m                 # r = 0: the shape, ahead of the null key 1
        rc, m, _ = call(product, keys=(0, 1, 0), gs=(3, 4, 4))
        assert rc == native.E_BADARG and m == "null argument"             # r = 1: its null key, ahead of its own even g
        rc, m, _ = call(product, keys=(0, 0, 1), gs=(3, 4, 3))
        assert rc == native.E_BADARG and "odd and below 2N" in m          # r = 1: even g, ahead of the null key 2
        for g in (0, 4, 2 * N, 2 * N + 1):
            rc, m, _ = call(product, gs=(3, 5, g), out=1 << 20)
            assert rc == native.E_BADARG and "odd and below 2N" in m, g   # ahead of the overlap
        rc, m, _ = call(product, k=5, group=0, level=0, nd=0, batch=-1, gs=(4, 4, 4))
        assert rc == native.E_BADARG and "n_special" in m
        rc, m, _ = call(product, group=0, level=0, nd=0, batch=-1)
        assert rc == native.E_BADARG and "group" in m
        rc, m, _ = call(product, level=5, nd=0, batch=-1)
        assert rc == native.E_LEVEL and "level" in m
        rc, m, _ = call(product, nd=1, batch=-1, gs=(4, 4, 4))
        assert rc == native.E_PARAMS and "components" in m
        rc, m, _ = call(product, batch=-1, gs=(4, 4, 4))
        assert rc == native.E_BADARG and "negative batch" in m
        # 4. out against ct: anywhere, the last word included
        n_out = 1 if product else 3
        for out in ((1 << 20) + ct_bytes - 8, (1 << 20) - n_out * ct_bytes + 8, 1 << 20):
            rc, m, _ = call(product, out=out)
            assert rc == native.E_BADARG and "overlaps" in m, out
        assert call(product, out=(1 << 20) + ct_bytes)[0] == native.OK and call(product, out=(1 << 20) - n_out * ct_bytes)[0] == native.OK
        # an empty batch: every check, then nothing to do
        assert call(product, batch=0) == (native.OK, "", 1)
        assert call(product, batch=0, gs=(3, 5, 4))[0] == native.E_BADARG
    # 2. more than 64 rotations: the product only, ahead of the keys
    many = dict(keys=(1,) * 65, gs=(4,) * 65)
    rc, m, _ = call(1, **many)
    assert rc == native.E_UNSUPPORTED and "at most 64" in m
    rc, m, _ = call(0, **many)
    assert rc == native.E_BADARG and m == "null argument"                 # no limit there: key 0 is null
    assert call(0, keys=(0,) * 65, gs=(3,) * 65)[0] == native.OK and call(1, keys=(0,) * 64, gs=(3,) * 64)[0] == native.OK
    # the product's diagonals: [n_rot + 1][level][N]
    d_bytes = 4 * 4 * N * 8
    for out in ((1 << 28) + d_bytes - 8, (1 << 28) - ct_bytes + 8):
        rc, m, _ = call(1, out=out)
        assert rc == native.E_BADARG and "overlaps" in m
    assert call(1, out=(1 << 28) + d_bytes)[0] == native.OK and call(0, out=(1 << 28) + 8)[0] == native.OK
    # no rotation at all: tfhe_rotate_many_grouped returns right after the null checks, the product runs the shape checks once
    assert call(0, keys=(), gs=(), Lk=0, level=0, batch=-1, out=1 << 20) == (native.OK, "", 1)
    rc, m, _ = call(1, keys=(), gs=(), level=5)
    assert rc == native.E_LEVEL and "level" in m
    rc, m, _ = call(1, keys=(), gs=(), out=1 << 20)
    assert rc == native.E_BADARG and "overlaps" in m
    assert call(1, keys=(), gs=()) == (native.OK, "", 0)


# ---- the code objects -----------------------------------------------------------------------------------------------------------

@KH.needs_hipcc
def test_gfx950_code_objects_use_no_scratch_and_fit_two_workgroups(tmp_path):
    """figures only: k_ks_group_rot_tail<0..4> keeps K + 2 words per coefficient in registers -- no scratch, at most 128 VGPRs (two
    256-thread workgroups per SIMD pair, as k_ks_rot_tail) -- and its per-limb constants in static LDS"""
    recs = {r["name"]: r for r in KH.kernel_resources("ks_group_rot_emul/resource_probe.hip", tmp_path) if "k_ks_group_rot_tailILi" in r["name"]}
    assert len(recs) == 5, sorted(recs)
    for n, r in recs.items():
        print(n, r)
        assert r["scratch"] == 0, r
        assert r["vgprs"] <= 128 and r["agprs"] == 0, r
        assert 0 < r["static_lds"] <= 4096, r


# ---- the mirror -------------------------------------------------------------------------------------------------------------------

def test_mirror_argument_rules():
    qs = H.chain(30, 6, 64)
    ring = types.SimpleNamespace(L=len(qs), moduli=list(qs), N=64)
    inner = types.SimpleNamespace(relin_window=0, sigma=3.2, scheme_name="CKKS", R_key=lambda: ring, R_cipher=lambda: ring)
    gp = she.GroupedRaised(inner, 2, 2)
    gk = she.GaloisKey(3, types.SimpleNamespace(params=gp, key=[None]))
    plain = she.GaloisKey(3, types.SimpleNamespace(params=inner, key=[None]))
    with pytest.raises(she.UsageError, match="prepared_grouped takes a key with grouped digits"):
        plain.prepared_grouped()
    with pytest.raises(she.UsageError, match="GaloisKey.prepared"):
        gk.prepared()                                       # the per-limb routes keep refusing
    assert she.rotate_many_grouped([], [0, 0]) == []
    for call in (lambda: she.rotate_many_grouped([plain], [0, 0]), lambda: she.matmul_diag_grouped([plain], [], [0, 0]),
                 lambda: she.rotate_many_grouped([gk, she.GaloisKey(5, types.SimpleNamespace(params=she.GroupedRaised(inner, 2, 2), key=[None]))], [0, 0])):
        with pytest.raises(she.UsageError, match="one parameter set with grouped digits"):
            call()
    with pytest.raises(she.UsageError, match="at least one Galois key"):
        she.matmul_diag_grouped([], [], [0, 0])
    with pytest.raises(AssertionError, match="2-element"):
        she.rotate_many_grouped([gk], [0, 0, 0])
