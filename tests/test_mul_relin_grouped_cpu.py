"""No-GPU checks of the product on grouped-digit keys (tfhe_mul_relin_grouped): the symbol is declared, exported, bound by ctypes and
by the Julia shim with one signature, and the mirror has its function while tf.mul_relin keeps refusing such keys; the header states
the chain and the order of the checks; a null context is refused by the library itself before any device use; every host check in
that order through the same function built for the host (a context cannot be made without a device); the per-coefficient body of the
tail with the rescale riding on it (csrc/ks_group_core.h, run on the CPU: tests/ks_group_tail_rescale_emul/) against exact integer
arithmetic -- K floor steps, the addend, then one more -- with the rescale's `last` and the special words planted at their edges; and
the gfx950 code objects of every instantiation use no scratch memory."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from tests import helpers as H
from tests import kernel_harness as KH
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native, she

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfhe_mul_relin_grouped"
# (ctx, key_limbs, level, n_special, group, evk, n_digits, c1, c2, ntt_in, rescale, out, batch)
CLASSES = ["ptr", "int", "int", "int", "int", "ptr", "int", "ptr", "ptr", "int", "int", "ptr", "i64"]


def _err():
    return native.lib().tfhe_last_error().decode()


# ---- one signature everywhere --------------------------------------------------------------------------------------------

def test_symbol_declared_exported_and_bound_with_one_signature():
    protos = shim.header_prototypes()
    assert NAME in protos, f"{NAME} is not declared in include/toyfhe_hip.h"
    assert protos[NAME] == ("int", CLASSES)
    assert NAME in native.EXPORTED_SYMBOLS
    f = getattr(native.lib(), NAME)                      # AttributeError: not exported by the library
    assert f.restype is C.c_int and len(f.argtypes) == len(CLASSES)
    for k, t in zip(CLASSES, f.argtypes):
        assert t is {"ptr": C.c_void_p, "int": C.c_int, "i64": C.c_int64}[k], (k, t)
    assert callable(native.Context.mul_relin_grouped)


def test_julia_shim_binds_the_same_signature_once():
    calls = [c for c in shim.shim_ccalls() if c[0] == NAME]
    assert len(calls) == 1, f"the shim binds {NAME} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == CLASSES and nargs == len(CLASSES)
    src = open(shim.SHIM).read()
    body = src[src.index("function mul_relin_grouped("):]
    body = body[:body.index("\nend")]
    assert "GC.@preserve" in body and "on(ctx" in body and "samecount(a, b)" in body and "rescale ? 1 : 0" in body


def test_header_states_the_chain_and_the_order_of_the_checks():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index(f"int {NAME}(")
    doc = text[text.rindex("/*", 0, i):i]
    for word in ("[batch][2][level][N]", "[batch][2][level-1][N]", "tfhe_nntt x2", "tfhe_tensor -> tfhe_inntt -> tfhe_keyswitch_grouped(polys = 3)",
                 "tfhe_rescale", "bit for bit", "tfhe_ctx_set_chunk", "(1, 1)", "(0, 1)", "tfhe_mul_relin(special = 1)", "tfhe_mul_relin(special = 0)",
                 "clamped", "tfhe_evalkey_gen", "rides on", "n_special == 0", "in this order"):
        assert word in doc, word
    order = [doc.index(w) for w in ("a null argument", "a negative batch", "ntt_in or rescale not 0 or 1", "rescale with level < 2", "out == c1 or out == c2",
                                    "the checks of tfhe_keyswitch_grouped with polys = 3", "overlapping c1 or c2","batch == 0 returns TFHE_OK", "above 2^31 - 1")]
    assert order == sorted(order), order
    assert i > text.index("int tfhe_matmul_diag_grouped(")
    # the comment of tfhe_rotate_many_grouped still ends at its declaration
    j = text.index("int tfhe_rotate_many_grouped(")
    assert text[:j].rstrip().endswith("*/")


def test_mirror_has_the_function_and_mul_relin_still_refuses_a_grouped_key():
    import toyfhe_jl_amd as tf
    assert tf.mul_relin_grouped is she.mul_relin_grouped
    ring = types.SimpleNamespace(L=6, moduli=H.chain(30, 6, 64), N=64)
    inner = types.SimpleNamespace(relin_window=0, sigma=3.2, scheme_name="CKKS", R_key=lambda: ring, R_cipher=lambda: ring)
    gp = she.GroupedRaised(inner, 2, 2)
    ct = types.SimpleNamespace(params=gp)
    grouped = she.EvalMultKey(types.SimpleNamespace(params=gp, key=[None]))
    with pytest.raises(she.UsageError, match="mul_relin has no support for keys with grouped digits"):
        she.mul_relin(grouped, ct, ct)
    per_limb = she.EvalMultKey(types.SimpleNamespace(params=she.ModulusRaised(inner), key=[None]))
    with pytest.raises(she.UsageError, match=r"mul_relin_grouped takes a key with grouped digits \(GroupedRaised\).*mul_relin"):
        she.mul_relin_grouped(per_limb, ct, ct)
    with pytest.raises(she.UsageError, match="differing parameters"):
        she.mul_relin_grouped(grouped, ct, types.SimpleNamespace(params=gp.params))


# ---- the host checks ----------------------------------------------------------------------------------------------------------

def test_a_null_context_is_refused_by_the_library_before_any_device_use():
    """no context and host pointers: each call also breaks later rules (a null context always) and must report the first"""
    lib = native.lib()
    buf = np.zeros(8, dtype=np.uint64).ctypes.data
    for args in ((None, 6, 4, 2, 2, buf, 2, buf, buf, 0, 1, buf, 1), (None, 0, 0, -1, 0, buf, 0, buf, buf, 2, 3, buf, -1),
                 (None, 6, 4, 2, 2, None, 2, buf, buf, 0, 0, buf, 1), (None, 6, 1, 2, 2, buf, 2, None, buf, 0, 1, buf, 0),
                 (None, 6, 4, 2, 2, buf, 2, buf, None, 0, 0, buf, 1), (None, 6, 4, 2, 2, buf, 2, buf, buf, 0, 0, None, 1)):
        assert getattr(lib, NAME)(*args) == native.E_BADARG and "null argument" in _err()
    with pytest.raises(AssertionError):
        native.check(getattr(lib, NAME)(None, 6, 4, 2, 2, buf, 2, buf, buf, 0, 0, buf, 1))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = KH.build_emul("ks_group_tail_rescale_emul/ks_group_tail_rescale_emul.cpp", tmp_path_factory.mktemp("ks_group_tail_rescale_emul"))
    vp, i32, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    L.ks_group_tail_rescale_emul.argtypes, L.ks_group_tail_rescale_emul.restype = [i32, i32, vp, C.c_long, vp, vp, vp], i32
    L.ks_group_tail_rescale_emul_check.argtypes = [i32, i32, i64, i32, i32, i32, i32, i32, i32, i64, i32, i32, u64, u64, u64, C.POINTER(i32),
                                                   C.c_char_p, C.c_size_t]
    L.ks_group_tail_rescale_emul_check.restype = i32
    return L


def test_every_host_check_in_the_headers_order(emul):
    """ks_group_mul_check (csrc/ks_group_core.h), the function tfhe_mul_relin_grouped runs first, on a ring of L = 8 limbs and N = 64:
    every call breaks one rule and later ones too where it can, and must report the earliest"""
    msg = C.create_string_buffer(200)
    nothing = C.c_int(0)
    N = 64
    ct_bytes = lambda level, batch=1: batch * 2 * level * N * 8
    A, B, O = 0x10000, 0x20000, 0x30000                      # addresses far enough apart for every shape below

    def call(null=0, L=8, logN=6, Lk=6, level=4, k=2, group=2, nd=2, batch=1, ntt_in=0, rescale=0, c1=A, c2=B, out=O):
        rc = emul.ks_group_tail_rescale_emul_check(null, L, 1 << logN, logN, Lk, level, k, group, nd, batch, ntt_in, rescale, c1, c2, out,
                                                   C.byref(nothing), msg, len(msg))
        return rc, msg.value.decode()
    assert call() == (native.OK, "") and nothing.value == 0
    assert call(rescale=1, ntt_in=1, c2=A, group=100, nd=1) == (native.OK, "")          # a square, one clamped digit
    inside = A + 8                                           # `out` inside c1's bytes without being c1 itself
    # 1. a null argument, ahead of everything
    assert call(null=1, batch=-1, ntt_in=2, rescale=1, level=1, out=A, Lk=0) == (native.E_BADARG, "null argument")
    # 2. a negative batch
    rc, m = call(batch=-1, ntt_in=2, rescale=1, level=1, out=A, Lk=0)
    assert rc == native.E_BADARG and m == "negative batch"
    # 3. the flags
    for ni, rs in ((2, 0), (-1, 1), (0, 2), (1, -1)):
        rc, m = call(ntt_in=ni, rescale=rs, level=1, out=A, Lk=0)
        assert rc == native.E_BADARG and "ntt_in and rescale are 0 or 1" in m, (ni, rs)
    # 4. a rescale needs two limbs: TFHE_E_LEVEL_MISMATCH
    for lv in (1, 0, -3):
        rc, m = call(rescale=1, level=lv, out=A, Lk=0)
        assert rc == native.E_LEVEL and "needs level >= 2" in m, lv
    assert call(rescale=0, level=1, nd=1)[0] == native.OK and call(rescale=1, level=2, nd=1)[0] == native.OK
    # 5. out is an operand
    for kw in (dict(out=A), dict(out=B), dict(out=A, c2=A)):
        rc, m = call(Lk=0, k=9, group=0, nd=0, **kw)
        assert rc == native.E_BADARG and m == "out overlaps an operand", kw
    # 6. the checks of tfhe_keyswitch_grouped with polys = 3, in its order, each ahead of the byte-range overlap
    for kw, status, word in ((dict(Lk=0, k=5, group=0), native.E_BADARG, "key_limbs"), (dict(Lk=9, k=5), native.E_BADARG, "key_limbs"),
                             (dict(k=5, group=0, level=9), native.E_BADARG, "n_special"), (dict(k=-1, group=0), native.E_BADARG, "n_special"),
                             (dict(group=0, level=9, nd=0), native.E_BADARG, "group"), (dict(level=5, nd=0), native.E_LEVEL, "level=5 outside [1,4]"),
                             (dict(nd=1), native.E_PARAMS, "components"), (dict(level=3, group=1, nd=2), native.E_PARAMS, "components")):
        rc, m = call(out=inside, **kw)
        assert rc == status and word in m and "3-element" not in m, (kw, rc, m)
    rc, m = call(L=64, Lk=44, level=40, k=4, group=4, nd=10, out=inside)
    assert rc == native.E_UNSUPPORTED and "working limbs" in m
    # 7. out overlaps an operand as a byte range -- also with an empty batch's later "nothing to do" and a batch past the row bound
    for kw in (dict(out=inside), dict(out=B + ct_bytes(4) - 8), dict(out=A - ct_bytes(4) + 8), dict(out=B - 8, rescale=1),
               dict(out=A + 8, batch=1 << 28)):
        rc, m = call(**kw)
        assert rc == native.E_BADARG and m == "out overlaps an operand", kw
    assert call(out=A + ct_bytes(4), c2=A)[0] == native.OK and call(out=A - ct_bytes(3), c2=A, rescale=1)[0] == native.OK
    assert call(out=A - ct_bytes(3) + 8, c2=A, rescale=1)[0] == native.E_BADARG
    # 8. an empty batch returns TFHE_OK without work, ahead of the row bound (which an empty batch cannot break) ...
    assert call(batch=0) == (native.OK, "") and nothing.value == 1
    assert call(batch=0, out=A + 8) == (native.OK, "") and nothing.value == 1           # (no bytes: nothing overlaps)
    # 9. ... and the 31-bit row count of tfhe_mul_relin: batch * 4 * level, shifted by log2 N - 14 above N = 2^14
    far = dict(c1=1 << 40, c2=1 << 50, out=1 << 60)
    rc, m = call(batch=(1 << 31) // 16, **far)
    assert rc == native.E_BADARG and m == "bad batch" and nothing.value == 0
    assert call(batch=(1 << 31) // 16 - 1, **far)[0] == native.OK
    rc, m = call(logN=16, batch=(1 << 31) // 64, **far)
    assert rc == native.E_BADARG and m == "bad batch"
    assert call(logN=16, batch=(1 << 31) // 64 - 1, **far)[0] == native.OK


# ---- the kernel body on the CPU ----------------------------------------------------------------------------------------------

def _exact(w, level, K, t, c):
    """exact integers: K floor steps of crt.jl:215-220 (the last special prime first), the addends, then one more step"""
    nw = level + K
    cur = [int(v) for v in t]
    for step in range(K):
        ql = w[nw - 1 - step]
        cur = [pow(ql, -1, w[j]) * (cur[j] - cur[-1] % w[j]) % w[j] for j in range(len(cur) - 1)]
    x = [(cur[j] + int(c[j])) % w[j] for j in range(level)]
    ql = w[level - 1]
    return x[level - 1], [pow(ql, -1, w[j]) * (x[j] - x[-1] % w[j]) % w[j] for j in range(level - 1)]


def _rings(K, level, N=64):
    return {"below": H.chain(40, level, N) + H.chain(30, K, N),                      # special primes below every ciphertext limb
            "above": H.chain(30, level, N) + H.chain(50, K, N),                      # above every one
            "mixed": H.chain(60, 1, N) + H.chain(40, level - 2, N) + H.chain(31, 1, N) +        # a narrow last limb under wide ones
                     (H.chain(41, K - 1, N) + H.chain(61, 1, N) if K > 1 else H.chain(61, 1, N)),
            "wide-last": H.chain(40, level - 1, N) + H.chain(61, 1, N) + H.chain(50, K, N)}     # a last limb above the others


@pytest.mark.parametrize("level", [2, 5])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("case", ["below", "above", "mixed", "wide-last"])
def test_tail_rescale_body_is_k_floor_steps_the_addend_and_one_more(emul, K, level, case):
    """random words; then rows with the special words at 0 and p - 1 and every other word at q - 1, the addend of the last limb chosen
    so that the rescale's `last` comes out 0, 1 and q_last - 1"""
    w = _rings(K, level)[case]
    nw = level + K
    assert len(w) == nw and len(set(w)) == nw
    rng = np.random.default_rng(10 * K + level)
    t = [[int(rng.integers(0, q)) for q in w] for _ in range(40)]
    c = [[int(rng.integers(0, q)) for q in w[:level]] for _ in range(40)]
    for sp in (lambda p: 0, lambda p: p - 1):
        for target in (0, 1, w[level - 1] - 1):
            row = [q - 1 for q in w[:level]] + [sp(p) for p in w[level:]]
            add = [q - 1 for q in w[:level]]
            before, _ = _exact(w, level, K, row, add[:level - 1] + [0])      # the last limb after the K steps, without its addend
            add[level - 1] = (target - before) % w[level - 1]
            assert _exact(w, level, K, row, add)[0] == target
            t.append(row)
            c.append(add)
    ta, ca, wa = (np.array(v, dtype=np.uint64) for v in (t, c, w))
    out = np.zeros((len(t), level - 1), dtype=np.uint64)
    assert emul.ks_group_tail_rescale_emul(K, level, wa.ctypes.data, len(t), ta.ctypes.data, ca.ctypes.data, out.ctypes.data) == 0
    want = np.array([_exact(w, level, K, tr, cr)[1] for tr, cr in zip(t, c)], dtype=np.uint64)
    assert np.array_equal(out, want), (K, level, case, np.argwhere(out != want)[:4])
    assert all(int(out[:, j].max()) < w[j] for j in range(level - 1))
    assert emul.ks_group_tail_rescale_emul(K, 1, wa.ctypes.data, 1, ta.ctypes.data, ca.ctypes.data, out.ctypes.data) == -1


@KH.needs_hipcc
def test_gfx950_code_objects_use_no_scratch(tmp_path):
    """k_ks_group_tail_rescale<1..4, 1..2>: every instantiation compiles for gfx950 and keeps its words in registers (no scratch, no
    LDS); the register counts are figures, printed for DESIGN.md"""
    recs = {r["name"]: r for r in KH.kernel_resources("ks_group_tail_rescale_emul/resource_probe.hip", tmp_path) if "k_ks_group_tail_rescaleILi" in r["name"]}
    assert len(recs) == 8, sorted(recs)
    for n, r in sorted(recs.items()):
        print(n, r)
        assert r["scratch"] == 0 and r["static_lds"] == 0, r
