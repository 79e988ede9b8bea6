"""No-GPU checks of tfhe_matmul_bsgs (the diagonal matrix product by baby and giant steps, one device call): the symbol is declared,
exported, bound by ctypes and by the Julia shim with one signature; every argument check that does not need the ring runs on the
host before any device use; she.bsgs_diagonals regroups a diagonal sum exactly; the accumulation bodies of the k_md_acc kernels
(csrc/lazy_sum.h) run on the CPU (tests/md_acc_emul/, one input) give exact big-integer sums at 61- and 62-bit moduli with more terms than the
lazy-reduction chunk; and the gfx950 code objects of the accumulation kernels use no scratch memory."""
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
# (ctx, key_limbs, level, special, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, n_digits, diags, ct, out, batch)
BSGS = ("tfhe_matmul_bsgs", ["ptr", "int", "int", "int", "ptr", "ptr", "int", "ptr", "ptr", "int", "int", "ptr", "ptr", "ptr", "i64"])


def _err():
    return native.lib().tfhe_last_error().decode()


# ---- one signature everywhere --------------------------------------------------------------------------------------------

def test_symbol_declared_exported_and_bound_with_one_signature():
    name, classes = BSGS
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
    assert f.argtypes[5]._type_ is C.c_uint64 and f.argtypes[8]._type_ is C.c_uint64     # the Galois elements are host u64 arrays
    assert callable(getattr(native.Context, "matmul_bsgs")) and callable(she.matmul_bsgs) and callable(she.bsgs_diagonals)


def test_julia_shim_binds_the_same_signature():
    name, classes = BSGS
    calls = [c for c in shim.shim_ccalls() if c[0] == name]
    assert len(calls) == 1, f"the shim binds {name} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == classes and nargs == len(classes)
    src = open(shim.SHIM).read()
    body = src[src.index("function matmul_bsgs("):]
    body = body[:body.index("\nend")]
    assert "GC.@preserve" in body and re.search(r"\bon\(", body) and "prepared(" in body


def test_header_states_the_layouts_the_composition_and_the_checks():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index("int tfhe_matmul_bsgs(")
    doc = text[text.rindex("/*", 0, i):i]
    for word in ("[n_giant + 1][n_baby + 1][level][N]", "PREPARED", "HOST", "coefficient domain", "word for word", "tfhe_rotate_many",
                 "tfhe_nntt", "tfhe_dot", "tfhe_inntt", "tfhe_rotate_prepared", "tfhe_add", "tfhe_ctx_set_chunk", "same bits", "TFHE_E_BADARG",
                 "batch == 0", "[0, 64]"):
        assert word in doc, word


# ---- argument validation precedes device use -------------------------------------------------------------------------------

def test_argument_validation_precedes_device_use():
    """every status that does not need the ring, with no context and host pointers; the context check follows them, so a call that
    passes them all ends at "null context" without having touched a device"""
    f = native.lib().tfhe_matmul_bsgs
    bufs = [np.zeros(64, dtype=np.uint64) for _ in range(5)]
    pk, pk2, pd, pc, po = (x.ctypes.data for x in bufs)

    def call(baby=(pk, pk2), bg=(3, 5), giant=(pk,), gg=(9,), n_baby=None, n_giant=None, diags=pd, ct=pc, out=po, batch=1, drop=None):
        arr = lambda t, xs: (t * max(1, len(xs)))(*xs)
        args = dict(baby=arr(C.c_void_p, baby), bg=arr(C.c_uint64, bg), giant=arr(C.c_void_p, giant), gg=arr(C.c_uint64, gg))
        if drop:
            args[drop] = None
        return f(None, 3, 2, 1, args["baby"], args["bg"], len(baby) if n_baby is None else n_baby, args["giant"], args["gg"],
                 len(giant) if n_giant is None else n_giant, 2, diags, ct, out, batch)
    for drop in ("baby", "bg", "giant", "gg"):
        assert call(drop=drop) == native.E_BADARG and "null argument" in _err(), drop
    for kw in ("diags", "ct", "out"):
        assert call(**{kw: None}) == native.E_BADARG and "null argument" in _err(), kw
    for n in (-1, 65):
        assert call(n_baby=n) == native.E_BADARG and "n_baby" in _err(), n
        assert call(n_giant=n) == native.E_BADARG and "n_giant" in _err(), n
    assert call(baby=(pk, None)) == native.E_BADARG and "null baby key 1" in _err()
    assert call(giant=(None,)) == native.E_BADARG and "null giant key 0" in _err()
    # a null key beyond its count is not read: no keys at all is the plain product
    assert call(baby=(None,), n_baby=0, giant=(None,), n_giant=0) == native.E_BADARG and "null context" in _err()
    assert call(bg=(3, 4)) == native.E_BADARG and "galois element must be odd" in _err()
    assert call(gg=(0,)) == native.E_BADARG and "galois element must be odd" in _err()
    assert call(out=pc) == native.E_BADARG and "out overlaps an operand" in _err()
    assert call(out=pd) == native.E_BADARG and "out overlaps an operand" in _err()
    # everything that needs no ring passed: the context is next, and an empty batch needs one too
    assert call() == native.E_BADARG and "null context" in _err()
    assert call(batch=0) == native.E_BADARG and "null context" in _err()
    with pytest.raises(AssertionError):
        native.check(call(n_baby=-1))


# ---- the regrouping --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,n1,block", [(8, 1, 1), (8, 2, 1), (8, 3, 1), (8, 4, 4), (8, 8, 2), (7, 3, 1), (8, 16, 1)])
def test_bsgs_diagonals_regroup_the_plain_diagonal_sum(n, n1, block):
    """sum_k dv[k] * roll(x, k block) = sum_j roll(sum_i D[j][i] * roll(x, i block), j n1 block), in numpy (a rotation by s steps acts as
    np.roll(x, s)); n = 7, n1 = 3 has a ragged last giant step, n1 = 16 > n is clipped to one giant step"""
    rng = np.random.default_rng(100 * n + n1)
    slots = n * block * 2
    dv = rng.integers(-9, 10, (n, slots)).astype(np.int64)
    x = rng.integers(-9, 10, slots).astype(np.int64)
    D, baby, giant = she.bsgs_diagonals(dv, n1, block)
    m1 = min(n1, n)
    n2 = -(-n // m1)
    assert D.shape == (n2, m1, slots)
    assert baby == [i * block for i in range(1, m1)] and giant == [j * m1 * block for j in range(1, n2)]
    want = sum(dv[k] * np.roll(x, k * block) for k in range(n))
    rots = [x] + [np.roll(x, s) for s in baby]
    inner = [sum(D[j][i] * rots[i] for i in range(m1)) for j in range(n2)]
    got = inner[0] + sum(np.roll(inner[j], giant[j - 1]) for j in range(1, n2))
    assert np.array_equal(got, want)
    for j in range(n2):
        for i in range(m1):
            if j * m1 + i >= n:
                assert not D[j][i].any()                  # the rows past the last diagonal are zero
            else:
                assert np.array_equal(D[j][i], np.roll(dv[j * m1 + i], -j * m1 * block))
    with pytest.raises(AssertionError):
        she.bsgs_diagonals(dv, 0)


@pytest.mark.parametrize("n1", [4, 8, 16])
def test_bsgs_diagonals_on_the_example_layout_give_the_matrix_product(n1):
    """the layout of examples/encrypted_mnist.py (64 windows x B images per ciphertext, slot = window * B + image, diagonal k =
    W[i, (i - k) % 64] repeated B times, rotation by k B slots): the regrouped sum is plain_matmul(W, x) = W @ x -- the direction
    of the rotations the --bsgs circuit shape depends on"""
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("encrypted_mnist", os.path.join(ROOT, "examples", "encrypted_mnist.py"))
    em = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(em)
    rng = np.random.default_rng(n1)
    n, B = 64, 4
    W, x = rng.normal(0, 1, (n, n)), rng.normal(0, 1, (n, B))
    vs = np.stack([np.repeat(np.array([W[i, (i - k) % n] for i in range(n)]), B) for k in range(n)])
    D, bs, gs = she.bsgs_diagonals(vs, n1, block=B)
    slots = x.reshape(-1)
    rots = [slots] + [np.roll(slots, s) for s in bs]
    inner = [sum(D[j][i] * rots[i] for i in range(n1)) for j in range(n // n1)]
    got = inner[0] + sum(np.roll(inner[j], gs[j - 1]) for j in range(1, n // n1))
    assert np.allclose(got.reshape(n, B), em.plain_matmul(W, x), rtol=0, atol=1e-12 * n)      # float64 sums of 64 terms of size ~1
    assert np.allclose(em.plain_matmul(W, x), W @ x, rtol=0, atol=1e-12 * n)


# ---- the accumulation bodies on the CPU --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return KH.md_acc_emul(tmp_path_factory.mktemp("md_acc_emul"))      # (nin inputs chained: nin = 1 here)


def _moduli():
    """(q, lazy-reduction chunk): the largest primes below 2^62 and 2^61, a 60-bit, a 50-bit and a 30-bit one (N = 64)"""
    out = [(H.primes_below(1 << 62, 1, 64)[0], 1), (H.primes_below(1 << 61, 1, 64)[0], 2), (H.primes_below(1 << 60, 1, 64)[0], 4),
           (H.primes_below(1 << 50, 1, 64)[0], 64), (H.primes_below(1 << 30, 1, 64)[0], 64)]
    assert [q.bit_length() for q, _ in out] == [62, 61, 60, 50, 30]
    return out


@pytest.mark.parametrize("q,chunk", _moduli())
@pytest.mark.parametrize("edge", [False, True])
def test_accumulation_bodies_match_exact_sums(emul, q, chunk, edge):
    """both forms, every output tile (1, 2, 4 giant steps per pass) at whole and ragged tile counts, n_baby + 1 = 6 and 9 terms: above
    the chunk of the 60-, 61- and 62-bit moduli (4, 2, 1), with random words and with every word q - 1"""
    assert emul.md_acc_emul_chunk(q) == chunk
    n = 64
    rng = np.random.default_rng(q % 1000 + edge)
    pinv = int(rng.integers(1, 1 << 29)) % q or 1
    for nrot, ngiant1, tile in ((5, 1, 1), (5, 2, 2), (8, 3, 4), (5, 4, 4), (8, 5, 4), (0, 3, 4), (5, 2, 4), (5, 3, 2)):
        assert nrot == 0 or nrot + 1 > chunk or chunk == 64
        x = H.words_mod(rng, q, (2, n), edge)
        diag = H.words_mod(rng, q, (ngiant1, nrot + 1, n), edge)
        # the dense form: ROT rows as they are
        rot = H.words_mod(rng, q, (max(nrot, 1), n), edge)
        inner = np.zeros((ngiant1, n), dtype=np.uint64)
        assert emul.md_acc_emul_dense(q, tile, n, nrot, ngiant1, 1, x[0].ctypes.data, rot.ctypes.data, diag.ctypes.data, inner.ctypes.data) == 0
        terms = [x[0].astype(object)] + [rot[t].astype(object) for t in range(nrot)]
        for j in range(ngiant1):
            want = sum(diag[j][i].astype(object) * terms[i] for i in range(nrot + 1)) % q
            assert np.array_equal(inner[j].astype(object), want), ("dense", q, nrot, ngiant1, tile, j)
        if nrot == 0:
            continue                                       # (the evaluation-domain form needs a rotation)
        # the gather form: rotated value V[pi_r k] - U[k] (U scaled by P^-1 in the term where uscale is set)
        gs = np.array([int(g) for g in rng.choice(np.arange(3, 2 * n, 2), nrot, replace=False)], dtype=np.uint64)
        v = H.words_mod(rng, q, (nrot, n, 2), False)
        u = H.words_mod(rng, q, (2, nrot, n), edge)
        for uscale in (0, 1):
            i0, i1 = np.zeros((ngiant1, n), dtype=np.uint64), np.zeros((ngiant1, n), dtype=np.uint64)
            assert emul.md_acc_emul_gather(q, tile, uscale, pinv, n, nrot, ngiant1, 1, x.ctypes.data, v.ctypes.data, u.ctypes.data, gs.ctypes.data,
                                           diag.ctypes.data, i0.ctypes.data, i1.ctypes.data) == 0      # (x [2][n], u [2][nrot][n]: one input's layout)
            for s, got in ((0, i0), (1, i1)):
                terms = [x[s].astype(object)]
                for t in range(nrot):
                    uu = u[s][t].astype(object) * (pinv if uscale else 1) % q
                    terms.append((v[t][H.galois_pos(n, int(gs[t])), s].astype(object) - uu) % q)
                for j in range(ngiant1):
                    want = sum(diag[j][i].astype(object) * terms[i] for i in range(nrot + 1)) % q
                    assert np.array_equal(got[j].astype(object), want), ("gather", q, nrot, ngiant1, tile, uscale, s, j)
    assert emul.md_acc_emul_dense(q, 3, n, 0, 1, 1, None, None, None, None) == -1


# ---- resources of the gfx950 code objects ------------------------------------------------------------------------------------

@KH.needs_hipcc
def test_accumulation_kernels_use_no_scratch(tmp_path):
    """compiler-reported scratch is 0 for every instantiation tfhe_matmul_diag and tfhe_matmul_bsgs launch: the accumulators stay in
    registers"""
    kernels = KH.kernel_resources("md_acc_emul/resource_probe.hip", tmp_path, ["PROBE_SEED=0"])
    # <USCALE, NG, false> / <NG, false> / k_bsgs_sum's first parameter
    mine = [k for k in kernels if re.match(r"_Z\d+(k_md_acc(ILb[01]ELi[124]ELb0EE|_denseILi[124]ELb0EE)|k_bsgs_sumP)", k["name"])]
    assert len(mine) == 10, [k["name"] for k in kernels]   # 6 x k_md_acc, 3 x k_md_acc_dense, k_bsgs_sum
    for k in mine:
        print(f"{k['name']}: {k['vgprs']} VGPRs, {k['agprs']} AGPRs, scratch {k['scratch']}")
        assert k["scratch"] == 0, (k["name"], k["scratch"])
