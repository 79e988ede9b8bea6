"""No-GPU checks of tfhe_dot_plain (ciphertext x plaintext sums over view operands with the forward transforms inside, one device
call): the symbol is declared, exported, bound by ctypes and by the Julia shim with one signature; every argument check that does
not need the ring runs on the host before any device use; the per-thread phases of the fused kernel (csrc/dot_core.h) run on the
CPU (tests/dot_core_emul/) give the oracle's sums bit for bit, for both arithmetic policies, at the edges of their modulus ranges
and with every word q - 1 over 64 terms; and the gfx950 code objects of every fused kernel the entry point launches use no scratch
memory and fit the LDS."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ref_cpu
from tests import dot_plain_oracle as DO
from tests import helpers as H
from tests import kernel_harness as KH
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ctx, acc, acc_stride, a, a_stride, a_ntt, b, b_stride, n_terms, dst, dst_stride, count, limbs, limb_idx)
DOT = ("tfhe_dot_plain", ["ptr", "ptr", "size", "ptr", "ptr", "ptr", "ptr", "ptr", "int", "ptr", "size", "i64", "int", "ptr"])


def _err():
    return native.lib().tfhe_last_error().decode()


# ---- one signature everywhere --------------------------------------------------------------------------------------------

def test_symbol_declared_exported_and_bound_with_one_signature():
    name, classes = DOT
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
            assert t is {"int": C.c_int, "i64": C.c_int64, "size": C.c_size_t}[k], (k, t)
    # the host arrays carry their element types: pointers, size_t strides, byte flags
    assert f.argtypes[4]._type_ is C.c_size_t and f.argtypes[7]._type_ is C.c_size_t and f.argtypes[5]._type_ is C.c_uint8
    assert callable(getattr(native.Context, "dot_plain"))


def test_julia_shim_binds_the_same_signature():
    name, classes = DOT
    calls = [c for c in shim.shim_ccalls() if c[0] == name]
    assert len(calls) == 1, f"the shim binds {name} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == classes and nargs == len(classes)
    src = open(shim.SHIM).read()
    assert re.search(r"^function dot_plain\(", src, flags=re.M)
    body = src[src.index("function dot_plain("):]
    body = body[:body.index("\nend")]
    assert "GC.@preserve" in body and re.search(r"\bon\(", body)


def test_header_names_sizes_views_statuses_and_the_overlap_rule():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index("int tfhe_dot_plain(")
    doc = text[text.rindex("/* ----", 0, i):i]
    for word in ("fused", "2^12 .. 2^14", "VIEW", "base + i * stride", "stride 0", "P * limbs * N", "SAME view", "TFHE_E_BADARG",
                 "TFHE_E_LEVEL_MISMATCH", "strided address ranges", "count == 0", "tfhe_ctx_set_chunk", "more than 64 terms", "canonical"):
        assert word in doc, word


# ---- argument validation precedes device use -------------------------------------------------------------------------------

def test_argument_validation_precedes_device_use():
    """every status that does not need the ring, with no context and host pointers; the context check follows them, so a call
    that passes them all ends at "null context" without having touched a device"""
    f = native.lib().tfhe_dot_plain
    bufs = [np.zeros(64, dtype=np.uint64) for _ in range(5)]
    pa, pb, pc, pacc, pdst = (x.ctypes.data for x in bufs)

    def call(acc=None, a=(pa, pc), b=(pb, pb), ntt=(0, 1), dst=pdst, count=1, n_terms=None, drop=None):
        n = len(a)
        A = (C.c_void_p * n)(*a)
        B = (C.c_void_p * n)(*b)
        AS = (C.c_size_t * n)(*([8] * n))
        BS = (C.c_size_t * n)(*([0] * n))
        AN = (C.c_uint8 * n)(*ntt)
        args = dict(a=A, a_stride=AS, a_ntt=AN, b=B, b_stride=BS)
        if drop:
            args[drop] = None
        return f(None, acc, 8, args["a"], args["a_stride"], args["a_ntt"], args["b"], args["b_stride"], n if n_terms is None else n_terms,
                 dst, 8, count, 1, None)
    for drop in ("a", "a_stride", "a_ntt", "b", "b_stride"):
        assert call(drop=drop) == native.E_BADARG and "null argument" in _err(), drop
    assert call(dst=None) == native.E_BADARG and "null argument" in _err()
    for n_terms in (0, -1):
        assert call(n_terms=n_terms) == native.E_BADARG and "at least one term" in _err()
    assert call(count=-1) == native.E_BADARG and "negative count" in _err()
    assert call(a=(pa, None)) == native.E_BADARG and "null operand 1" in _err()
    assert call(b=(None, pb)) == native.E_BADARG and "null operand 0" in _err()
    for ntt in ((2, 0), (0, 255)):
        assert call(ntt=ntt) == native.E_BADARG and "a_ntt" in _err(), ntt
    # dst where an operand starts (the full range test with strides needs the ring's N and follows the context check)
    assert call(a=(pa, pdst)) == native.E_BADARG and "overlaps operand 1" in _err()
    assert call(b=(pdst, pb)) == native.E_BADARG and "overlaps operand 0" in _err()
    # acc as the same view as dst is the in-place form: accepted, the context is next
    assert call(acc=pdst) == native.E_BADARG and "null context" in _err()
    assert call(acc=pacc) == native.E_BADARG and "null context" in _err()
    # a missing context is an error even for an empty batch
    assert call(count=0) == native.E_BADARG and "null context" in _err()
    with pytest.raises(AssertionError):
        native.check(call(count=-1))


# ---- the fused kernel's phases on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = KH.build_emul("dot_core_emul/dot_core_emul.cpp", tmp_path_factory.mktemp("dot_core_emul"))
    vp = C.c_void_p
    L.dot_core_emul_dot.argtypes = [C.c_int, C.c_uint64, C.c_int, vp, vp, vp, vp, C.c_int, vp, C.POINTER(C.c_double)]
    L.dot_core_emul_dot.restype = C.c_int

    L.dot_core_emul_dot_split.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_longlong, vp, vp, vp, vp, C.c_int, vp, C.POINTER(C.c_int)]
    L.dot_core_emul_dot_split.restype = C.c_int

    def dot_split(logn, q, fp, fill, acc, a, a_ntt, b):
        a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
        flags = np.ascontiguousarray(a_ntt, dtype=np.uint8)
        acc = np.array(acc, dtype=np.uint64)                 # in place: dst is acc
        ns = C.c_int(0)
        rc = L.dot_core_emul_dot_split(logn, q, int(fp), fill, acc.ctypes.data, a.ctypes.data, flags.ctypes.data, b.ctypes.data, a.shape[0],
                                       acc.ctypes.data, C.byref(ns))
        assert rc == 0, rc
        return acc, ns.value

    def dot(logn, q, fp, acc, a, a_ntt, b, in_place=False):
        a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
        flags = np.ascontiguousarray(a_ntt, dtype=np.uint8)
        acc = None if acc is None else np.array(acc, dtype=np.uint64)
        out = acc if in_place else np.empty(1 << logn, dtype=np.uint64)
        ratio = C.c_double(0)
        rc = L.dot_core_emul_dot(logn, q, int(fp), None if acc is None else acc.ctypes.data, a.ctypes.data, flags.ctypes.data, b.ctypes.data,
                                 a.shape[0], out.ctypes.data, C.byref(ratio))
        assert rc == 0, rc
        return out, ratio.value
    dot.split, dot.lib = dot_split, L
    return dot


FP_LIMIT = 7.9      # fp64arith.h TFHE_FP_LIMIT: |operand| / p admitted into an fp64 product or reduction


def _want(ref, acc, a, flags, b):
    return DO.dot_plain_ref(ref, None if acc is None else acc[None, None], [x[None, None] for x in a], list(flags), [x[None] for x in b])[0, 0]


@pytest.mark.parametrize("logn,q,fp", H.row_policy_cases())
def test_fused_body_matches_the_oracle_on_random_words(emul, logn, q, fp):
    N = 1 << logn
    assert (q < H.FP_QMAX) if fp else (q.bit_length() in (53, 62))
    rng = np.random.default_rng(7 * logn + fp)
    ref = ref_cpu.RefCtx(N, [q])
    seen = []
    for terms, flags, with_acc, in_place in ((1, [0], False, False), (5, [0, 1, 0, 0, 1], True, False), (3, [1, 1, 1], True, True),
                                             (4, [0, 0, 0, 0], True, True)):
        a = H.rand_residues(rng, [q], (terms,), N)[:, 0]
        b = H.rand_residues(rng, [q], (terms,), N)[:, 0]
        acc = H.rand_residues(rng, [q], (), N)[0] if with_acc else None
        want = _want(ref, acc, a, flags, b)
        got, ratio = emul(logn, q, fp, acc, a, flags, b, in_place)
        assert np.array_equal(got, want), (logn, q, fp, flags, in_place)
        assert int(got.max()) < q
        seen.append(ratio)
        print(f"dot_plain N=2^{logn} q={q} fp={fp} flags={flags}: max |operand|/p = {ratio:.3f}")
        assert (ratio < FP_LIMIT) if fp else ratio == 0
    assert max(seen) > 0 if fp else True                 # the tracker is alive


@pytest.mark.parametrize("logn,q,fp", H.row_policy_cases())
def test_fused_body_with_every_word_at_q_minus_1_over_64_terms(emul, logn, q, fp):
    """every operand, plaintext and accumulator word q - 1, 64 terms, transformed and untransformed terms mixed"""
    N = 1 << logn
    ref = ref_cpu.RefCtx(N, [q])
    terms = 64
    a = np.full((terms, N), q - 1, dtype=np.uint64)
    flags = [(k % 3) == 1 for k in range(terms)]          # mixed, starting with a transform
    acc = np.full(N, q - 1, dtype=np.uint64)
    want = _want(ref, acc, a, flags, a)
    got, ratio = emul(logn, q, fp, acc, a, flags, a)
    assert np.array_equal(got, want), (logn, q, fp)
    assert int(got.max()) < q
    print(f"dot_plain N=2^{logn} q={q} fp={fp} all q-1, 64 terms: max |operand|/p = {ratio:.3f}")
    assert (0 < ratio < FP_LIMIT) if fp else ratio == 0


@pytest.mark.parametrize("logn,q,fp", H.row_policy_cases()[1:4])          # a 53-bit u64 limb at 2^12, the 62-bit one at 2^14, the fp64 policy at 2^12
def test_split_over_terms_and_join_match_the_oracle(emul, logn, q, fp):
    """few rows: the pass is split over its terms (dot_split, split_terms, part_row) and joined (dot_join_word); acc in place.
    (fill, terms) -> splits: one split when the rows fill the chip or there are at most four terms, at least four terms per split,
    an uneven last split"""
    N = 1 << logn
    rng = np.random.default_rng(11 * logn + fp)
    ref = ref_cpu.RefCtx(N, [q])
    for fill, terms, splits in ((1, 9, 1), (512, 4, 1), (512, 9, 3), (2, 9, 2), (512, 17, 5), (3, 13, 3)):
        a = H.rand_residues(rng, [q], (terms,), N)[:, 0]
        b = H.rand_residues(rng, [q], (terms,), N)[:, 0]
        acc = H.rand_residues(rng, [q], (), N)[0]
        flags = [(k % 3) == 1 for k in range(terms)]
        got, ns = emul.split(logn, q, fp, fill, acc, a, flags, b)
        assert ns == splits, (fill, terms, ns)
        assert np.array_equal(got, _want(ref, acc, a, flags, b)), (logn, q, fp, fill, terms)


# ---- resources of the gfx950 code objects ------------------------------------------------------------------------------------

@KH.needs_hipcc
def test_fused_kernels_use_no_scratch_and_fit_the_lds(tmp_path, emul):
    """compiler-reported scratch is 0 and static + dynamic LDS <= 163 840 B for every instantiation the entry point launches"""
    jobs = [(lb, fp) for lb in (12, 13, 14) for fp in (0, 1)]
    found = KH.probe_all("dot_core_emul/resource_probe.hip", tmp_path, [(f"PROBE_LB={lb}", f"PROBE_FP={fp}") for lb, fp in jobs])
    seen = 0
    for (lb, fp), kernels in zip(jobs, found):
        dynamic = KH.lds_bytes(emul.lib, lb)              # what the launch asks for (launch_fused_rows)
        mine = [k for k in kernels if k["name"].startswith("_Z17k_dot_plain_fused")]
        assert len(mine) == 1, (lb, fp, [k["name"] for k in mine])
        for k in mine:
            print(f"{k['name']}: {k['vgprs']} VGPRs, scratch {k['scratch']}, static LDS {k['static_lds']}, dynamic LDS {dynamic}")
            assert k["scratch"] == 0, (k["name"], k["scratch"])
            assert k["static_lds"] + dynamic <= KH.LDS_LIMIT, (k["name"], k["static_lds"], dynamic)
            seen += 1
    assert seen == 6
