"""No-GPU checks of tfhe_mul_relin (ciphertext product + relinearisation + modswitch of CKKS / BGV in one call):
the symbol is declared, exported, bound by ctypes and by the Julia shim with one signature; every argument check runs on the
host before any device use; the per-thread phases of the u64 fused product core (csrc/mul_core.h) run on the CPU
(tests/mul_core_emul/) give the oracle's enc_mul (transforms, tensor, inverse transforms) bit for bit; and the gfx950 code objects of every fused
kernel the entry point launches use no scratch memory and fit the LDS."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ref_cpu
from tests import helpers as H
from tests import kernel_harness as KH
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfhe_mul_relin"
# (ctx, key_limbs, level, special, evk, n_digits, c1, c2, ntt_in, rescale, out, batch)
CLASSES = ["ptr", "int", "int", "int", "ptr", "int", "ptr", "ptr", "int", "int", "ptr", "i64"]


def _err():
    return native.lib().tfhe_last_error().decode()


# ---- one signature everywhere --------------------------------------------------------------------------------------------

def test_symbol_declared_exported_and_bound_with_one_signature():
    protos = shim.header_prototypes()
    assert NAME in protos, f"{NAME} is not declared in include/toyfhe_hip.h"
    assert protos[NAME] == ("int", CLASSES)
    assert NAME in native.EXPORTED_SYMBOLS
    f = getattr(native.lib(), NAME)                      # AttributeError: not exported by the library
    assert len(f.argtypes) == len(CLASSES)
    want = {"ptr": C.c_void_p, "int": C.c_int, "i64": C.c_int64}
    assert [want[k] for k in CLASSES] == list(f.argtypes)
    assert f.restype is C.c_int
    assert callable(getattr(native.Context, "mul_relin"))


def test_julia_shim_binds_the_same_signature():
    calls = [c for c in shim.shim_ccalls() if c[0] == NAME]
    assert len(calls) == 1, "the shim binds tfhe_mul_relin exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == CLASSES and nargs == len(CLASSES)
    src = open(shim.SHIM).read()
    assert re.search(r"^function mul_relin\(ek::KeySwitchKey, c1::CipherText\{E1,P,", src, flags=re.M)


def test_header_says_which_sizes_are_fused():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index("int tfhe_mul_relin(")
    doc = text[text.rindex("/* ----", 0, i):i]
    for word in ("fused", "2^12 .. 2^14", "TFHE_E_LEVEL_MISMATCH", "overlapping", "batch == 0"):
        assert word in doc, word


# ---- argument validation precedes device use -------------------------------------------------------------------------------

def test_argument_validation_precedes_device_use():
    """every status the header names, with no context and no device: the checks that do not need the ring run first"""
    f = native.lib().tfhe_mul_relin
    a = np.zeros(64, dtype=np.uint64)
    b = np.zeros(64, dtype=np.uint64)
    o = np.zeros(64, dtype=np.uint64)
    k = np.zeros(64, dtype=np.uint64)
    pa, pb, po, pk = (x.ctypes.data for x in (a, b, o, k))
    for args in ((None, pa, pb, po), (pk, None, pb, po), (pk, pa, None, po), (pk, pa, pb, None)):
        assert f(None, 3, 2, 1, args[0], 3, args[1], args[2], 0, 0, args[3], 1) == native.E_BADARG
        assert "null" in _err()
    assert f(None, 3, 2, 1, pk, 3, pa, pb, 0, 0, po, -1) == native.E_BADARG
    assert "negative batch" in _err()
    for ntt_in, rescale in ((2, 0), (0, 2), (-1, 0)):
        assert f(None, 3, 2, 1, pk, 3, pa, pb, ntt_in, rescale, po, 1) == native.E_BADARG
    # modswitch of a one-limb ciphertext
    for level in (1, 0, -3):
        assert f(None, 3, level, 1, pk, 3, pa, pb, 0, 1, po, 1) == native.E_LEVEL
        assert "level >= 2" in _err()
    # out on top of an operand (the full range test needs the ring's N and follows the context check)
    assert f(None, 3, 2, 1, pk, 3, pa, pb, 0, 0, pa, 1) == native.E_BADARG
    assert "overlaps" in _err()
    assert f(None, 3, 2, 1, pk, 3, pa, pb, 0, 1, pb, 1) == native.E_BADARG
    assert "overlaps" in _err()
    # a missing context is an error even for an empty batch, as in tfhe_keyswitch
    assert f(None, 3, 2, 1, pk, 3, pa, pb, 0, 0, po, 0) == native.E_BADARG
    assert "null" in _err()
    # the mirror maps the statuses to the reference's exception classes
    with pytest.raises(native.UsageError):
        native.check(f(None, 3, 1, 1, pk, 3, pa, pb, 0, 1, po, 1))


# ---- the u64 fused core on the CPU -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = KH.build_emul("mul_core_emul/mul_core_emul.cpp", tmp_path_factory.mktemp("mul_core_emul"))
    u64p = C.POINTER(C.c_uint64)
    L.mul_core_emul.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int, u64p, u64p, u64p]
    L.mul_core_emul.restype = C.c_int

    def run(logn, q, a, b, square, ntt_in):
        a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
        out = np.empty((3, 1 << logn), dtype=np.uint64)
        rc = L.mul_core_emul(logn, q, 0, int(square), int(ntt_in), a.ctypes.data_as(u64p), b.ctypes.data_as(u64p), out.ctypes.data_as(u64p))
        assert rc == 0, rc
        return out
    run.lib = L
    return run


def _edge_moduli(N):
    """just above TFHE_FP_QMAX (the smallest modulus the u64 core serves), at 60 bits, just below 2^62 (the largest)"""
    return [H.primes_above(H.FP_QMAX, 1, N)[0], H.primes_above(1 << 59, 1, N)[0], H.primes_below(H.Q_LIMIT, 1, N)[0]]


@pytest.mark.parametrize("logn", [12, 13])
@pytest.mark.parametrize("ntt_in", [False, True])
@pytest.mark.parametrize("square", [False, True])
def test_u64_core_body_matches_the_oracle(emul, logn, square, ntt_in):
    N = 1 << logn
    rng = np.random.default_rng(1000 * logn + 2 * square + ntt_in)
    for q in _edge_moduli(N):
        assert H.FP_QMAX <= q < H.Q_LIMIT
        ref = ref_cpu.RefCtx(N, [q])
        a = H.rand_residues(rng, [q], (1, 2), N)                      # [1][2][1][N]
        b = a if square else H.rand_residues(rng, [q], (1, 2), N)
        # extreme words: 0, 1, q - 1 in the first positions of both components
        for x in ((a,) if square else (a, b)):
            x[0, :, 0, :3] = np.array([0, 1, q - 1], dtype=np.uint64)
        # the oracle's enc_mul takes and returns coefficients (transforms, tensor, inverse transforms: rlwe_she.jl:247-262)
        want = ref.enc_mul(a, b).reshape(3, N)
        ain, bin_ = (ref.nntt(a.reshape(2, 1, N)), ref.nntt(b.reshape(2, 1, N))) if ntt_in else (a, b)
        got = emul(logn, q, ain.reshape(2, N), bin_.reshape(2, N), square, ntt_in)
        assert np.array_equal(got, want), (logn, q, square, ntt_in)
        assert int(got.max()) < q


def test_u64_core_body_two_parking_rows_at_2_14(emul):
    """N = 2^14 takes the allocation with two parking rows (general form): one modulus at the top of the range"""
    N = 1 << 14
    q = H.primes_below(H.Q_LIMIT, 1, N)[0]
    rng = np.random.default_rng(14)
    ref = ref_cpu.RefCtx(N, [q])
    a, b = H.rand_residues(rng, [q], (1, 2), N), H.rand_residues(rng, [q], (1, 2), N)
    want = ref.enc_mul(a, b).reshape(3, N)
    assert np.array_equal(emul(14, q, a.reshape(2, N), b.reshape(2, N), False, False), want)


# ---- resources of the gfx950 code objects ------------------------------------------------------------------------------------

@KH.needs_hipcc
def test_fused_kernels_use_no_scratch_and_fit_the_lds(tmp_path, emul):
    """compiler-reported scratch is 0 and static + dynamic LDS <= 163 840 B for every instantiation tfhe_mul_relin launches"""
    jobs = [(lb, fp) for lb in (12, 13, 14) for fp in (0, 1)]
    found = KH.probe_all("mul_core_emul/resource_probe.hip", tmp_path, [(f"PROBE_LB={lb}", f"PROBE_FP={fp}") for lb, fp in jobs])
    seen = 0
    for (lb, fp), kernels in zip(jobs, found):
        dynamic = KH.lds_bytes(emul.lib, lb)              # what the launch asks for (mul_api.inc)
        mine = [k for k in kernels if k["name"].startswith(("_Z14k_mul_core_int", "_Z16k_bfv_core_fused"))]
        assert len(mine) == (4 if (fp == 0 or lb < 14) else 3), (lb, fp, [k["name"] for k in mine])
        for k in mine:
            print(f"{k['name']}: {k['vgprs']} VGPRs, scratch {k['scratch']}, static LDS {k['static_lds']}, dynamic LDS {dynamic}")
            assert k["scratch"] == 0, (k["name"], k["scratch"])
            assert k["static_lds"] + dynamic <= KH.LDS_LIMIT, (k["name"], k["static_lds"], dynamic)
            seen += 1
    assert seen == 23
