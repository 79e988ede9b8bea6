"""No-GPU checks of tfhe_evalkey_gen (public, relinearisation and Galois keys in one device call): the symbol is declared, exported,
bound by ctypes and by the Julia shim with one signature; every argument check that does not need the ring runs on the host, in the
order the header states, with no device present; the per-thread phases of the fused kernel (csrc/keygen_core.h) run on the CPU
(tests/keygen_core_emul/) give the oracle's (NTT(a), gamma old - (NTT(a) s + NTT(mult e))) bit for bit, for both arithmetic policies,
at the edges of their modulus ranges, with growth-maximising mask rows, every gadget residue class and every source of `old`; and
the gfx950 code objects of every fused kernel the entry point launches use no scratch memory and fit the LDS."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ref_cpu, spec
from tests import helpers as H
from tests import kernel_harness as KH
from tests import keygen_oracle as KO
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ctx, key_limbs, secret, old, galois_elements, n_keys, gadget, n_digits, sigma_e, mult_e, seed, stream_mask, stream_noise,
#  mask_poly, noise_poly, poly_stride, mask_rand, noise_rand, evks)
KEY = ("tfhe_evalkey_gen", ["ptr", "int", "ptr", "ptr", "ptr", "int", "ptr", "int", "f64", "u64", "u64", "u32", "u32", "u64", "u64", "u64",
                            "ptr", "ptr", "ptr"])
I32_BOUND = 2**31 - 1
FP_LIMIT = 7.9      # fp64arith.h TFHE_FP_LIMIT: |operand| / p admitted into an fp64 product or reduction


def _err():
    return native.lib().tfhe_last_error().decode()


# ---- one signature everywhere --------------------------------------------------------------------------------------------

def test_symbol_declared_exported_and_bound_with_one_signature():
    name, classes = KEY
    protos = shim.header_prototypes()
    assert name in protos, f"{name} is not declared in include/toyfhe_hip.h"
    assert protos[name] == ("int", classes)
    assert name in native.EXPORTED_SYMBOLS
    f = getattr(native.lib(), name)                      # AttributeError: not exported by the library
    got = ["ptr" if (t is C.c_void_p or hasattr(t, "contents")) else
           {C.c_int: "int", C.c_int64: "i64", C.c_uint64: "u64", C.c_uint32: "u32", C.c_double: "f64"}[t] for t in f.argtypes]
    assert got == classes
    assert f.restype is C.c_int
    assert callable(getattr(native.Context, "evalkey_gen"))


def test_julia_shim_binds_the_same_signature():
    name, classes = KEY
    calls = [c for c in shim.shim_ccalls() if c[0] == name]
    assert len(calls) == 1, f"the shim binds {name} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == classes and nargs == len(classes)
    src = open(shim.SHIM).read()
    assert re.search(r"^ToyFHE\.make_eval_key\(rng::HipRng, ", src, flags=re.M)
    assert re.search(r"^function ToyFHE\.keygen\(rng::HipRng, ", src, flags=re.M)


def test_mirror_exports_the_batched_galois_keygen_and_keeps_the_composition():
    import toyfhe_jl_amd as tf
    assert callable(tf.keygen_galois_many)
    for name in ("_keygen_composed", "_make_eval_key_composed", "_keygen_evalmult_composed", "_keygen_galois_composed"):
        assert callable(getattr(tf.she, name)), name
    assert isinstance(tf.she._FUSED_KEYGEN, bool)


def test_header_names_sizes_counters_and_statuses():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index("int tfhe_evalkey_gen(")
    doc = text[text.rindex("/* ----", 0, i):i]
    for word in ("fused", "2^12 .. 2^14", "[n_digits][2][key_limbs][N]", "mask_poly + m poly_stride", "noise_poly + m poly_stride",
                 "reach 2^32", "key_limbs <= 256", "TFHE_E_BADARG", "TFHE_E_LEVEL_MISMATCH", "overlapping", "n_keys == 0", "mult_e",
                 "in this order", "galois_elements", "gadget == NULL", "[n_keys][n_digits][key_limbs][N]", "int32 [n_keys][n_digits][N]"):
        assert word in doc, word


# ---- argument validation precedes device use -------------------------------------------------------------------------------

def test_argument_validation_precedes_device_use_in_the_stated_order():
    """every status the header names for the checks that do not need the ring, with no context and host pointers; each call breaks
    one rule and every later one too where it can, so that the ORDER shows"""
    f = native.lib().tfhe_evalkey_gen
    bufs = [np.zeros(64, dtype=np.uint64) for _ in range(7)]
    s, old, mr, nr, o0, o1, gad = (x.ctypes.data for x in bufs)
    gad_p = C.cast(gad, native.u64p)
    gal = (C.c_uint64 * 2)(0, 3)

    def call(key_limbs=3, secret=s, old=None, gal=gal, n_keys=2, gadget=gad_p, n_digits=3, sigma=3.2, mask_poly=0, noise_poly=1, stride=2,
             mask_rand=None, noise_rand=None, outs=(o0, o1), evks_null=False):
        ev = None if evks_null else (C.c_void_p * max(1, len(outs)))(*outs)
        return f(None, key_limbs, secret, old, gal, n_keys, gadget, n_digits, sigma, 1, 7, 0, 1, mask_poly, noise_poly, stride,
                 mask_rand, noise_rand, ev)
    # 1. null secret / evks, before the counts
    assert call(secret=None, n_digits=0) == native.E_BADARG and "null" in _err()
    assert call(evks_null=True, n_digits=0) == native.E_BADARG and "null" in _err()
    # 2. the counts, before key_limbs
    assert call(n_keys=-1, key_limbs=0) == native.E_BADARG and "n_keys" in _err()
    assert call(n_digits=0, key_limbs=0) == native.E_BADARG and "n_digits" in _err()
    # 3. key_limbs below 1, before the randomness pairing
    for kl in (0, -1):
        assert call(key_limbs=kl, mask_rand=mr) == native.E_LEVEL and "key_limbs" in _err()
    # 4. exactly one of the two buffers, before the counters
    assert call(mask_rand=mr, mask_poly=2**32) == native.E_BADARG and "together" in _err()
    assert call(noise_rand=nr, mask_poly=2**32) == native.E_BADARG and "together" in _err()
    # 5. device randomness: sigma, then the counters (the LAST component's counter may be 2^32 - 1, not 2^32), then the limb byte
    assert call(sigma=-1.0, mask_poly=2**32) == native.E_BADARG and "sigma" in _err()
    assert call(mask_poly=2**32 - 10, key_limbs=300) == native.E_BADARG and "counter" in _err()      # 6 components, stride 2: + 10
    assert call(noise_poly=2**32 - 10) == native.E_BADARG and "counter" in _err()
    assert call(mask_poly=2**32 - 1, noise_poly=0, n_keys=1, n_digits=1, stride=2**40, outs=(o0,)) == native.E_BADARG and "null context" in _err()
    assert call(mask_poly=2**32 - 11, noise_poly=2**32 - 11) == native.E_BADARG and "null context" in _err()
    assert call(stride=2**63) == native.E_BADARG and "counter" in _err()
    assert call(key_limbs=257, outs=(None, o1)) == native.E_BADARG and "256" in _err()
    #    given randomness: no counters, no limb byte -- the context is next
    assert call(mask_rand=mr, noise_rand=nr, mask_poly=2**40, sigma=-1.0, key_limbs=257) == native.E_BADARG and "null context" in _err()
    # 6. galois_elements where it is needed, a null output
    assert call(gal=None) == native.E_BADARG and "galois_elements" in _err()
    assert call(gal=None, old=old) == native.E_BADARG and "null context" in _err()                     # `old` given: not needed
    assert call(gal=None, gadget=None) == native.E_BADARG and "null context" in _err()                 # public key: not needed
    assert call(outs=(o0, None)) == native.E_BADARG and "null output 1" in _err()
    # 7. an output on top of an operand or of another output (the full range test needs N and follows the context check)
    for kw in (dict(outs=(o0, s)), dict(outs=(old, o1), old=old), dict(outs=(mr, o1), mask_rand=mr, noise_rand=nr),
               dict(outs=(o0, nr), mask_rand=mr, noise_rand=nr), dict(outs=(o0, o0))):
        assert call(**kw) == native.E_BADARG and "overlaps" in _err(), kw
    assert call(outs=(old, o1), old=old, gadget=None) == native.E_BADARG and "null context" in _err()  # public key: `old` is ignored
    # 8. a missing context is an error even for no keys
    assert call(n_keys=0, outs=()) == native.E_BADARG and "null context" in _err()
    with pytest.raises(native.UsageError):
        native.check(call(key_limbs=0))
    with pytest.raises(AssertionError):
        native.check(call(n_digits=0))


# ---- the fused kernel's phases on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = KH.build_emul("keygen_core_emul/keygen_core_emul.cpp", tmp_path_factory.mktemp("keygen_core_emul"))
    vp = C.c_void_p
    L.keygen_core_emul_item.argtypes = [C.c_int, C.c_uint64, C.c_int, vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, vp, C.POINTER(C.c_double)]
    L.keygen_core_emul_item.restype = C.c_int

    def item(logn, q, fp, s, old, gamma, gel, mask, noise, mult_e):
        s, mask = np.ascontiguousarray(s, dtype=np.uint64), np.ascontiguousarray(mask, dtype=np.uint64)
        noise = np.ascontiguousarray(noise, dtype=np.int32)
        old = None if old is None else np.ascontiguousarray(old, dtype=np.uint64)
        out, ratio = np.full((2, 1 << logn), 2**64 - 1, dtype=np.uint64), C.c_double(0)
        rc = L.keygen_core_emul_item(logn, q, int(fp), s.ctypes.data, None if old is None else old.ctypes.data, gamma, gel, mask.ctypes.data,
                                     noise.ctypes.data, mult_e, out.ctypes.data, C.byref(ratio))
        assert rc == 0, rc
        return out, ratio.value
    L.keygen_core_emul_item_stream.argtypes = [C.c_int, C.c_uint64, C.c_int, vp, C.c_uint64, C.c_uint64, C.c_double, C.c_uint64, C.c_uint64,
                                               C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                               vp, vp, C.POINTER(C.c_double)]
    L.keygen_core_emul_item_stream.restype = C.c_int

    def stream(logn, q, fp, s, gamma, gel, sigma, mult_e, seed, stream_mask, stream_noise, mask_poly, noise_poly, stride, m, j, key_limbs):
        s = np.ascontiguousarray(s, dtype=np.uint64)
        out, noise, ratio = np.full((2, 1 << logn), 2**64 - 1, dtype=np.uint64), np.zeros(1 << logn, dtype=np.int64), C.c_double(0)
        rc = L.keygen_core_emul_item_stream(logn, q, int(fp), s.ctypes.data, gamma, gel, sigma, mult_e, seed, stream_mask, stream_noise,
                                            mask_poly, noise_poly, stride, m, j, key_limbs, out.ctypes.data, noise.ctypes.data, C.byref(ratio))
        assert rc == 0, rc
        return out, noise, ratio.value
    item.stream, item.lib = stream, L
    return item


def _policies():
    """(q, fp) at N = 2^12: the u64 policy with a 60-bit prime; the fp64 policy at a 50-bit prime and at the largest prime below
    TFHE_FP_QMAX"""
    N = 1 << 12
    return [(H.primes_above(1 << 60, 1, N)[0], 0), (H.primes_above(1 << 50, 1, N)[0], 1), (H.primes_below(H.FP_QMAX, 1, N)[0], 1)]


_REF = {}


def _shared(q):
    """per modulus: the oracle context, a secret's NTT image, an explicit `old` row and the two old rows the call forms itself"""
    if q not in _REF:
        N = 1 << 12
        ref = ref_cpu.RefCtx(N, [q])
        rng = np.random.default_rng(q % 1000003)
        s = ref.nntt(KO.small_residues(np.rint(rng.normal(0, 3.2, size=(1, N))).astype(np.int64), 1, [q]))[0]
        _REF[q] = (ref, s, H.rand_residues(rng, [q], (1,), N), rng)
    return _REF[q]


def _mask_rows(q, N):
    alt = np.zeros(N, dtype=np.uint64)
    alt[1::2] = q - 1
    return {"all q-1": np.full(N, q - 1, dtype=np.uint64), "alternating 0, q-1": alt}


@pytest.mark.parametrize("source", ["explicit", "square", "g=3", "g=2N-1"])
@pytest.mark.parametrize("q,fp", _policies())
def test_fused_body_matches_the_oracle(emul, q, fp, source):
    logn, N = 12, 1 << 12
    assert (q < H.FP_QMAX) if fp else q.bit_length() == 61
    ref, s, old, rng = _shared(q)
    gel = {"explicit": 0, "square": 0, "g=3": 3, "g=2N-1": 2 * N - 1}[source]
    noise = np.where(rng.integers(0, 2, size=N) == 1, I32_BOUND, -I32_BOUND - 1).astype(np.int64)
    noise[:5] = np.array([I32_BOUND, -I32_BOUND - 1, 0, 1, -1])
    seen = []
    for name, mask in _mask_rows(q, N).items():
        for gamma in (0, 1, q - 1):
            for mult, nz in ((1, noise), (65537, np.rint(rng.normal(0, 3.2, size=N)).astype(np.int64))):
                want = KO.evalkey_ref(ref, s, mask[None, None, None], nz[None, None], mult, gadget=[[gamma]],
                                      old=old if source == "explicit" else None, galois=[gel])[0, 0, :, 0]
                got, ratio = emul(logn, q, fp, s[0], old[0, 0] if source == "explicit" else None, gamma, gel, mask, nz, mult)
                assert np.array_equal(got[0], want[0]), (name, gamma, mult, "mask row")
                assert np.array_equal(got[1], want[1]), (name, gamma, mult, "masked row")
                assert int(got.max()) < q
                seen.append(ratio)
                assert (ratio < FP_LIMIT) if fp else ratio == 0
    print(f"evalkey N=2^{logn} q={q} fp={fp} old={source}: max |operand|/p = {max(seen):.3f}")
    assert max(seen) > 0 if fp else True               # the tracker is alive


@pytest.mark.parametrize("logn", [13, 14])
@pytest.mark.parametrize("fp", [0, 1])
def test_fused_body_at_the_larger_sizes(emul, logn, fp):
    """N = 2^13 and 2^14 (the 512-thread register map; at 2^14 the combine reads NTT(a) back from row 0), both policies, the
    all q - 1 mask row, noise at the int32 bound, a Galois source"""
    N = 1 << logn
    q = H.primes_below(H.FP_QMAX, 1, N)[0] if fp else H.primes_above(1 << 60, 1, N)[0]
    ref = ref_cpu.RefCtx(N, [q])
    rng = np.random.default_rng(logn)
    s = ref.nntt(KO.small_residues(np.rint(rng.normal(0, 3.2, size=(1, N))).astype(np.int64), 1, [q]))[0]
    mask = np.full(N, q - 1, dtype=np.uint64)
    noise = np.where(rng.integers(0, 2, size=N) == 1, I32_BOUND, -I32_BOUND - 1).astype(np.int64)
    want = KO.evalkey_ref(ref, s, mask[None, None, None], noise[None, None], 65537, gadget=[[q - 1]], galois=[2 * N - 1])[0, 0, :, 0]
    got, ratio = emul(logn, q, fp, s[0], None, q - 1, 2 * N - 1, mask, noise, 65537)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (0 < ratio < FP_LIMIT) if fp else ratio == 0


@pytest.mark.parametrize("q,fp", _policies()[:2])
def test_fused_body_with_device_randomness(emul, q, fp):
    """the device-randomness form (mask_form, noise_form<false>) thread id by thread id: component m = 4 of a call with stride 2,
    limb 2 of 3.  The row of the uniform stream is the stream definition's, word for word; the Gaussian draws are the definition's
    up to rounding ties of the two libms; the key is the oracle's on the kernel's own draws."""
    logn, N = 12, 1 << 12
    ref, s, _, _ = _shared(q)
    seed, sm, sn, mask_poly, noise_poly, stride, m, j, sigma = 0xC0FFEE, 4, 9, 17, 1000, 2, 4, 2, 3.2
    for gel, mult in ((0, 1), (3, 65537)):
        got, noise, ratio = emul.stream(logn, q, fp, s[0], 1, gel, sigma, mult, seed, sm, sn, mask_poly, noise_poly, stride, m, j, 3)
        if gel == 0:                                  # (the draws do not depend on the source of old: computed once)
            mask = np.array([spec.sample_uniform_mod(((mask_poly + m * stride) << 32) | k, j, sm, seed, q) for k in range(N)], dtype=np.uint64)
        assert (noise != KO.stream_gauss(N, seed, sn, noise_poly + m * stride, sigma)).mean() < 0.01
        want = KO.evalkey_ref(ref, s, mask[None, None, None], noise[None, None], mult, gadget=[[1]], galois=[gel])[0, 0, :, 0]
        assert np.array_equal(got[0], want[0]), "row 0 is the transform of the uniform stream's polynomial"
        assert np.array_equal(got[1], want[1])
        assert (0 < ratio < FP_LIMIT) if fp else ratio == 0


def test_the_gadget_tables_of_the_mirror_are_the_oracles():
    """the residues the mirror hands to the call: RNS digits, raised RNS (zero special row and column), windows, raised windows"""
    import toyfhe_jl_amd as tf

    class P:      # the two fields _gadget_table reads
        def __init__(self, w):
            self.relin_window = w
    N = 1 << 5
    qs = H.primes_above(1 << 30, 3, N)

    class R:
        moduli, L = qs, len(qs)

        @staticmethod
        def modulus():
            return qs[0] * qs[1] * qs[2]
    assert tf.she._gadget_table(P(0), R) == KO.rns_gadget(qs)
    assert tf.she._gadget_table(P(16), R) == KO.window_gadget(qs, 16)
    raised = tf.ModulusRaised.__new__(tf.ModulusRaised)
    for w, want in ((0, KO.rns_gadget(qs, special=True)), (16, KO.window_gadget(qs, 16, special=True))):
        raised.relin_window = w
        got = tf.she._gadget_table(raised, R)
        assert got == want
        assert all(row[-1] == 0 for row in got)
    assert KO.rns_gadget(qs, special=True)[-1] == [0, 0, 0]


# ---- resources of the gfx950 code objects ------------------------------------------------------------------------------------

@KH.needs_hipcc
def test_fused_kernels_use_no_scratch_and_fit_the_lds(tmp_path, emul):
    """compiler-reported scratch is 0 and static + dynamic LDS <= 163 840 B for every instantiation the entry point launches.
    Resource figures only: nothing here looks at a kernel's instructions."""
    jobs = [(lb, fp) for lb in (12, 13, 14) for fp in (0, 1)]
    found = KH.probe_all("keygen_core_emul/resource_probe.hip", tmp_path, [(f"PROBE_LB={lb}", f"PROBE_FP={fp}") for lb, fp in jobs])
    seen = 0
    for (lb, fp), kernels in zip(jobs, found):
        dynamic = KH.lds_bytes(emul.lib, lb)              # what the launch asks for (keygen_api.inc)
        mine = [k for k in kernels if k["name"].startswith("_Z15k_evalkey_fused")]
        assert len(mine) == 2, (lb, fp, [k["name"] for k in mine])            # device randomness and given randomness
        for k in mine:
            print(f"{k['name']}: {k['vgprs']} VGPRs, scratch {k['scratch']}, static LDS {k['static_lds']}, dynamic LDS {dynamic}")
            assert k["scratch"] == 0, (k["name"], k["scratch"])
            assert k["static_lds"] + dynamic <= KH.LDS_LIMIT, (k["name"], k["static_lds"], dynamic)
            seen += 1
    assert seen == 12
