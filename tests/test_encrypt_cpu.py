"""No-GPU checks of tfhe_encrypt / tfhe_decrypt_phase (public-key encryption and the decryption phase of a batch in one device
call each): the symbols are declared, exported, bound by ctypes and by the Julia shim with one signature; every argument check
runs on the host before any device use; the per-thread phases of the fused kernels (csrc/enc_core.h) run on the CPU
(tests/enc_core_emul/) give the oracle's masked u + e1 + m, mask u + e2 and c1 + s c2 + s^2 c3 bit for bit, for both arithmetic
policies, at the edges of their modulus ranges and with growth-maximising operands; and the gfx950 code objects of every fused
kernel the entry points launch use no scratch memory and fit the LDS."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ref_cpu
from tests import enc_oracle as EO
from tests import helpers as H
from tests import kernel_harness as KH
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ctx, key_limbs, level, pk, sigma_u, sigma_e, mult_e, seed, stream, first_poly, rand, msg, out, batch)
ENC = ("tfhe_encrypt", ["ptr", "int", "int", "ptr", "f64", "f64", "u64", "u64", "u32", "u64", "ptr", "ptr", "ptr", "i64"])
# (ctx, key_limbs, level, secret, ct, polys, ntt_in, out, batch)
DEC = ("tfhe_decrypt_phase", ["ptr", "int", "int", "ptr", "ptr", "int", "int", "ptr", "i64"])
I32_BOUND = 2**31 - 1


def _err():
    return native.lib().tfhe_last_error().decode()


# ---- one signature everywhere --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,classes", [ENC, DEC])
def test_symbol_declared_exported_and_bound_with_one_signature(name, classes):
    protos = shim.header_prototypes()
    assert name in protos, f"{name} is not declared in include/toyfhe_hip.h"
    assert protos[name] == ("int", classes)
    assert name in native.EXPORTED_SYMBOLS
    f = getattr(native.lib(), name)                      # AttributeError: not exported by the library
    want = {"ptr": C.c_void_p, "int": C.c_int, "i64": C.c_int64, "u64": C.c_uint64, "u32": C.c_uint32, "f64": C.c_double}
    assert [want[k] for k in classes] == list(f.argtypes)
    assert f.restype is C.c_int
    assert callable(getattr(native.Context, "encrypt")) and callable(getattr(native.Context, "decrypt_phase"))


@pytest.mark.parametrize("name,classes", [ENC, DEC])
def test_julia_shim_binds_the_same_signature(name, classes):
    calls = [c for c in shim.shim_ccalls() if c[0] == name]
    assert len(calls) == 1, f"the shim binds {name} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == classes and nargs == len(classes)
    src = open(shim.SHIM).read()
    assert re.search(r"^function ToyFHE\.encrypt\(rng::HipRng, pk::PubKey, ", src, flags=re.M)
    assert re.search(r"^function ToyFHE\.decrypt\(key::PrivKey, c::CipherText\{", src, flags=re.M)


def test_header_names_sizes_counters_and_statuses():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index("int tfhe_encrypt(")
    doc = text[text.rindex("/* ----", 0, i):i]
    for word in ("fused", "2^12 .. 2^14", "first_poly + batch + b", "first_poly + 2 batch + b", "first_poly + 3 batch must not exceed 2^32",
                 "TFHE_E_BADARG", "TFHE_E_LEVEL_MISMATCH", "TFHE_E_UNSUPPORTED", "overlapping", "batch == 0", "mult_e"):
        assert word in doc, word


# ---- argument validation precedes device use -------------------------------------------------------------------------------

def test_encrypt_argument_validation_precedes_device_use():
    """every status the header names, with no context and host pointers: the checks that do not need the ring run first"""
    f = native.lib().tfhe_encrypt
    bufs = [np.zeros(64, dtype=np.uint64) for _ in range(4)]
    pk, msg, out, rnd = (x.ctypes.data for x in bufs)

    def call(key_limbs=3, level=2, pk=pk, first=0, rand=None, msg=None, out=out, batch=1, sigma=3.2):
        return f(None, key_limbs, level, pk, sigma, sigma, 1, 7, 1, first, rand, msg, out, batch)
    assert call(pk=None) == native.E_BADARG and "null" in _err()
    assert call(out=None) == native.E_BADARG and "null" in _err()
    assert call(batch=-1) == native.E_BADARG and "negative batch" in _err()
    for key_limbs, level in ((3, 0), (3, 4), (3, -1), (0, 1)):
        assert call(key_limbs=key_limbs, level=level) == native.E_LEVEL, (key_limbs, level)
        assert "level" in _err()
    # the polynomial counter: first_poly + 3 batch may reach 2^32, not pass it
    assert call(first=2**32 - 2, batch=1) == native.E_BADARG and "counter" in _err()
    assert call(first=0, batch=(2**32) // 3 + 1) == native.E_BADARG and "counter" in _err()
    assert call(first=2**32 - 3, batch=1) == native.E_BADARG and "null context" in _err()      # 2^32 exactly: accepted, the context is next
    assert call(first=2**32 - 2, batch=1, rand=rnd) == native.E_BADARG and "null context" in _err()   # given randomness: no counters
    assert call(sigma=-1.0) == native.E_BADARG and "sigma" in _err()
    # out on top of an operand (the full range test needs the ring's N and follows the context check)
    for kw in (dict(pk=out), dict(msg=out), dict(rand=out)):
        assert call(**kw) == native.E_BADARG and "overlaps" in _err(), kw
    # a missing context is an error even for an empty batch
    assert call(batch=0) == native.E_BADARG and "null context" in _err()
    with pytest.raises(native.UsageError):
        native.check(call(level=5))


def test_decrypt_argument_validation_precedes_device_use():
    f = native.lib().tfhe_decrypt_phase
    bufs = [np.zeros(64, dtype=np.uint64) for _ in range(3)]
    s, ct, out = (x.ctypes.data for x in bufs)

    def call(key_limbs=3, level=2, s=s, ct=ct, polys=2, ntt_in=0, out=out, batch=1):
        return f(None, key_limbs, level, s, ct, polys, ntt_in, out, batch)
    for kw in (dict(s=None), dict(ct=None), dict(out=None)):
        assert call(**kw) == native.E_BADARG and "null" in _err(), kw
    assert call(batch=-1) == native.E_BADARG and "negative batch" in _err()
    assert call(ntt_in=2) == native.E_BADARG
    for polys in (1, 4, 0):
        assert call(polys=polys) == native.E_UNSUPPORTED, polys
        assert "2 or 3" in _err()
    for key_limbs, level in ((3, 0), (3, 4), (0, 1)):
        assert call(key_limbs=key_limbs, level=level) == native.E_LEVEL
    for kw in (dict(ct=out), dict(s=out)):
        assert call(**kw) == native.E_BADARG and "overlaps" in _err(), kw
    assert call(batch=0) == native.E_BADARG and "null context" in _err()
    with pytest.raises(NotImplementedError):
        native.check(call(polys=4))


# ---- the fused kernels' phases on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = KH.build_emul("enc_core_emul/enc_core_emul.cpp", tmp_path_factory.mktemp("enc_core_emul"))
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.enc_core_emul_encrypt.argtypes = [C.c_int, C.c_uint64, C.c_int, vp, vp, C.c_uint64, vp, vp, dp]
    L.enc_core_emul_decrypt.argtypes = [C.c_int, C.c_uint64, C.c_int, vp, vp, C.c_int, C.c_int, vp, dp]
    L.enc_core_emul_encrypt.restype = L.enc_core_emul_decrypt.restype = C.c_int

    class E:
        lib = L

        @staticmethod
        def encrypt(logn, q, fp, pk, rand, mult_e, msg):
            pk, rand = np.ascontiguousarray(pk, dtype=np.uint64), np.ascontiguousarray(rand, dtype=np.int32)
            msg = None if msg is None else np.ascontiguousarray(msg, dtype=np.uint64)
            out, ratio = np.empty((2, 1 << logn), dtype=np.uint64), C.c_double(0)
            rc = L.enc_core_emul_encrypt(logn, q, int(fp), pk.ctypes.data, rand.ctypes.data, mult_e, None if msg is None else msg.ctypes.data,
                                         out.ctypes.data, C.byref(ratio))
            assert rc == 0, rc
            return out, ratio.value

        @staticmethod
        def decrypt(logn, q, fp, s, ct, ntt_in):
            s, ct = np.ascontiguousarray(s, dtype=np.uint64), np.ascontiguousarray(ct, dtype=np.uint64)
            out, ratio = np.empty(1 << logn, dtype=np.uint64), C.c_double(0)
            rc = L.enc_core_emul_decrypt(logn, q, int(fp), s.ctypes.data, ct.ctypes.data, ct.shape[0], int(ntt_in), out.ctypes.data, C.byref(ratio))
            assert rc == 0, rc
            return out, ratio.value
    return E


FP_LIMIT = 7.9      # fp64arith.h TFHE_FP_LIMIT: |operand| / p admitted into an fp64 product or reduction


def _extreme_rand(rng, N):
    """u, e1, e2 at +- the int32 bound in seeded random sign patterns, the first words pinned to +bound, -bound, 0, 1, -1"""
    r = np.where(rng.integers(0, 2, size=(3, N)) == 1, I32_BOUND, -I32_BOUND - 1).astype(np.int64)
    r[:, :5] = np.array([I32_BOUND, -I32_BOUND - 1, 0, 1, -1])
    return r


@pytest.mark.parametrize("logn,q,fp", H.row_policy_cases())
def test_fused_encrypt_body_matches_the_oracle(emul, logn, q, fp):
    N = 1 << logn
    assert (q < H.FP_QMAX) if fp else (q.bit_length() in (53, 62))
    rng = np.random.default_rng(100 * logn + fp)
    ref = ref_cpu.RefCtx(N, [q])
    # growth-maximising: noise at the int32 bound, key and message words q - 1; then seeded random operands with a BGV multiplier
    full = np.full((2, 1, N), q - 1, dtype=np.uint64)
    for pk, rand, mult, msg in ((full, _extreme_rand(rng, N), 1, np.full((1, N), q - 1, dtype=np.uint64)),
                                (H.rand_residues(rng, [q], (2,), N), rng.integers(-40, 41, size=(3, N)), 65537, None),
                                (H.rand_residues(rng, [q], (2,), N), _extreme_rand(rng, N), 65537, H.rand_residues(rng, [q], (), N))):
        want = EO.encrypt_ref(ref, pk, rand[None], mult, None if msg is None else msg[None])[0, :, 0]
        got, ratio = emul.encrypt(logn, q, fp, pk.reshape(2, N), rand, mult, None if msg is None else msg.reshape(N))
        assert np.array_equal(got, want), (logn, q, fp, mult)
        assert int(got.max()) < q
        print(f"encrypt N=2^{logn} q={q} fp={fp}: max |operand|/p = {ratio:.3f}")
        assert (0 < ratio < FP_LIMIT) if fp else ratio == 0


@pytest.mark.parametrize("ntt_in", [False, True])
@pytest.mark.parametrize("polys", [2, 3])
@pytest.mark.parametrize("logn,q,fp", H.row_policy_cases())
def test_fused_decrypt_body_matches_the_oracle(emul, logn, q, fp, polys, ntt_in):
    N = 1 << logn
    rng = np.random.default_rng(1000 * logn + 10 * polys + ntt_in + fp)
    ref = ref_cpu.RefCtx(N, [q])
    seen = []
    for s, ct in ((np.full((1, N), q - 1, dtype=np.uint64), np.full((1, polys, 1, N), q - 1, dtype=np.uint64)),
                  (H.rand_residues(rng, [q], (), N), H.rand_residues(rng, [q], (1, polys), N))):
        want = EO.decrypt_ref(ref, s, ct, ntt_in)[0, 0]
        got, ratio = emul.decrypt(logn, q, fp, s.reshape(N), ct.reshape(polys, N), ntt_in)
        assert np.array_equal(got, want), (logn, q, fp, polys, ntt_in)
        assert int(got.max()) < q
        seen.append(ratio)
        assert ratio < FP_LIMIT if fp else ratio == 0
    assert max(seen) > 0 if fp else True             # the tracker is alive (all-(q - 1) NTT images sum to zero: nothing to track there)


# ---- resources of the gfx950 code objects ------------------------------------------------------------------------------------

@KH.needs_hipcc
def test_fused_kernels_use_no_scratch_and_fit_the_lds(tmp_path, emul):
    """compiler-reported scratch is 0 and static + dynamic LDS <= 163 840 B for every instantiation the two entry points launch"""
    jobs = [(lb, fp) for lb in (12, 13, 14) for fp in (0, 1)]
    found = KH.probe_all("enc_core_emul/resource_probe.hip", tmp_path, [(f"PROBE_LB={lb}", f"PROBE_FP={fp}") for lb, fp in jobs])
    seen = 0
    for (lb, fp), kernels in zip(jobs, found):
        dynamic = KH.lds_bytes(emul.lib, lb)              # what the launch asks for (enc_api.inc)
        mine = [k for k in kernels if k["name"].startswith(("_Z15k_encrypt_fused", "_Z15k_decrypt_fused"))]
        assert len(mine) == (6 if lb < 14 else 5), (lb, fp, [k["name"] for k in mine])   # (2^14: no fused form for 3 NTT-domain components)
        for k in mine:
            print(f"{k['name']}: {k['vgprs']} VGPRs, scratch {k['scratch']}, static LDS {k['static_lds']}, dynamic LDS {dynamic}")
            assert k["scratch"] == 0, (k["name"], k["scratch"])
            assert k["static_lds"] + dynamic <= KH.LDS_LIMIT, (k["name"], k["static_lds"], dynamic)
            seen += 1
    assert seen == 34
