"""No-GPU checks of tfhe_encrypt / tfhe_decrypt_phase (public-key encryption and the decryption phase of a batch in one device
call each): the symbols are declared, exported, bound by ctypes and by the Julia shim with one signature; every argument check
runs on the host before any device use; the per-thread phases of the fused kernels (csrc/enc_core.h) run on the CPU
(tests/enc_core_emul/) give the oracle's masked u + e1 + m, mask u + e2 and c1 + s c2 + s^2 c3 bit for bit, for both arithmetic
policies, at the edges of their modulus ranges and with growth-maximising operands; and the gfx950 code objects of every fused
kernel the entry points launch use no scratch memory and fit the LDS."""
import ctypes as C
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import ref_cpu
from tests import enc_oracle as EO
from tests import helpers as H
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
    so = str(tmp_path_factory.mktemp("enc_core_emul") / "libenc_core_emul.so")
    src = os.path.join(ROOT, "tests", "enc_core_emul", "enc_core_emul.cpp")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           "-shared", "-o", so, src])
    L = C.CDLL(so)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.enc_core_emul_encrypt.argtypes = [C.c_int, C.c_uint64, C.c_int, vp, vp, C.c_uint64, vp, vp, dp]
    L.enc_core_emul_decrypt.argtypes = [C.c_int, C.c_uint64, C.c_int, vp, vp, C.c_int, C.c_int, vp, dp]
    L.enc_core_emul_encrypt.restype = L.enc_core_emul_decrypt.restype = C.c_int

    class E:
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


def _cases():
    """(logn, q, fp): the u64 policy at the largest prime below 2^62 and at a 53-bit prime, N = 2^12 and 2^14; the fp64 policy at
    the top of its class (the largest prime below TFHE_FP_QMAX), N = 2^12, 2^13, 2^14"""
    out = []
    for logn in (12, 14):
        N = 1 << logn
        out += [(logn, H.primes_below(H.Q_LIMIT, 1, N)[0], 0), (logn, H.primes_above(1 << 52, 1, N)[0], 0)]
    out += [(logn, H.primes_below(H.FP_QMAX, 1, 1 << logn)[0], 1) for logn in (12, 13, 14)]
    return out


FP_LIMIT = 7.9      # fp64arith.h TFHE_FP_LIMIT: |operand| / p admitted into an fp64 product or reduction


def _extreme_rand(rng, N):
    """u, e1, e2 at +- the int32 bound in seeded random sign patterns, the first words pinned to +bound, -bound, 0, 1, -1"""
    r = np.where(rng.integers(0, 2, size=(3, N)) == 1, I32_BOUND, -I32_BOUND - 1).astype(np.int64)
    r[:, :5] = np.array([I32_BOUND, -I32_BOUND - 1, 0, 1, -1])
    return r


@pytest.mark.parametrize("logn,q,fp", _cases())
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
@pytest.mark.parametrize("logn,q,fp", _cases())
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

LDS_LIMIT = 163840   # bytes of LDS a workgroup may use on gfx950 (160 KiB)


def _probe(lb, fp, outdir):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "tests", "enc_core_emul", "resource_probe.hip")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value", "--cuda-device-only", "-c", src,
           f"-DPROBE_LB={lb}", f"-DPROBE_FP={fp}", "-o", os.path.join(outdir, f"probe_{lb}_{fp}.o"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def _dynamic_lds(lb):
    """what the launch asks for (enc_api.inc): the padded row image lds_words<LOGB, LOGT>() * 8 (ntt_core.h)"""
    m = (1 << lb) - 1
    words = (m + 2 * (m >> 6) + (m >> 10) + 1) if lb >= 13 else (m + 4 * (m >> 6) + (m >> 9) + 1)
    return words * 8


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc is not installed")
def test_fused_kernels_use_no_scratch_and_fit_the_lds(tmp_path):
    """compiler-reported scratch is 0 and static + dynamic LDS <= 163 840 B for every instantiation the two entry points launch"""
    jobs = [(lb, fp) for lb in (12, 13, 14) for fp in (0, 1)]
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        logs = list(ex.map(lambda j: _probe(j[0], j[1], str(tmp_path)), jobs))
    seen = 0
    for (lb, fp), log in zip(jobs, logs):
        blocks = re.split(r"remark: [^\n]*Function Name: ", log)[1:]
        mine = [b for b in blocks if b.startswith("_Z15k_encrypt_fused") or b.startswith("_Z15k_decrypt_fused")]
        assert len(mine) == (6 if lb < 14 else 5), (lb, fp, [b.split()[0] for b in mine])   # (2^14: no fused form for 3 NTT-domain components)
        for b in mine:
            name = b.split()[0]
            scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
            static_lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
            vgprs = int(re.search(r" VGPRs: (\d+)", b).group(1))
            print(f"{name}: {vgprs} VGPRs, scratch {scratch}, static LDS {static_lds}, dynamic LDS {_dynamic_lds(lb)}")
            assert scratch == 0, (name, scratch)
            assert static_lds + _dynamic_lds(lb) <= LDS_LIMIT, (name, static_lds, _dynamic_lds(lb))
            seen += 1
    assert seen == 34
