"""No-GPU checks of the key switch with grouped RNS digits and several special primes (tfhe_keyswitch_grouped, tfhe_rotate_grouped):
the two symbols are declared, exported, bound by ctypes and by the Julia shim with one signature; the oracle
(tests/ks_grouped_oracle.py) equals oracle/spec.py -- `keyswitch` in the two degenerate cases, a direct composition of switch_poly,
poly_mul and modswitch_poly otherwise -- and a relinearisation with a genuine grouped key decrypts within the derived bound; the host
checks of the entry points in the header's order (the null arguments through the library itself, every check through the same
function built for the host: a context cannot be made without a device); the digit and tail bodies of csrc/ks_group_core.h, run on
the CPU (tests/ks_group_emul/), against the oracle at the edges of every group; the gfx950 code objects use no scratch memory; and
the mirror's gadget table and usage errors."""
import ctypes as C
import math
import os
import random
import types

import numpy as np
import pytest

from oracle import ref_cpu, spec
from tests import helpers as H
from tests import kernel_harness as KH
from tests import ks_grouped_oracle as KO
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native, she

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ctx, key_limbs, level, n_special, group, evk, n_digits, ct, polys, out, batch)
KSG = ("tfhe_keyswitch_grouped", ["ptr", "int", "int", "int", "int", "ptr", "int", "ptr", "int", "ptr", "i64"])
# (ctx, key_limbs, level, n_special, group, evk, n_digits, galois_element, ct, out, batch)
ROT = ("tfhe_rotate_grouped", ["ptr", "int", "int", "int", "int", "ptr", "int", "u64", "ptr", "ptr", "i64"])


def _err():
    return native.lib().tfhe_last_error().decode()


# ---- one signature everywhere --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,classes", [KSG, ROT])
def test_symbols_declared_exported_and_bound_with_one_signature(name, classes):
    protos = shim.header_prototypes()
    assert name in protos, f"{name} is not declared in include/toyfhe_hip.h"
    assert protos[name] == ("int", classes)
    assert name in native.EXPORTED_SYMBOLS
    f = getattr(native.lib(), name)                      # AttributeError: not exported by the library
    assert f.restype is C.c_int and len(f.argtypes) == len(classes)
    for k, t in zip(classes, f.argtypes):
        assert t is {"ptr": C.c_void_p, "int": C.c_int, "i64": C.c_int64, "u64": C.c_uint64}[k], (k, t)
    assert callable(getattr(native.Context, name[len("tfhe_"):]))
    import toyfhe_jl_amd as tf
    assert tf.GroupedRaised is she.GroupedRaised and not issubclass(she.GroupedRaised, she.ModulusRaised)


@pytest.mark.parametrize("name,classes", [KSG, ROT])
def test_julia_shim_binds_the_same_signature(name, classes):
    calls = [c for c in shim.shim_ccalls() if c[0] == name]
    assert len(calls) == 1, f"the shim binds {name} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == classes and nargs == len(classes)
    src = open(shim.SHIM).read()
    body = src[src.index(f"function {name[len('tfhe_'):]}("):]
    body = body[:body.index("\nend")]
    assert "GC.@preserve" in body and "on(ctx" in body and "batchsize(c)" in body


def test_header_states_the_definition_and_the_order_of_the_checks():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index("int tfhe_keyswitch_grouped(")
    doc = text[text.rindex("/*", 0, i):i]
    for word in ("signedmod.jl:12-19", "bfv.jl:202-226", "rlwe_she.jl:326-329", "crt.jl:215-228", "rlwe_she.jl:324", "the last special prime first",
                 "[n_digits][2][key_limbs][N]", "[batch][polys][level][N]", "[batch][2][level][N]", "coefficient domain", "tfhe_evalkey_gen",
                 "(1, 1)", "(0, 1)", "tfhe_keyswitch(special = 1)", "tfhe_keyswitch(special = 0)", "ragged", "in this order", "batch == 0"):
        assert word in doc, word
    order = [doc.index(w) for w in ("a null argument", "polys outside {2,3}", "key_limbs outside [1, L]", "n_special outside [0, min(4, key_limbs - 1)]",
                                    "group < 1", "level outside [1, key_limbs - n_special]", "n_digits < ceil(level / group)",
                                    "level + n_special > 40", "a negative batch", "a Galois element that is even or not below 2N")]
    assert order == sorted(order), order
    assert text.index("int tfhe_rotate_grouped(") > i


# ---- the oracle against oracle/spec.py ------------------------------------------------------------------------------------

def _spec_setup(seed, N, qs, level, polys, ndig):
    """uniform key and ciphertext as spec lists (coefficient domain) and as the oracle's arrays (key in the NTT domain)"""
    rng = random.Random(seed)
    keyring = spec.Ring(N, qs)
    cring = keyring.select(range(level))
    evk = [(spec.sample_uniform(rng, keyring), spec.sample_uniform(rng, keyring)) for _ in range(ndig)]
    ct = [spec.sample_uniform(rng, cring) for _ in range(polys)]
    ref = ref_cpu.RefCtx(N, qs, keyring.psis)
    evk_np = np.array([[spec.poly_nntt(p, keyring) for p in pair] for pair in evk], dtype=np.uint64)
    ct_np = np.array(ct, dtype=np.uint64)[None]
    return keyring, cring, evk, ct, ref, evk_np, ct_np


@pytest.mark.parametrize("N,bits,Lk,level,special,polys", [(16, 30, 4, 3, 1, 3), (16, 30, 4, 2, 1, 2), (32, 40, 3, 3, 0, 3), (32, 40, 4, 2, 0, 2),
                                                             (64, 30, 3, 2, 1, 2)])
def test_oracle_is_spec_keyswitch_in_the_degenerate_cases(N, bits, Lk, level, special, polys):
    """(k, alpha) = (1, 1) and (0, 1) at the key's full level and at a lower one"""
    keyring, cring, evk, ct, ref, evk_np, ct_np = _spec_setup(N + level, N, H.chain(bits, Lk, N), level, polys, Lk)
    want = np.array(spec.keyswitch(evk, ct, cring, keyring, bool(special)), dtype=np.uint64)
    got = KO.keyswitch_grouped_ref(ref, level, special, 1, evk_np, ct_np)
    assert got.shape == (1, 2, level, N) and np.array_equal(got[0], want)


def _spec_grouped(evk, ct, keyring, level, k, alpha):
    """the definition as a direct composition of spec.switch_poly, poly_mul and modswitch_poly"""
    Lk = keyring.L
    W = KO.working_limbs(Lk, level, k)
    wring = keyring.select(W)
    P = math.prod(keyring.qs[Lk - k:])
    raise_ = lambda c: [[(P % q) * x % q for x in c[j]] for j, q in enumerate(wring.qs[:level])] + [[0] * keyring.N for _ in range(k)]
    c1 = raise_(ct[0])
    c2 = spec.poly_zero(wring) if len(ct) == 2 else raise_(ct[1])
    for g, G in enumerate(KO.groups(level, alpha)):
        p = spec.switch_poly([ct[-1][i] for i in G], keyring.select(G), wring)
        c2 = spec.poly_add(c2, spec.poly_mul([evk[g][0][j] for j in W], p, wring), wring)
        c1 = spec.poly_add(c1, spec.poly_mul([evk[g][1][j] for j in W], p, wring), wring)
    ring = wring
    for _ in range(k):
        c1, c2 = spec.modswitch_poly(c1, ring), spec.modswitch_poly(c2, ring)
        ring = ring.drop_last()
    return [c1, c2]


def _mixed(N):
    return H.chain(60, 1, N) + H.chain(40, 5, N)


GROUPED = [  # (N, moduli, k, alpha, level, polys)
    (16, H.chain(30, 6, 16), 2, 2, 4, 3), (16, H.chain(30, 6, 16), 2, 2, 3, 2),        # full level; a lower one: groups (0, 1), (2)
    (32, _mixed(32), 3, 2, 3, 3),                                                        # (60-bit, 40-bit), (40-bit): mixed and ragged
    (32, _mixed(32), 2, 3, 4, 2),                                                        # (60, 40, 40), (40)
    (64, H.chain(30, 7, 64), 3, 3, 4, 3), (64, H.chain(30, 7, 64), 3, 3, 2, 2),        # ragged at the top level; one short group
    (16, H.chain(30, 6, 16), 1, 6, 5, 2), (16, H.chain(30, 6, 16), 0, 2, 5, 3),        # one digit of five limbs; no special prime
    (16, H.chain(30, 6, 16), 4, 1, 2, 3),                                              # four special primes, per-limb digits
]


@pytest.mark.parametrize("N,qs,k,alpha,level,polys", GROUPED)
def test_oracle_is_the_composition_of_switch_mul_and_modswitch(N, qs, k, alpha, level, polys):
    d = -(-level // alpha)
    keyring, cring, evk, ct, ref, evk_np, ct_np = _spec_setup(N + 7 * k + alpha, N, qs, level, polys, d + 1)   # (a spare component: unused)
    want = np.array(_spec_grouped(evk, ct, keyring, level, k, alpha), dtype=np.uint64)
    got = KO.keyswitch_grouped_ref(ref, level, k, alpha, evk_np, ct_np)
    assert np.array_equal(got[0], want)
    assert all(int(got[0, s, j].max()) < qs[j] for s in range(2) for j in range(level))


@pytest.mark.parametrize("N,qs,k,alpha,level", [(16, H.chain(30, 6, 16), 2, 2, 4), (16, H.chain(30, 6, 16), 2, 2, 3), (32, _mixed(32), 3, 2, 3),
                                                (32, H.chain(30, 7, 32), 3, 3, 4)])
def test_relinearisation_with_a_genuine_grouped_key_decrypts_within_the_bound(N, qs, k, alpha, level):
    """key_g = (mask, gamma_g s^2 - (mask s + e)) over the key ring with the hand-built gadget gamma (P at the limbs of group g of the
    key's top level); keyswitch of (c0, c1, c2) moves the phase c0 + c1 s + c2 s^2 by at most
        d N (max Q_g // 2 + 1) max|e| // P + 1 + k (1 + N max|s|)
    (the key noise against digits of at most Q_g // 2, divided by P; one unit of rounding per contraction step and component, the
    second component times s), the maxima taken from the actual draws"""
    rng = random.Random(N + level)
    keyring = spec.Ring(N, qs)
    Lk = keyring.L
    cring = keyring.select(range(level))
    s_int = spec.sample_gauss_ints(rng, N, 3.2)
    s = spec.poly_from_ints(s_int, keyring)
    s2 = spec.poly_mul(s, s, keyring)
    gadget = KO.gadget_table(qs, k, alpha)
    assert len(gadget) == -(-(Lk - k) // alpha) and all(row[j] == 0 for row in gadget for j in range(Lk - k, Lk))
    evk, emax = [], 0
    for row in gadget:
        mask = spec.sample_uniform(rng, keyring)
        e_int = spec.sample_gauss_ints(rng, N, 3.2)
        emax = max(emax, max(abs(x) for x in e_int))
        a = [[row[j] * x % q for x in s2[j]] for j, q in enumerate(qs)]
        masked = spec.poly_sub(a, spec.poly_add(spec.poly_mul(mask, s, keyring), spec.poly_from_ints(e_int, keyring), keyring), keyring)
        evk.append((mask, masked))
    ct = [spec.sample_uniform(rng, cring) for _ in range(3)]
    ref = ref_cpu.RefCtx(N, qs, keyring.psis)
    evk_np = np.array([[spec.poly_nntt(p, keyring) for p in pair] for pair in evk], dtype=np.uint64)
    out = KO.keyswitch_grouped_ref(ref, level, k, alpha, evk_np, np.array(ct, dtype=np.uint64)[None])[0]
    sc = [x[:] for x in s[:level]]
    before = spec.poly_to_ints(spec.decrypt_raw(sc, ct, cring), cring)
    after = spec.poly_to_ints(spec.decrypt_raw(sc, [[list(map(int, r)) for r in out[0]], [list(map(int, r)) for r in out[1]]], cring), cring)
    delta = max(abs(spec.centred((a - b) % cring.Q, cring.Q)) for a, b in zip(after, before))
    groups = KO.groups(level, alpha)
    qg = max(math.prod(qs[i] for i in G) for G in groups)
    P = math.prod(qs[Lk - k:])
    bound = len(groups) * N * (qg // 2 + 1) * emax // P + 1 + k * (1 + N * max(abs(x) for x in s_int))
    print(f"N={N} k={k} alpha={alpha} level={level}: |delta phase| = {delta}, bound = {bound}")
    assert emax > 0 and delta <= bound, (delta, bound)


# ---- the host checks ----------------------------------------------------------------------------------------------------------

def test_a_null_argument_is_refused_by_the_library_before_any_device_use():
    """no context and host pointers: each call also breaks later rules (a null context always) and must report the first"""
    lib = native.lib()
    buf = np.zeros(8, dtype=np.uint64).ctypes.data
    for args in ((None, 3, 2, 1, 1, buf, 2, buf, 2, buf, 1), (None, 0, 0, -1, 0, buf, 0, buf, 4, buf, -1)):
        assert lib.tfhe_keyswitch_grouped(*args) == native.E_BADARG and "null argument" in _err()
    for args in ((None, 3, 2, 1, 1, buf, 2, 3, buf, buf, 1), (None, 3, 2, 1, 1, None, 2, 4, buf, buf, 0), (None, 3, 2, 1, 1, buf, 2, 4, None, buf, 0),
                 (None, 3, 2, 1, 1, buf, 2, 4, buf, None, -1)):
        assert lib.tfhe_rotate_grouped(*args) == native.E_BADARG and "null argument" in _err()
    with pytest.raises(AssertionError):
        native.check(lib.tfhe_keyswitch_grouped(None, 3, 2, 1, 1, None, 2, None, 2, None, 1))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = KH.build_emul("ks_group_emul/ks_group_emul.cpp", tmp_path_factory.mktemp("ks_group_emul"))
    vp, i32, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    L.ks_group_emul_digits.argtypes, L.ks_group_emul_digits.restype = [i32, i32, vp, i32, vp, C.c_long, vp, vp], C.c_long
    L.ks_group_emul_lift_digit.argtypes, L.ks_group_emul_lift_digit.restype = [u64, u64, u64], u64
    L.ks_group_emul_tail.argtypes, L.ks_group_emul_tail.restype = [i32, i32, vp, C.c_long, vp, vp], i32
    L.ks_group_emul_rescale_add.argtypes, L.ks_group_emul_rescale_add.restype = [u64, u64, u64, u64], u64
    L.ks_group_emul_check.argtypes = [i32, i32, i64, i32, i32, i32, i32, i32, i32, i64, i32, u64, C.c_char_p, C.c_size_t]
    L.ks_group_emul_check.restype = i32
    return L


def test_every_host_check_in_the_headers_order(emul):
    """the function tfhe_keyswitch_grouped / tfhe_rotate_grouped run first (csrc/ks_group_core.h ks_group_check), on a ring of
    L = 8 limbs and N = 64: every call breaks one rule and later ones too where it can, and must report the earliest"""
    msg = C.create_string_buffer(200)

    def call(null=0, L=8, N=64, Lk=6, level=4, k=2, group=2, nd=2, polys=2, batch=1, rot=0, g=3):
        rc = emul.ks_group_emul_check(null, L, N, Lk, level, k, group, nd, polys, batch, rot, g, msg, len(msg))
        return rc, msg.value.decode()
    assert call() == (native.OK, "")
    assert call(polys=3, batch=0, nd=5, group=100, level=1) == (native.OK, "")
    # 1. a null argument, ahead of everything
    assert call(null=1, polys=4, Lk=0, k=9, group=0, level=0, nd=0, batch=-1) == (native.E_BADARG, "null argument")
    # 2. polys
    for p in (1, 4, 0):
        rc, m = call(polys=p, Lk=9, k=-1, group=0, level=0, nd=0, batch=-1)
        assert rc == native.E_BADARG and "2- or 3-element" in m, p
    # 3. key_limbs outside [1, L]
    for lk in (0, -1, 9):
        rc, m = call(Lk=lk, k=5, group=0, level=0, nd=0, batch=-1)
        assert rc == native.E_BADARG and "key_limbs" in m, lk
    # 4. n_special outside [0, min(4, key_limbs - 1)]
    for lk, k in ((6, -1), (6, 5), (8, 5), (3, 3), (1, 1)):
        rc, m = call(Lk=lk, k=k, group=0, level=0, nd=0, batch=-1)
        assert rc == native.E_BADARG and "n_special" in m, (lk, k)
    assert call(Lk=5, k=4, level=1, nd=1)[0] == native.OK and call(Lk=3, k=2, level=1, nd=1)[0] == native.OK
    # 5. group < 1
    for grp in (0, -2):
        rc, m = call(group=grp, level=0, nd=0, batch=-1)
        assert rc == native.E_BADARG and "group" in m, grp
    # 6. level outside [1, key_limbs - n_special]: TFHE_E_LEVEL_MISMATCH
    for lv in (0, -1, 5, 6):
        rc, m = call(level=lv, nd=0, batch=-1)
        assert rc == native.E_LEVEL and "level" in m, lv
    # 7. too few key components: TFHE_E_PARAMS_MISMATCH
    for lv, grp, nd in ((4, 2, 1), (3, 2, 1), (4, 1, 3), (4, 3, 1), (4, 4, 0)):
        rc, m = call(level=lv, group=grp, nd=nd, batch=-1)
        assert rc == native.E_PARAMS and "components" in m, (lv, grp, nd)
    assert call(level=3, group=2, nd=2)[0] == native.OK and call(level=4, group=4, nd=1)[0] == native.OK
    # 8. more working limbs than the engine holds (a ring of more than 40 limbs): TFHE_E_UNSUPPORTED
    rc, m = call(L=64, Lk=44, level=40, k=4, group=4, nd=10, batch=-1)
    assert rc == native.E_UNSUPPORTED and "working limbs" in m
    assert call(L=64, Lk=44, level=36, k=4, group=4, nd=9)[0] == native.OK
    # 9. a negative batch, ahead of the Galois element
    rc, m = call(batch=-1, rot=1, g=4)
    assert rc == native.E_BADARG and "negative batch" in m
    # 10. the Galois element: odd and below 2N (tfhe_rotate_grouped only)
    for g in (0, 4, 128, 129, 2**63 + 1):
        rc, m = call(rot=1, g=g)
        assert rc == native.E_BADARG and "odd and below 2N" in m, g
    assert call(rot=1, g=127)[0] == native.OK and call(rot=0, g=4)[0] == native.OK
    # 12. an empty batch is fine
    assert call(batch=0, rot=1)[0] == native.OK


# ---- the kernel bodies on the CPU ------------------------------------------------------------------------------------------

def _planted(qs_group, rng, count):
    """residues [count + 5][k] of random integers below Q_g and of 0, 1, Q_g - 1, Q_g // 2, Q_g // 2 + 1, with the integers"""
    Qg = math.prod(qs_group)
    ints = [rng.randrange(Qg) for _ in range(count)] + [0, 1, Qg - 1, Qg // 2, Qg // 2 + 1]
    return np.array([[x % q for q in qs_group] for x in ints], dtype=np.uint64), ints, Qg


def _emul_digits(emul, G, a, t, x):
    a, t = np.array(a, dtype=np.uint64), np.array(t, dtype=np.uint64)
    out = np.zeros((x.shape[0], len(t)), dtype=np.uint64)
    slow = emul.ks_group_emul_digits(G, len(a), a.ctypes.data, len(t), t.ctypes.data, x.shape[0], np.ascontiguousarray(x).ctypes.data, out.ctypes.data)
    assert slow >= 0
    return out, slow


DIGIT_RINGS = [H.chain(30, 8, 64), _mixed(64) + H.chain(41, 2, 64), H.chain(50, 4, 64) + H.chain(61, 2, 64)]


@pytest.mark.parametrize("G", [1, 2, 3, 4, 0])
@pytest.mark.parametrize("ring", range(len(DIGIT_RINGS)))
def test_digit_body_against_the_oracle_at_the_edges_of_every_group(emul, G, ring):
    """every group size the instantiation takes (a group cut short included; G = 0, the run-time loop, also 5 and 6 limbs), its limbs
    among the targets (the copy path) and outside them, random integers and the five planted ones"""
    qs = DIGIT_RINGS[ring]
    rng = random.Random(10 * G + ring)
    total_slow = 0
    for k in (range(1, G + 1) if G else (1, 3, 5, 6)):
        if k > len(qs) - 1:
            continue
        for start in (0, 1):
            group = qs[start:start + k]
            x, ints, Qg = _planted(group, rng, 40)
            got, slow = _emul_digits(emul, G, group, qs, x)
            cen = [v - Qg if v > Qg // 2 else v for v in ints]
            want = np.array([[c % q for q in qs] for c in cen], dtype=np.uint64)
            assert np.array_equal(got, want), (G, k, start)
            if start == 0:   # the oracle's own digits: one group of k limbs, every other limb of the ring a "special prime"
                assert np.array_equal(KO.digits(qs, len(qs), k, len(qs) - k, k, x.T[None])[0, 0], want.T)
            total_slow += slow
            if k == 1:   # a group of one is the per-limb digit of tfhe_keyswitch
                lift = np.array([[emul.ks_group_emul_lift_digit(int(v[0]), group[0], q) for q in qs] for v in x], dtype=np.uint64)
                assert np.array_equal(got, lift), (G, start)
    print(f"G={G} ring={ring}: exact multi-word branch taken {total_slow} times")


def test_planted_integers_take_the_exact_multi_word_branch(emul):
    """Q_g // 2 lifts to x' = Q_g - 1, whose fixed-point fraction is within the slack of wrapping once Q_g passes 2^64: the planted
    inputs must be decided by conv_prepare's exact comparison (counted by TFHE_EMUL_COUNT_SLOW), and decided right"""
    qs = H.chain(40, 6, 64)
    for G, k in ((2, 2), (3, 3), (4, 4), (0, 5)):
        group = qs[:k]
        Qg = math.prod(group)
        ints = [Qg // 2, Qg // 2 - 1, Qg // 2 + 2]
        x = np.array([[v % q for q in group] for v in ints], dtype=np.uint64)
        got, slow = _emul_digits(emul, G, group, qs, x)
        assert slow > 0, (G, k)
        want = np.array([[(v - Qg if v > Qg // 2 else v) % q for q in qs] for v in ints], dtype=np.uint64)
        assert np.array_equal(got, want), (G, k)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("case", ["below", "above", "mixed"])
def test_tail_body_is_k_modswitch_steps_the_last_special_prime_first(emul, K, case):
    """special primes below every ciphertext limb, above every one, and a 60-bit limb beside 40-bit ones: the unsigned reduction of
    `last` in both directions; random words and every word q - 1"""
    N = 64
    if case == "below":
        w = H.chain(40, 3, N) + H.chain(30, K, N)
    elif case == "above":
        w = H.chain(30, 3, N) + H.chain(50, K, N)
    else:
        w = H.chain(60, 1, N) + H.chain(40, 2, N) + (H.chain(41, K - 1, N) + H.chain(61, 1, N) if K > 1 else H.chain(61, 1, N))
    level, nw = 3, 3 + K
    rng = np.random.default_rng(K)
    t = np.stack([rng.integers(0, q, size=50, dtype=np.uint64) for q in w], axis=1)
    t = np.concatenate([t, np.array([[q - 1 for q in w], [0] * nw, [q - 1 for q in w[:level]] + [0] * K, [0] * level + [q - 1 for q in w[level:]]],
                                    dtype=np.uint64)])
    out = np.zeros((t.shape[0], level), dtype=np.uint64)
    wa = np.array(w, dtype=np.uint64)
    assert emul.ks_group_emul_tail(K, level, wa.ctypes.data, t.shape[0], np.ascontiguousarray(t).ctypes.data, out.ctypes.data) == 0
    cur = [[int(v) for v in row] for row in t]
    for step in range(K):                                  # crt.jl:215-220 on Python integers
        ql = w[nw - 1 - step]
        cur = [[pow(ql, -1, w[j]) * (row[j] - row[-1] % w[j]) % w[j] for j in range(len(row) - 1)] for row in cur]
    assert np.array_equal(out, np.array(cur, dtype=np.uint64)), (K, case)
    if K == 1:   # the words of k_ks_rescale_add
        ra = np.array([[emul.ks_group_emul_rescale_add(int(row[j]), int(row[level]), w[j], w[level]) for j in range(level)] for row in t], dtype=np.uint64)
        assert np.array_equal(out, ra)


@KH.needs_hipcc
def test_gfx950_code_objects_use_no_scratch(tmp_path):
    """figures only: k_ks_group_digits<1..4> and k_ks_group_tail<1..4>, one and two coefficients per thread, hold their residues in
    registers (no scratch, no LDS); the run-time-loop form of the digits (G = 0) may spill"""
    recs = [r for r in KH.kernel_resources("ks_group_emul/resource_probe.hip", tmp_path) if "ks_group" in r["name"]]
    digits = {n: r for r in recs for n in [r["name"]] if "k_ks_group_digitsILi" in n}
    tails = {n: r for r in recs for n in [r["name"]] if "k_ks_group_tailILi" in n}
    assert len(digits) == 10 and len(tails) == 8, sorted(r["name"] for r in recs)
    for n, r in {**digits, **tails}.items():
        print(n, r)
        if "digitsILi0E" in n:
            continue
        assert r["scratch"] == 0 and r["static_lds"] == 0, r
        assert r["vgprs"] <= 128, r                       # four waves per SIMD at least


# ---- the mirror ---------------------------------------------------------------------------------------------------------------

def _stub_params(qs):
    ring = types.SimpleNamespace(L=len(qs), moduli=list(qs), N=64)
    inner = types.SimpleNamespace(relin_window=0, sigma=3.2, scheme_name="CKKS", R_key=lambda: ring, R_cipher=lambda: ring)
    return ring, inner


@pytest.mark.parametrize("Lk,k,alpha", [(6, 2, 2), (7, 3, 3), (6, 0, 4), (5, 1, 1), (6, 4, 5)])
def test_grouped_raised_gadget_table_is_the_oracles(Lk, k, alpha):
    qs = H.chain(30, Lk, 64)
    ring, inner = _stub_params(qs)
    gp = she.GroupedRaised(inner, k, alpha)
    table = she._gadget_table(gp, ring)
    assert table == KO.gadget_table(qs, k, alpha)
    assert len(table) == -(-(Lk - k) // alpha) and [list(G) for G in gp.digit_groups(Lk - k)] == [list(G) for G in KO.groups(Lk - k, alpha)]
    if (k, alpha) == (1, 1):   # ModulusRaised's table with the special prime's own (zero) row dropped
        assert table == she._gadget_table(she.ModulusRaised(inner), ring)[:Lk - 1]


def test_grouped_raised_refuses_what_it_cannot_take():
    qs = H.chain(30, 6, 64)
    ring, inner = _stub_params(qs)
    for k, alpha in ((-1, 1), (5, 1), (6, 1), (1, 0)):
        with pytest.raises(she.UsageError, match="n_special"):
            she.GroupedRaised(inner, k, alpha)
    windowed = types.SimpleNamespace(**{**inner.__dict__, "relin_window": 8})
    with pytest.raises(she.UsageError, match="relin_window"):
        she.GroupedRaised(windowed, 1, 1)
    gp = she.GroupedRaised(inner, 2, 2)
    ksk = types.SimpleNamespace(params=gp, key=[None])
    gk = she.GaloisKey(3, ksk)
    ct = types.SimpleNamespace(params=gp)
    with pytest.raises(she.UsageError, match="mul_relin has no support for keys with grouped digits"):
        she.mul_relin(she.EvalMultKey(ksk), ct, ct)
    with pytest.raises(she.UsageError, match="GaloisKey.prepared"):
        gk.prepared()
    for name, call in (("rotate_many", lambda: she.rotate_many([gk], [0, 0])), ("matmul_diag", lambda: she.matmul_diag([gk], [], [0, 0])),
                       ("matmul_bsgs", lambda: she.matmul_bsgs([gk], [], [], [0, 0])), ("matmul_bsgs", lambda: she.matmul_bsgs([], [gk], [], [0, 0])),
                       ("matmul_bsgs_blocks", lambda: she.matmul_bsgs_blocks([gk], [], [[]], [[0, 0]])),
                       ("matmul_bsgs_fold", lambda: she.matmul_bsgs_fold([], [], [[]], [[0, 0]], [[gk]])),
                       ("rotate_sum", lambda: she.rotate_sum([[gk]], [0, 0]))):
        with pytest.raises(she.UsageError, match=f"{name}.* has no support for keys with grouped digits"):
            call()
