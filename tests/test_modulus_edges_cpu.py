"""Modulus size-class edges without a GPU: the class thresholds of tests/helpers.py read back out of the engine's sources (so
the edge tests follow a moved bound instead of quietly testing the comfortable end of a class), the kernel bodies under
tests/emul at the primes where each range budget binds, and the C ABI's refusal of moduli from 2^62 up."""
import os
import random
import re

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu, spec
from tests import helpers as H
from tests import kernel_harness as KH
from tests.emul import emul

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "toyfhe.jl_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_class_thresholds_match_the_engine_sources(tmp_path):
    fp = _src("fp64arith.h")
    assert int(re.search(r"#define TFHE_FP_QMAX (\d+)ull", fp).group(1)) == H.FP_QMAX
    assert (1 << int(re.search(r"#define TFHE_FPS_QMAX \(1ull << (\d+)\)", fp).group(1))) == H.FPS_QMAX
    k = _src("kernels.h")
    # k_ks_inner: fold above 52 bits, DCH terms up to 61 bits and KS_FOLD_LAZY_62 at 62; k_ks_inner_n2 (acc52) up to 52
    assert int(re.search(r"const bool fold = qbits > (\d+);", k).group(1)) == H.FOLD_BITS
    assert int(re.search(r"const int lazy = fold \? \(qbits <= 61 \? DCH : (\d+)\)", k).group(1)) == H.KS_FOLD_LAZY_62
    assert re.search(r'static_assert\(DCH <= 15, "fold budget at 61 bits"\)', k)
    assert re.search(r'static_assert\(DCH \+ 1 <= 16, "acc52 term budget"\)', k)
    # the chunk of every Barrett-window sum kernel: the rule is written in ONE function (lazy_sum.h lazy_chunk) over all of csrc/
    # (bfv_tables.h's `room = 62 - bits` is the conversions' own rule, below), every such kernel calls it, and compiled for the host
    # (tests/md_acc_emul/) it gives H.sum_chunk at the smallest and the largest modulus of every bit length
    code = {f: re.sub(r"//[^\n]*", "", _src(f)) for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".inc", ".hip"))}
    rule = r"(?<!room = )62 - bits"
    assert [f for f, text in code.items() if re.search(rule, text)] == ["lazy_sum.h"]
    body = re.search(r"\nTFHE_HD u32 lazy_chunk\(u64 q\) \{\n(.*?)\n\}\n", code["lazy_sum.h"], re.S).group(1)
    assert len(re.findall(rule, body)) == len(re.findall(rule, code["lazy_sum.h"])) >= 1
    assert not any(re.search(r"\bchunk = bits\b", text) for text in code.values())
    for f, kernel in (("kernels.h", "k_dot"), ("kernels.h", "k_lincomb"), ("kernels.h", "k_lincomb_many"), ("dot_core.h", "k_dot_view"),
                      ("kernels.h", "k_md_acc"), ("kernels.h", "k_md_acc_dense")):
        bodies = re.findall(r"\bvoid %s\(.*?\n\}\n" % kernel, code[f], re.S)
        assert len(bodies) == 1 and len(re.findall(r"\bchunk = (?:\(int\))?lazy_chunk\(L\.q\);", bodies[0])) == 1, kernel
    lazy_chunk = KH.md_acc_emul(tmp_path).md_acc_emul_chunk
    for bits in range(2, 63):
        for q in ((1 << bits) - 1, 1 << (bits - 1)):
            assert lazy_chunk(q) == H.sum_chunk(bits), (bits, q)
    b = _src("bfv_tables.h")
    rooms = re.findall(r"room = (\d+) - (?:max)?bits;", b)
    assert rooms == ["62", "62"], rooms
    m = re.search(r"auto lazy_of = \[\]\(int bits, int k\) \{ const int room = (\d+) - bits; return std::max\(1, std::min\(k, "
                  r"room >= (\d+) \? \(1 << (\d+)\) : \(1 << std::max\(0, room\)\)\)\); \};", b)
    room0, big, bigexp = (int(x) for x in m.groups())
    for bits in range(2, 63):
        for k in (1, 2, 3, 14, 40):
            room = room0 - bits
            assert max(1, min(k, (1 << bigexp) if room >= big else 1 << max(0, room))) == H.conv_lazy(bits, k), (bits, k)
    assert "B.narrow = (maxmod < TFHE_FP_QMAX && ns + 2 <= 16 && np + 2 <= 16)" in b
    h = _src("toyfhe_hip.hip")
    assert int(re.search(r"return 1ll << \(\(l >= 0 && l < 40\) \? l : (\d+)\);", h).group(1)) == 20 == H.MIXED_MIN_WORDS.bit_length() - 1
    assert "q[l] >= (1ull << 62)" in h and H.Q_LIMIT == 1 << 62
    # ArithFpS only behind the plan's flag, and the flag only after EVERY working limb was compared against TFHE_FPS_QMAX
    ks = _src("ks_api.inc")
    assert "for (int j = 0; j < nw; j++) small = small && c->q[A.w.idx[j]] < TFHE_FPS_QMAX;" in ks
    assert len(re.findall(r"\bfps = ", ks)) == 1 and "P.fps = small && fps_on;" in ks
    assert len(re.findall(r"\?\s*k_ks_fused_sub<ArithFpS", ks)) == 2 == len(re.findall(r"P\.fps \? k_ks_fused_sub<ArithFpS", ks))
    assert "ArithFpS" not in h


def test_range_plans_cover_their_class_tops():
    """The fp64 range plans are computed for a = TFHE_FP_A (TFHE_FPS_A) and sweep before TFHE_FP_LIMIT p (TFHE_FPS_LIMIT p).  They
    prove exactness only for moduli with q 2^-52 <= a and limit < 2^53 / q, so a class threshold moved past either bound is
    wrong even when no input reaches the plan's worst case (measured on the edge rows: about half of the exactness limit)."""
    fp = _src("fp64arith.h")
    num = lambda name: float(re.search(r"#define %s ([0-9.]+)" % name, fp).group(1))
    for qmax, a, lim in ((H.FP_QMAX, num("TFHE_FP_A"), num("TFHE_FP_LIMIT")), (H.FPS_QMAX, num("TFHE_FPS_A"), num("TFHE_FPS_LIMIT"))):
        assert qmax * 2.0**-52 <= a, (qmax, a)
        assert lim < 2.0**53 / qmax, (qmax, lim)


@pytest.mark.parametrize("N", [1 << 10, 1 << 14])
def test_edge_prime_helpers(N):
    for bound in (H.FPS_QMAX, H.FP_QMAX, 1 << 52, 1 << 62, 1 << 31):
        below, above = H.primes_below(bound, 3, N), H.primes_above(bound, 3, N)
        assert below == sorted(below, reverse=True) and above == sorted(above)
        for q in below + above:
            assert spec.is_prime(q) and (q - 1) % (2 * N) == 0
        assert below[0] < bound < above[0]
        # nothing NTT-friendly is skipped between them
        assert not any(spec.is_prime(q) for q in range(below[0] + 2 * N, above[0], 2 * N))
    for k, bits in ((9, 61), (5, 62)):
        q = H.primes_above_ratio(k, bits, 2, N)[0]
        assert q > (1 << 64) // k and (1 << 64) % q > q - (k + 1) * 2 * N * 64


def _pats(q, N, seed):
    """growth-maximising rows: all q - 1, alternating 0 / q - 1, all (q -+ 1)/2, centring edges, one uniform row"""
    rng = np.random.default_rng(seed)
    e = np.array([0, 1, q - 1, q // 2, q // 2 + 1] * (N // 5 + 1), dtype=np.uint64)[:N]
    return [np.full(N, q - 1, dtype=np.uint64), np.array([0, q - 1] * (N // 2), dtype=np.uint64),
            np.full(N, (q - 1) // 2, dtype=np.uint64), np.full(N, (q + 1) // 2, dtype=np.uint64), e,
            rng.integers(0, q, size=N, dtype=np.uint64)]


def _edge_ntt_primes(N):
    return {"fp-top": H.primes_below(H.FP_QMAX, 1, N)[0], "u64-bottom": H.primes_above(H.FP_QMAX, 1, N)[0],
            "fold61": H.primes_above_ratio(9, 61, 1, N)[0], "fold62": H.primes_above_ratio(5, 62, 1, N)[0],
            "top62": H.primes_below(H.Q_LIMIT, 1, N)[0]}


@pytest.mark.parametrize("logn", [10, 11, 12, 13, 14])
@pytest.mark.parametrize("which", ["fp-top", "u64-bottom", "fold61", "fold62", "top62"])
def test_ntt_bodies_at_the_class_edges(logn, which):
    """ntt_core.h block bodies (variant 0: the policy the modulus selects, 1: generic radix-2, 2: u64 forced) at the top of the
    fp64 class, the bottom of the u64 class, the fold primes and the largest prime below 2^62 (lazy range 4q < 2^64), on
    growth-maximising coefficient- and evaluation-domain rows.  The fp64 budget (every operand below 2^53) is asserted where it
    applies; the u64 primes must not touch the fp64 path at all."""
    N = 1 << logn
    q = _edge_ntt_primes(N)[which]
    ctx = ref_cpu.RefCtx(N, [q])
    emul.fp_max_ratio_reset()
    for a in _pats(q, N, logn):
        want = ctx.nntt(a.reshape(1, 1, N)).reshape(N)
        wi = ctx.inntt(a.reshape(1, 1, N)).reshape(N)
        for variant in (0, 1, 2):
            assert np.array_equal(emul.ntt(a, q, variant=variant), want), (which, variant)
            assert np.array_equal(emul.ntt(want, q, inverse=True, variant=variant), a), (which, variant)
            assert np.array_equal(emul.ntt(a, q, inverse=True, variant=variant), wi), (which, variant)
    worst = emul.fp_max_ratio_reset()
    if q < H.FP_QMAX:
        assert 0 < worst < 2.0**53 / q, worst
    else:
        assert worst == 0, worst


def _conv_want(a, t, res, centred):
    A = 1
    for x in a:
        A *= x
    out = []
    for r in res:
        x = spec.rns_to_int([int(v) for v in r], a)
        if centred:
            x = spec.centred(x, A)
        out.append([x % ti for ti in t])
    return np.array(out, dtype=np.uint64)


def _edge_bases(k, m, N=64):
    """source / target bases of k / m primes at each class edge"""
    return {"fp-top": H.primes_below(H.FP_QMAX, k + m, N), "u64-bottom": H.primes_above(H.FP_QMAX, k + m, N),
            "top62": H.primes_below(H.Q_LIMIT, k + m, N), "fold62": H.primes_above_ratio(5, 62, k + m, N),
            "below31": H.primes_below(1 << 31, k + m, N), "top52": H.primes_below(1 << 52, k + m, N)}


@pytest.mark.parametrize("which", ["fp-top", "u64-bottom", "top62", "fold62", "below31", "top52"])
@pytest.mark.parametrize("k,m", [(14, 14), (3, 4), (1, 2)])
@pytest.mark.parametrize("centred", [False, True])
def test_exact_conversion_bodies_at_the_class_edges(which, k, m, centred):
    """conv_core.h: lazy = 2^(62 - maxbits) products between two reductions (1 at 62 bits), all residues q - 1 and the alpha /
    centring boundaries, 14-prime bases at the top of the fp64 class, primes below 2^31"""
    ch = _edge_bases(k, m)[which]
    a, t = ch[:k], ch[k:]
    A = 1
    for x in a:
        A *= x
    rng = random.Random(k * 100 + m)
    vals = [0, 1, 2, A - 1, A - 2, A // 2, A // 2 + 1, A // 2 - 1, A // 2 + 2, A - A // a[0]]
    vals += [rng.randrange(A) for _ in range(60)]
    res = np.array([[v % x for x in a] for v in vals], dtype=np.uint64)
    res[-1] = np.array(a, dtype=np.uint64) - 1                       # every residue q - 1: the largest lazy sum
    got, _ = emul.conv(a, t, res, centred)
    assert np.array_equal(got, _conv_want(a, t, res, centred))


def _bfv_edge(which, ns, nextra, N=32):
    n = 2 * ns + nextra + 1
    return _edge_bases(n, 0, N)[which][::-1] if which in ("fp-top", "top62", "below31", "top52") else _edge_bases(n, 0, N)[which]


def _bfv_inputs(qs, pb, t, N, seed):
    small, big = spec.Ring(N, qs), spec.Ring(N, pb)
    rng = np.random.default_rng(seed)
    a = np.stack([rng.integers(0, q, size=(4, N), dtype=np.uint64) for q in qs], axis=1)
    for k, x in enumerate([0, 1, small.Q - 1, small.Q // 2, small.Q // 2 + 1, 7, small.Q - 7]):
        a[0, :, k] = [x % q for q in qs]
    a[1] = (np.array(qs, dtype=np.uint64) - 1)[:, None]
    y = np.stack([rng.integers(0, p, size=(4, N), dtype=np.uint64) for p in pb], axis=1)
    tinv = pow(t, -1, big.Q)
    edges = [0, 1, big.Q - 1, big.Q // 2, big.Q // 2 + 1, small.Q // 2, small.Q // 2 + 1, small.Q, small.Q - 1,
             3 * small.Q + small.Q // 2, 3 * small.Q + small.Q // 2 + 1, big.Q - small.Q // 2, big.Q - small.Q // 2 - 1]
    for k, x in enumerate(edges):
        y[0, :, k] = [(x * tinv) % big.Q % p for p in pb]
    y[1] = (np.array(pb, dtype=np.uint64) - 1)[:, None]
    return a, y


@pytest.mark.parametrize("which,ns,nextra", [("fp-top", 14, 0), ("u64-bottom", 14, 0), ("top62", 3, 1), ("fold62", 6, 1),
                                             ("below31", 8, 1), ("below31", 3, 1), ("top52", 3, 1)])
@pytest.mark.parametrize("mode", ["superset", "disjoint"])
def test_bfv_bodies_at_the_class_edges(which, ns, nextra, mode):
    """bfv_core.h expand / contract (the general kernels, Barrett sums of lazy = 2^(62 - maxbits) products) at the edge rings:
    14 + 14 limbs at the top of the fp64 class and just above it, 62-bit moduli (lazy = 1), primes below 2^31.  (The narrow
    acc52 bodies are bfv_fast.h only, for the compiled (ns, np) pairs: test_bfv_fast_bodies_at_the_class_edges.)"""
    N, t = 32, 65537
    ch = _bfv_edge(which, ns, nextra, N)
    qs = ch[:ns]
    pb = ch[: 2 * ns + nextra] if mode == "superset" else ch[ns: 2 * ns + nextra + 1]
    cs, cb = ref_cpu.RefCtx(N, qs), ref_cpu.RefCtx(N, pb)
    a, y = _bfv_inputs(qs, pb, t, N, ns + len(which))
    got, _ = emul.bfv(qs, pb, t, a, N, contract=False)
    assert np.array_equal(got, ref_cpu.switch(cs, cb, a))
    got, _ = emul.bfv(qs, pb, t, y, N, contract=True)
    assert np.array_equal(got, ref_cpu.contract(cb, cs, t, y))


@pytest.mark.parametrize("which,ns,np_", [("fp-top", 8, 9), ("u64-bottom", 8, 9), ("top62", 6, 7), ("fold62", 3, 4),
                                          ("below31", 3, 4), ("below31", 6, 7), ("top52", 2, 3), ("fp-top", 2, 3)])
def test_bfv_fast_bodies_at_the_class_edges(which, ns, np_):
    """bfv_fast.h (register-resident conversions: the narrow acc52 / acc52_redc bodies below TFHE_FP_QMAX -- at most NS + 2 = 10
    and NP + 2 = 11 terms at (8, 9), carries that must fit 32 bits at primes with large low 26 bits, a single final
    subtraction at primes below 2^31 -- and the wide bodies above) at the edge rings"""
    N, t = 32, 65537
    ch = _edge_bases(ns + np_, 0, N)[which]
    qs = ch[:ns]
    pb = ch[ns:] + ch[:ns]
    cs, cb = ref_cpu.RefCtx(N, qs), ref_cpu.RefCtx(N, pb)
    a, y = _bfv_inputs(qs, pb, t, N, ns * 10 + np_)
    assert np.array_equal(emul.bfv_fast(qs, pb, t, a, N, contract=False), ref_cpu.switch(cs, cb, a))
    assert np.array_equal(emul.bfv_fast(qs, pb, t, y, N, contract=True), ref_cpu.contract(cb, cs, t, y))


def test_moduli_from_2_62_up_are_refused_before_device_use():
    """tfhe_ctx_create: every modulus must be a prime below 2^62 (TFHE_E_BADARG), checked on the host like
    test_abi_cpu.test_argument_validation_precedes_device_use"""
    for N in (16, 1 << 10):
        q = H.primes_above(H.Q_LIMIT, 1, N)[0]
        with pytest.raises(AssertionError, match="below 2\\^62"):
            tf.Context(N, [q])
        with pytest.raises(AssertionError, match="below 2\\^62"):
            tf.Context(N, [H.primes_below(H.Q_LIMIT, 1, N)[0], q])
