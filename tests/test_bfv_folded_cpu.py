"""The narrow BFV conversion bodies after the fold (csrc/bfv_fast.h), on the CPU: the contraction on rows that arrive multiplied by
their per-limb input constants (FOLDED) with three-product sums -- against the C oracle, against the general bodies (bfv_core.h)
and against the unfolded narrow forms, which keep their four-product sums -- and the narrow expansion, which shares the
accumulator type and keeps four products as well.  Inputs: all 0, all
p - 1, the centred extremes a transform output may take, rows that force the exact-alpha decision in each conversion, and a few
thousand random coefficients.  The lanes that reached acc52_redc are checked against the limits its proof states (modarith.h)."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_cpu
from tests import helpers as H
from tests import kernel_harness as KH
from tests.emul import emul

N, T = 4096, 65537
u64p = C.POINTER(C.c_uint64)

# limits of the lanes handed to acc52_redc (modarith.h: "s0 < 2^56 + 2^52, s1 and s2 less"; s2 sums 16 products of two high halves,
# each below 2^25: < 2^53, the bound the reduction's header states) and of psum's middle lane (bfv_fast.h: below 2^57)
LANE_LIMITS = ((1 << 56) + (1 << 52), 1 << 57, 1 << 53, 1 << 57)


@pytest.fixture(scope="module")
def bodies(tmp_path_factory):
    L = KH.build_emul("bfv_folded_emul/bfv_folded_emul.cpp", tmp_path_factory.mktemp("bfv_folded_emul"))
    L.bfvf_run.argtypes = [u64p, C.c_int, u64p, C.c_int, C.c_uint64, C.c_int, C.c_int64, u64p, u64p, u64p, C.POINTER(C.c_int64)]
    L.bfvf_run.restype = C.c_int
    L.bfvf_kappa.argtypes = [u64p, C.c_int, u64p, C.c_int, C.c_uint64, u64p, u64p, C.POINTER(C.c_double)]
    L.bfvf_kappa.restype = C.c_int

    class Bodies:
        @staticmethod
        def run(qs, pb, mode, src):
            """src [limbs in][n] -> (out [limbs out][n], lane maxima [4], exact-alpha hits by source limb count [17])"""
            qa, pa = np.array(qs, dtype=np.uint64), np.array(pb, dtype=np.uint64)
            src = np.ascontiguousarray(src, dtype=np.uint64)
            n = src.shape[1]
            out = np.zeros((len(pb) if mode == 0 else len(qs), n), dtype=np.uint64)
            lanes, hits = np.zeros(4, dtype=np.uint64), np.zeros(17, dtype=np.int64)
            rc = L.bfvf_run(qa.ctypes.data_as(u64p), len(qs), pa.ctypes.data_as(u64p), len(pb), T, mode, n, src.ctypes.data_as(u64p),
                            out.ctypes.data_as(u64p), lanes.ctypes.data_as(u64p), hits.ctypes.data_as(C.POINTER(C.c_int64)))
            assert rc == 0, rc
            return out, [int(x) for x in lanes], hits

        @staticmethod
        def kappa(qs, pb, ninv):
            qa, pa = np.array(qs, dtype=np.uint64), np.array(pb, dtype=np.uint64)
            nv = np.array(ninv, dtype=np.uint64)
            k, f = np.zeros(len(pb), dtype=np.uint64), np.zeros(len(pb), dtype=np.float64)
            rc = L.bfvf_kappa(qa.ctypes.data_as(u64p), len(qs), pa.ctypes.data_as(u64p), len(pb), T, nv.ctypes.data_as(u64p),
                              k.ctypes.data_as(u64p), f.ctypes.data_as(C.POINTER(C.c_double)))
            assert rc == 0, rc
            return [int(x) for x in k], [float(x) for x in f]
    return Bodies


def _moduli(kind, n):
    if kind == "top":        # just below TFHE_FP_QMAX: the lane budget and the Montgomery bounds are tight
        return H.primes_below(H.FP_QMAX, n, N)
    if kind == "bench50":    # the benchmark's chain: the first primes above 2^50 that serve N = 2^14 (and so this N)
        return H.chain(50, n, 16384)
    return H.primes_below(1 << 30, n, N)   # 30 bits: where the r < 2 p argument of acc52_redc was once wrong


def _setup(kind, ns, np_):
    ch = _moduli(kind, ns + np_)
    qs = ch[:ns]
    pb = ch[ns:] + ch[:ns]          # P limbs first, shared limbs last
    pb = pb[1:] + pb[:1]            # rotate: positions are arbitrary
    Qs = 1
    for q in qs:
        Qs *= q
    Pp = 1
    for p in ch[ns:]:
        Pp *= p
    return qs, pb, Qs, Pp


_CTX = {}


def _ctx(qs):
    key = tuple(qs)
    if key not in _CTX:
        _CTX[key] = ref_cpu.RefCtx(N, list(qs))
    return _CTX[key]


def _columns(values, mods):
    """integers -> residues [len(mods)][len(values)]"""
    return np.array([[v % m for v in values] for m in mods], dtype=np.uint64)


def _centred_doubles(res, mods):
    """canonical residues [limbs][n] -> the centred representative of each as the bit pattern of its double"""
    m = np.array(mods, dtype=np.int64).reshape(-1, 1)
    c = res.astype(np.int64)
    c = np.where(c > m // 2, c - m, c)
    return c.astype(np.float64).view(np.uint64)


def _times(res, consts, mods):
    """residues [limbs][n] times one constant per limb, mod the limb's modulus (exact: Python integers)"""
    return np.array([[(int(x) * k) % m for x in row] for row, k, m in zip(res, consts, mods)], dtype=np.uint64)


PAIRS = [(2, 3), (8, 9)]
KINDS = ["top", "bench50", "bits30"]


@pytest.mark.parametrize("ns,np_", PAIRS)
@pytest.mark.parametrize("kind", KINDS)
def test_folded_contraction_body(bodies, kind, ns, np_):
    qs, pb, Qs, Pp = _setup(kind, ns, np_)
    Q = Qs * Pp
    cs, cb = _ctx(qs), _ctx(pb)
    kappa, _ = bodies.kappa(qs, pb, [1] * len(pb))
    rng = np.random.default_rng(ns * 100 + len(kind))
    y = np.stack([rng.integers(0, p, size=N, dtype=np.uint64) for p in pb])       # a few thousand random coefficients
    y[:, 0] = 0                                                                   # all residues 0
    y[:, 1] = np.array(pb, dtype=np.uint64) - 1                                   # all residues p - 1
    tinv = pow(T, -1, Q)
    # first conversion (out of ℛ): t y + h within a few units of a multiple of q, on either side
    edges = [x * tinv % Q for x in (0, 1, Q - 1, Q // 2, Q // 2 + 1, Qs // 2, Qs // 2 + 1, Qs, Qs - 1, 3 * Qs + Qs // 2, 3 * Qs + Qs // 2 + 1,
                                    Q - Qs // 2, Q - Qs // 2 - 1, Qs * (Pp // 2), Qs * (Pp // 2) + Qs // 2 + 1)]
    # second conversion (out of P): round(t y / q) + floor(P/2) within a few units of a multiple of P, y ~ Q (2 k + 1) / (2 t)
    for k in (0, 1, T // 2, T - 1):
        centre = Q * (2 * k + 1) // (2 * T)
        edges += [(centre + d) % Q for d in (-Qs, -1, 0, 1, Qs)]
    y[:, 2:2 + len(edges)] = _columns(edges, pb)
    want = ref_cpu.contract(cb, cs, T, y[None])[0]
    general, _ = emul.bfv(qs, pb, T, y[None], N, contract=True)
    assert np.array_equal(general[0], want)
    words, lanes_w, _ = bodies.run(qs, pb, 1, y)                                   # the unfolded forms: canonical words ...
    assert np.array_equal(words, want)
    unfolded, lanes_u, _ = bodies.run(qs, pb, 2, _centred_doubles(y, pb))          # ... and reduced doubles
    assert np.array_equal(unfolded, want)
    yk = _centred_doubles(_times(y, kappa, pb), pb)                                # what the core leaves under the folded table
    got, lanes, hits = bodies.run(qs, pb, 3, yk)
    assert np.array_equal(got, want)
    assert hits[ns] >= 1 and hits[np_] >= 1, (int(hits[ns]), int(hits[np_]))       # the exact-alpha decision, in each conversion
    for name, l in (("words", lanes_w), ("doubles", lanes_u), ("folded", lanes)):
        for lane, limit in zip(l, LANE_LIMITS):
            assert lane < limit, (name, [x.bit_length() for x in l])
    # c2's form: the same residues written as centred doubles
    lifted, _, _ = bodies.run(qs, pb, 4, yk)
    assert np.array_equal(lifted, _centred_doubles(want, qs))


@pytest.mark.parametrize("ns,np_", PAIRS)
@pytest.mark.parametrize("kind", KINDS)
def test_folded_contraction_takes_the_extremes_of_a_transform_output(bodies, kind, ns, np_):
    """|y'| <= p/2 + 1 is what the last stage of the transform guarantees whatever its constant: +-floor(p/2) and +-(floor(p/2) + 1)
    on every limb, alone and mixed with each other and with random rows"""
    qs, pb, Qs, Pp = _setup(kind, ns, np_)
    cs, cb = _ctx(qs), _ctx(pb)
    kappa, _ = bodies.kappa(qs, pb, [1] * len(pb))
    rng = np.random.default_rng(7 + ns)
    half = np.array([p // 2 for p in pb], dtype=np.int64).reshape(-1, 1)
    n = 256
    yk = np.empty((len(pb), n), dtype=np.int64)
    for c, e in enumerate((half, -half, half + 1, -(half + 1))):
        yk[:, c:c + 1] = e
    pick = rng.integers(0, 5, size=(len(pb), n - 4))
    rand = np.stack([rng.integers(-(p // 2), p // 2 + 1, size=n - 4) for p in pb])
    yk[:, 4:] = np.choose(pick, [np.broadcast_to(half, rand.shape), np.broadcast_to(-half, rand.shape),
                                 np.broadcast_to(half + 1, rand.shape), np.broadcast_to(-(half + 1), rand.shape), rand])
    kinv = [pow(k, -1, p) for k, p in zip(kappa, pb)]
    y = np.array([[(int(v) * ki) % p for v in row] for row, ki, p in zip(yk, kinv, pb)], dtype=np.uint64)   # the residues they stand for
    ypad = np.zeros((len(pb), N), dtype=np.uint64)
    ypad[:, :n] = y
    want = ref_cpu.contract(cb, cs, T, ypad[None])[0][:, :n]
    got, lanes, _ = bodies.run(qs, pb, 3, yk.astype(np.float64).view(np.uint64))
    assert np.array_equal(got, want)
    for lane, limit in zip(lanes, LANE_LIMITS):
        assert lane < limit, [x.bit_length() for x in lanes]


@pytest.mark.parametrize("ns,np_", PAIRS)
@pytest.mark.parametrize("kind", KINDS)
def test_expansion_body(bodies, kind, ns, np_):
    qs, pb, Qs, Pp = _setup(kind, ns, np_)
    cs, cb = _ctx(qs), _ctx(pb)
    rng = np.random.default_rng(ns * 10 + len(kind))
    a = np.stack([rng.integers(0, q, size=N, dtype=np.uint64) for q in qs])
    a[:, 0] = 0
    a[:, 1] = np.array(qs, dtype=np.uint64) - 1
    edges = [0, 1, Qs - 1, Qs // 2, Qs // 2 + 1, Qs // 2 - 1, Qs // 2 + 2, 7, Qs - 7]   # around the centring: the exact-alpha decision
    a[:, 2:2 + len(edges)] = _columns(edges, qs)
    want = ref_cpu.switch(cs, cb, a[None])[0]
    general, _ = emul.bfv(qs, pb, T, a[None], N, contract=False)
    assert np.array_equal(general[0], want)
    got, lanes, hits = bodies.run(qs, pb, 0, a)
    assert np.array_equal(got, want)
    assert hits[ns] >= 1, int(hits[ns])
    for lane, limit in zip(lanes, LANE_LIMITS):
        assert lane < limit, [x.bit_length() for x in lanes]


@pytest.mark.parametrize("kind", KINDS)
def test_fold_scales_the_closing_constants_only_by_kappa(bodies, kind):
    """bfv_fold_limb: N^-1 kappa mod p as the double the folded table holds; kappa = t (q/q_i)^-1 on an ℛ-limb, and on a P-limb
    t q^-1 (P/p_j)^-1 2^78, all mod the limb's prime"""
    ns, np_ = 2, 3
    qs, pb, Qs, Pp = _setup(kind, ns, np_)
    ninv = [pow(N, -1, p) for p in pb]
    kappa, folded = bodies.kappa(qs, pb, ninv)
    for l, p in enumerate(pb):
        if p in qs:
            want = T * pow(Qs // p, -1, p) % p
        else:
            want = T * pow(Qs, -1, p) * pow(Pp // p, -1, p) * pow(2, 78, p) % p
        assert kappa[l] == want
        assert folded[l] == float(ninv[l] * want % p)
