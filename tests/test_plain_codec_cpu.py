"""No-GPU checks of the BFV / BGV plaintext-codec bodies (toyfhe.jl_amd/csrc/plain_core.h): the CPU emulation harness
tests/plain_emul/plain_emul.cpp runs the very per-coefficient code and host table of the device kernels against the oracle
(spec.bfv_decode, spec.bgv_decode, spec.bfv_encode, and the noise remainder birem of she.invariant_noise_budget)."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import spec
from tests import kernel_harness as KH

WORDS = 40  # TFHE_MAX_LIMBS: words per noise remainder in the harness output
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    # (the warnings and the range tracker tests/emul/Makefile builds the general bodies with)
    L = KH.build_emul("plain_emul/plain_emul.cpp", tmp_path_factory.mktemp("plain_emul"),
                      ("-Wall", "-Wno-unused-function", "-DTFHE_EMUL_TRACK_RANGE"))
    L.plain_emul_run.argtypes = [u64p, C.c_int, C.c_uint64, C.c_int, C.c_int, u64p, u64p, C.c_long, C.POINTER(C.c_long)]
    L.plain_emul_km.argtypes = [C.c_int]
    return L


HITS = np.zeros(4, dtype=np.int64)  # quotient corrected down / up, exact tie, exact-α decision (summed over the module)


def _run(L, qs, t, op, inp, km=0):
    qa = np.array(qs, dtype=np.uint64)
    inp = np.ascontiguousarray(inp, dtype=np.uint64)
    n = inp.shape[0]
    width = {0: 1, 1: 1, 2: WORDS, 3: len(qs), 4: len(qs)}[op]
    out = np.zeros((n, width), dtype=np.uint64)
    hits = (C.c_long * 4)()
    rc = L.plain_emul_run(qa.ctypes.data_as(u64p), len(qs), t, op, km, inp.ctypes.data_as(u64p), out.ctypes.data_as(u64p), n, hits)
    if rc == 0:
        HITS[:] += np.array(list(hits), dtype=np.int64)
    return rc, out


def _residues(xs, qs):
    return np.array([[x % q for q in qs] for x in xs], dtype=np.uint64).reshape(len(xs), len(qs))


def _words(v):
    return [(v >> (64 * i)) & (2**64 - 1) for i in range(WORDS)]


def _birem(x, delta):
    r = x % delta
    return delta - r if r > delta // 2 else r


def _chain(bits, n, start_index=0):
    return spec.prime_chain(2**bits + 1, n + start_index, 1024)[start_index:]


RINGS = {
    "1x30": _chain(30, 1), "1x40": _chain(40, 1), "1x50": _chain(50, 1), "1x60": _chain(60, 1), "1x61": _chain(61, 1),
    "2x30": _chain(30, 2), "60+40": _chain(60, 1) + _chain(40, 1),
    "3x50": _chain(50, 3), "61+30+40": _chain(61, 1) + _chain(30, 1) + _chain(40, 1),
    "8x50": _chain(50, 8), "8 mixed": _chain(60, 2) + _chain(40, 3) + _chain(30, 2) + _chain(61, 1),
    "16x40": _chain(40, 16), "16 mixed": _chain(60, 4) + _chain(40, 8) + _chain(50, 4),
    "40x61": _chain(61, 40), "40 mixed": _chain(30, 10) + _chain(61, 10) + _chain(40, 10) + _chain(50, 10),
}
TS = [2, 3, 17, 256, 65537, 2**31 - 1, 2**61 - 1]


def _inputs(Q, delta, rng):
    xs = {0, 1, 2, Q - 1, Q - 2, Q // 2, Q // 2 + 1, Q // 2 - 1}
    for k in [1, 2, 3, Q // delta // 2, Q // delta // 2 + 1, Q // delta - 1, Q // delta] + [rng.randrange(1, Q // delta + 1) for _ in range(6)]:
        for d in (-1, 0, 1):
            for x in (k * delta + d, Q - (k * delta + d)):
                xs.add(x)
        if delta % 2 == 0:                                       # exact ties of the rounding, both signs
            for x in (k * delta + delta // 2, k * delta - delta // 2):
                xs.add(x)
                xs.add(Q - x)
    xs |= {rng.randrange(Q) for _ in range(24)}
    xs |= {rng.randrange(2**20) for _ in range(4)} | {Q - rng.randrange(1, 2**20) for _ in range(4)}
    return sorted(x % Q for x in xs)


def _even_delta_t(Q, t):
    """the smallest t' >= t with an even Δ = Q ÷ t' (and t' < 2^62, t' < Q), or None"""
    for tt in range(t, t + 64):
        if tt < min(Q, 2**62) and (Q // tt) % 2 == 0:
            return tt
    return None


def _check_ring(emul, qs, t, rng):
    Q = 1
    for q in qs:
        Q *= q
    if t >= Q:
        rc, _ = _run(emul, qs, t, 0, _residues([0], qs))
        assert rc == -1, "t >= Q must be rejected"
        return
    delta = Q // t
    xs = _inputs(Q, delta, rng)
    ring = spec.Ring(len(xs), qs, [1] * len(qs))
    poly = spec.poly_from_ints(xs, ring)
    res = _residues(xs, qs)
    rc, got = _run(emul, qs, t, 0, res)
    assert rc == 0
    assert [int(v) for v in got[:, 0]] == spec.bfv_decode(poly, ring, t), (qs, t)
    rc, got = _run(emul, qs, t, 1, res)
    assert rc == 0
    assert [int(v) for v in got[:, 0]] == spec.bgv_decode(poly, ring, t), (qs, t)
    rc, got = _run(emul, qs, t, 2, res)
    assert rc == 0
    for x, row in zip(xs, got):
        assert [int(w) for w in row] == _words(_birem(x, delta)), (qs, t, x)
    ms = [0, 1, t - 1, t, t + 1, 2 * t - 1, 2**64 - 1, 2**63] + [rng.randrange(2**64) for _ in range(8)] + [rng.randrange(t) for _ in range(8)]
    mring = spec.Ring(len(ms), qs, [1] * len(qs))
    rc, got = _run(emul, qs, t, 3, np.array(ms, dtype=np.uint64))
    assert rc == 0
    want = spec.bfv_encode(ms, mring, t)
    assert got.T.tolist() == want, (qs, t)
    rc, got = _run(emul, qs, t, 4, np.array(ms, dtype=np.uint64))
    assert rc == 0
    assert got.T.tolist() == [[(m % t) % q for m in ms] for q in qs], (qs, t)


@pytest.mark.parametrize("name", list(RINGS))
def test_codec_bodies_match_oracle(emul, name):
    qs = RINGS[name]
    rng = random.Random(hash(name) & 0xFFFF)
    Q = 1
    for q in qs:
        Q *= q
    ts = list(TS)
    for t in TS:                                                  # even-Δ companions of the listed t: exact ties
        te = _even_delta_t(Q, t)
        if te is not None:
            ts.append(te)
    for t in ts:
        _check_ring(emul, qs, t, rng)


def test_t_dividing_into_a_ring_modulus_and_powers_of_two(emul):
    """t equal to one of the ring's primes (conv_eval's copy path) and powers of two up to 2^61"""
    rng = random.Random(7)
    qs = _chain(40, 3)
    for t in [qs[1], qs[0], 2**10, 2**32, 2**61]:
        _check_ring(emul, qs, t, rng)
    _check_ring(emul, _chain(61, 2), 2**61, rng)


def test_bound_choice_does_not_change_results(emul):
    """the compile-time limb bound (registers vs rolled loops) is an implementation detail: every bound >= L agrees"""
    rng = np.random.default_rng(3)
    qs = _chain(50, 3)
    res = np.stack([rng.integers(0, q, size=300, dtype=np.uint64) for q in qs], axis=1)
    for op in (0, 1, 2):
        outs = [_run(emul, qs, 65537, op, res, km)[1] for km in (4, 8, 16, 40)]
        for o in outs[1:]:
            assert np.array_equal(o, outs[0])
    assert _run(emul, qs, 65537, 0, res, 2)[0] == -2  # a bound below L is refused


def test_rejects_bad_plaintext_modulus(emul):
    qs = _chain(40, 2)
    res = _residues([5], qs)
    for t in (0, 1, 2**62, 2**63):
        assert _run(emul, qs, t, 0, res)[0] == -1


def test_every_rare_branch_ran(emul):
    """(runs after the oracle comparisons above) the ±1 quotient corrections, the exact ties and the exact-α decision were
    all exercised"""
    if HITS.sum() == 0:
        for name in ("3x50", "8x50", "1x61"):
            test_codec_bodies_match_oracle(emul, name)
    down, up, tie, exact = (int(v) for v in HITS)
    assert down > 0 and up > 0, HITS
    assert tie > 0, HITS
    assert exact > 0, HITS
