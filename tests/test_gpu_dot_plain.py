"""tfhe_dot_plain on the device, through the C ABI, against the oracle (tests/dot_plain_oracle.py over oracle/ref_cpu): the fused
kernel at N = 2^12 .. 2^14 under both arithmetic policies and on the two lanes, every operand form (dense elements, components of
packed buffers, shared and batched plaintexts, acc absent / separate / in place, dst inside a packed buffer, limb subsets), the item
walk's wrap, the composed path at every size and setting that takes it, the chunk seams, the overlap and stride checks, and the host
mirror: CipherText.dot_plain through the call against the staging route it replaces, word for word."""
import gc

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import dot_plain_oracle as DO
from tests import helpers as H
from tests import many_limbs as ML
from toyfhe_jl_amd import native

pytestmark = pytest.mark.gpu


def dev(a):
    return tf.DeviceBuffer.from_numpy(a)


def ring(N, bits):
    """one NTT-friendly prime per entry of `bits`, distinct, just above 2^bits"""
    qs = []
    for b in bits:
        qs.append(next(q for q in H.primes_above(1 << b, len(bits) + 1, N) if q not in qs))
    return qs


_CTX = {}


def context(N, qs):
    key = (N, tuple(qs))
    if key not in _CTX:
        ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
        assert ctx.psis == ref.psis
        _CTX[key] = (ctx, ref)
    return _CTX[key]


class View:
    """component p of a packed host array [count][P][limbs][N] (P = 1: a dense element) and its device twin"""

    def __init__(self, host, p):
        self.host, self.p = host, p
        self.count, self.P, self.limbs, self.N = host.shape
        self.buf = dev(host)

    @property
    def arr(self):
        return self.host[:, self.p]

    def at(self, p):
        v = View.__new__(View)
        v.__dict__.update(self.__dict__)
        v.p = p
        return v

    @property
    def ptr(self):
        return self.buf.ptr + self.p * self.limbs * self.N * 8

    @property
    def stride(self):
        return self.P * self.limbs * self.N

    def read(self):
        return self.buf.to_numpy(self.host.shape)


def residues(rng, qs, prefix, N, extreme=False):
    if extreme:
        return np.broadcast_to((np.array(qs, dtype=np.uint64) - 1)[:, None], tuple(prefix) + (len(qs), N)).copy()
    return H.rand_residues(rng, qs, prefix, N)


LAYOUTS = {"dense": (1, 0), "p0of2": (2, 0), "p1of2": (2, 1), "p2of3": (3, 2)}


def run_case(N, qs, count, n_terms, flags, acc_mode, layouts, b_shared, dst_packed=False, idx=None, limbs=None, extreme=False, seed=1,
             variant=0, chunk=0, want=None):
    """one tfhe_dot_plain call against the oracle.  flags: "0", "1" or "mixed"; acc_mode: None, "separate", "inplace"; layouts: the
    operand forms the terms cycle through; returns the result words."""
    ctx, ref = context(N, qs)
    limbs = (len(qs) if idx is None else len(idx)) if limbs is None else limbs
    sel = list(range(limbs)) if idx is None else list(idx)
    sq = [qs[j] for j in sel]
    rng = np.random.default_rng(seed)
    a_ntt = [{"0": 0, "1": 1}.get(flags, (k % 3) == 1) for k in range(n_terms)]
    # a small pool of packed operands per layout; the terms cycle through layouts and pool entries (operands may repeat)
    pool = {}
    for name in set(layouts):
        P, _ = LAYOUTS[name]
        pool[name] = [View(residues(rng, sq, (count, P), N, extreme), 0) for _ in range(2)]
    a = [pool[layouts[k % len(layouts)]][(k // len(layouts)) % 2].at(LAYOUTS[layouts[k % len(layouts)]][1]) for k in range(n_terms)]
    nb = min(n_terms, 3)
    if b_shared:
        bh = [residues(rng, sq, (), N, extreme) for _ in range(nb)]
        b = [(dev(x), 0) for x in bh]
    else:
        bh = [residues(rng, sq, (count,), N, extreme) for _ in range(nb)]
        b = [(dev(x), limbs * N) for x in bh]
    acc_h = None if acc_mode is None else residues(rng, sq, (count,), N, extreme)
    sentinel = np.uint64(0xDEADBEEFCAFEF00D)
    dst_h = np.full((count, 2 if dst_packed else 1, limbs, N), sentinel, dtype=np.uint64)
    if acc_mode == "inplace":
        dst_h[:, -1] = acc_h
    dst = View(dst_h, dst_h.shape[1] - 1)
    acc_buf = dev(acc_h) if acc_mode == "separate" else None
    acc = None if acc_mode is None else ((dst.ptr, dst.stride) if acc_mode == "inplace" else (acc_buf.ptr, limbs * N))
    ctx.set_ntt_variant(variant)
    ctx.set_chunk(chunk)
    try:
        ctx.dot_plain(acc, [(v.ptr, v.stride, f) for v, f in zip(a, a_ntt)], [(b[k % nb][0].ptr, b[k % nb][1]) for k in range(n_terms)],
                      (dst.ptr, dst.stride), count, limbs, idx)
        got = dst.read()
    finally:
        ctx.set_ntt_variant(0)
        ctx.set_chunk(0)
    if want is None:
        want = DO.dot_plain_ref(ref, acc_h, [v.arr for v in a], a_ntt, [bh[k % nb] for k in range(n_terms)], sel)
    assert np.array_equal(got[:, -1], want), (N, count, n_terms, flags, acc_mode, layouts, b_shared, idx, variant, chunk)
    assert int((got[:, -1] >= np.array(sq, dtype=np.uint64)[None, :, None]).sum()) == 0
    if dst_packed:
        assert (got[:, 0] == sentinel).all(), "the other component of the packed destination is untouched"
    for v in a:                                      # operands are read only
        assert np.array_equal(v.read(), v.host)
    return got[:, -1]


# ---- the fused sizes ---------------------------------------------------------------------------------------------------------------

R1, R2, R3, R4, R5 = (12, (50, 50, 50), 2), (12, (60, 60), 2), (12, (60, 40, 60), 3), (13, (60, 40), 2), (14, (60, 50), 2)
MIX = ("dense", "p0of2", "p1of2", "p2of3")
FUSED = [
    # ring, n_terms, flags, acc, layouts, b shared, dst packed
    (R1, 1, "0", None, ("dense",), True, False),
    (R1, 2, "1", "separate", ("p0of2", "p1of2"), False, True),
    (R1, 7, "mixed", "inplace", ("p2of3",), True, False),
    (R1, 65, "mixed", None, MIX, False, False),
    (R2, 64, "0", "separate", ("dense",), True, False),
    (R2, 7, "mixed", "inplace", MIX, False, True),
    (R2, 2, "0", None, ("p1of2",), False, False),
    (R3, 7, "mixed", "separate", MIX, True, True),
    (R3, 65, "0", None, ("dense", "p2of3"), False, False),
    (R3, 1, "1", "inplace", ("p0of2",), True, False),
    (R4, 2, "0", None, ("dense",), False, False),
    (R4, 7, "mixed", "inplace", MIX, True, True),
    (R4, 64, "1", "separate", ("p1of2",), False, False),
    (R5, 1, "0", "separate", ("p2of3",), True, False),
    (R5, 7, "mixed", None, MIX, False, True),
    (R5, 64, "0", "inplace", ("dense",), True, False),
]


@pytest.mark.parametrize("rg,n_terms,flags,acc,layouts,shared,packed", FUSED)
def test_fused_sizes_match_the_oracle(rg, n_terms, flags, acc, layouts, shared, packed):
    logn, bits, count = rg
    N = 1 << logn
    run_case(N, ring(N, bits), count, n_terms, flags, acc, layouts, shared, packed, seed=n_terms + logn)


@pytest.mark.parametrize("bits", [(50, 50, 50), (60, 60)])       # the fp64 policy, the u64 policy
def test_every_word_at_q_minus_1_over_64_terms(bits):
    N = 1 << 12
    run_case(N, ring(N, bits), 2, 64, "mixed", "separate", ("dense", "p1of2"), False, extreme=True)


def test_limb_subsets():
    """a non-prefix limb_idx subset (in an order of its own, both policies) and a level below the ring's"""
    N = 1 << 12
    qs = ring(N, (60, 40, 60))
    run_case(N, qs, 2, 7, "mixed", "separate", MIX, True, True, idx=[2, 1])
    run_case(N, qs, 2, 3, "0", None, ("p1of2",), False, idx=[1])
    run_case(N, ring(N, (50, 50, 50)), 2, 7, "mixed", "inplace", MIX, False, limbs=2)


def test_item_walk_wraps():
    """more (item, limb) rows than persistent workgroups: N = 2^12, (50, 60), count 1400, 2 terms.  The operands are seven distinct items
    repeated, the accumulator is distinct in every item: the expected words are the oracle's seven sums plus the accumulator (exact in
    64 bits: both below 2^61)."""
    N, count, per = 1 << 12, 1400, 7
    qs = ring(N, (50, 60))
    ctx, ref = context(N, qs)
    rng = np.random.default_rng(5)
    a7 = [H.rand_residues(rng, qs, (per,), N) for _ in range(2)]
    b7 = H.rand_residues(rng, qs, (per,), N)
    sums = DO.dot_plain_ref(ref, None, a7, [0, 1], [b7, b7])
    acc = H.rand_residues(rng, qs, (count,), N)
    q = np.array(qs, dtype=np.uint64)[None, :, None]
    want = (acc + np.tile(sums, (count // per, 1, 1))) % q
    da = [dev(np.tile(x, (count // per, 1, 1))) for x in a7]
    db, dacc, dst = dev(np.tile(b7, (count // per, 1, 1))), dev(acc), tf.DeviceBuffer(count * 2 * N)
    row = 2 * N
    ctx.dot_plain((dacc.ptr, row), [(da[0].ptr, row, 0), (da[1].ptr, row, 1)], [(db.ptr, row)] * 2, (dst.ptr, row), count, 2)
    assert np.array_equal(dst.to_numpy((count, 2, N)), want)


# ---- the composed path ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("logn,bits,count,n_terms", [(11, (40, 60), 3, 7), (15, (50, 60), 2, 3), (16, (60, 40), 1, 2)])
def test_composed_sizes_match_the_oracle(logn, bits, count, n_terms):
    N = 1 << logn
    run_case(N, ring(N, bits), count, n_terms, "mixed", "separate", MIX, False, True, seed=logn)
    run_case(N, ring(N, bits), count, n_terms, "0", None, ("p1of2", "dense"), True, seed=logn + 1)


def test_composed_variant_1_and_33_limbs():
    N = 1 << 12
    run_case(N, ring(N, (50, 60)), 2, 7, "mixed", "inplace", MIX, True, variant=1)
    run_case(N, ML.mixed(33, N), 1, 3, "mixed", "separate", ("dense", "p1of2"), False)
    run_case(N, ML.mixed(33, N), 2, 2, "1", None, ("p0of2",), True)      # nothing to transform: no workspace


@pytest.mark.parametrize("logn", [12, 11])                      # fused, composed
def test_chunk_seams_leave_the_words_unchanged(logn):
    """tfhe_ctx_set_chunk 1 and 3 against the uncapped call: 5 items and a 65-term sum, both cut unevenly by 3"""
    N = 1 << logn
    qs = ring(N, (50, 60))
    args = (N, qs, 5, 65, "mixed", "separate", MIX, False, True)
    want = run_case(*args, seed=9)
    for chunk in (1, 3):
        got = run_case(*args, seed=9, chunk=chunk, want=want)
        assert np.array_equal(got, want)


# ---- checks that need the ring ---------------------------------------------------------------------------------------------------------

def test_overlap_and_stride_checks_leave_the_buffers_untouched():
    N, count = 1 << 12, 2
    qs = ring(N, (50, 60))
    ctx, _ = context(N, qs)
    row = 2 * N
    rng = np.random.default_rng(3)
    ah, bh = H.rand_residues(rng, qs, (count, 2), N), H.rand_residues(rng, qs, (count,), N)
    a, b, d = dev(ah), dev(bh), dev(np.zeros((count, 2, N), dtype=np.uint64))
    good_a, good_b = [(a.ptr, 2 * row, 0)], [(b.ptr, row)]

    def bad(acc, av, bv, dst, word):
        with pytest.raises(AssertionError) as e:                        # TFHE_E_BADARG
            ctx.dot_plain(acc, av, bv, dst, count, 2)
        assert word in str(e.value), str(e.value)
    # dst inside the strided range of a[k] (the other component of the same packed buffer), of b[k], at an odd offset
    bad(None, good_a, good_b, (a.ptr + row * 8, 2 * row), "overlaps operand 0")
    bad(None, good_a, good_b, (b.ptr + N * 8, row), "overlaps operand 0")
    bad(None, good_a + [(a.ptr + row * 8, 2 * row, 1)], good_b * 2, (a.ptr + (2 * row + 8) * 8, row), "overlaps operand")
    # acc overlapping dst other than as the same view
    bad((d.ptr + 8 * 8, row), good_a, good_b, (d.ptr, row), "overlaps acc")
    bad((d.ptr, 2 * row), good_a, good_b, (d.ptr, row), "overlaps acc")
    # strides below limbs * N; a b stride of 0 is the shared plaintext
    bad(None, [(a.ptr, row - 1, 0)], good_b, (d.ptr, row), "stride")
    bad(None, good_a, [(b.ptr, row - 1)], (d.ptr, row), "stride")
    bad(None, good_a, good_b, (d.ptr, row - 1), "stride")
    bad((b.ptr, 1), good_a, good_b, (d.ptr, row), "stride")
    assert np.array_equal(a.to_numpy(ah.shape), ah) and np.array_equal(b.to_numpy(bh.shape), bh) and not d.to_numpy().any()
    # count * limbs must fit the row kernels' item counter (checked before anything is read: the buffers hold two items)
    with pytest.raises(AssertionError) as e:
        ctx.dot_plain(None, good_a, good_b, (d.ptr, row), 2**30, 2)
    assert "polynomial count" in str(e.value)
    # limbs / limb_idx as make_sel reports them
    with pytest.raises(AssertionError):
        ctx.dot_plain(None, good_a, good_b, (d.ptr, row), count, 0)
    with pytest.raises(native.UsageError) as e:                         # TFHE_E_LEVEL_MISMATCH
        ctx.dot_plain(None, good_a, good_b, (d.ptr, row), count, 2, [0, 2])
    assert "limb_idx" in str(e.value)
    ctx.dot_plain(None, good_a, good_b, (d.ptr, row), 0, 2)              # count == 0: nothing happens
    assert not d.to_numpy().any()


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("logn", [12, 11])                      # fused (with a special prime), composed
def test_mirror_dot_plain_through_the_call_equals_the_staging_route(monkeypatch, logn):
    """CipherText.dot_plain with the call (default) against TFHE_DOT_PLAIN_CALL=0, word for word: split ciphertexts, unsplit results of
    chained rotations, a mix; unsplit operands stay unsplit; equal to sum(c.mul_plain(p)); the call route leaves no staging buffer."""
    N = 1 << logn
    R = tf.NegacyclicRing(N, H.chain(40, 4, N))
    params = tf.ModulusRaised(tf.CKKSParams(R, 0, 3.2))
    rng = np.random.default_rng(21)
    kp = tf.keygen(rng, params)
    gk = tf.keygen_galois(rng, kp.priv, steps=1)
    B, K = 3, 5
    vals = np.repeat((np.arange(1, N // 2 + 1) / N).astype(complex)[None], B, axis=0)
    c = tf.encrypt(rng, kp, tf.ckks_encode(vals, params.R_cipher(), 2**40), scale=2**40)
    pts = [tf.ckks_encode(np.repeat(np.cos(np.arange(N // 2) * (k + 1) / 40.0).astype(complex)[None], B, axis=0), params.R_cipher(), 2**40)
           for k in range(K)]
    rots = [c]
    for _ in range(K - 1):
        rots.append(tf.rotate(gk, rots[-1]))
    split = [tf.CipherText(params, [tf.RingElement.from_residues(params.R_cipher(), x.to_numpy()) for x in tf.rotate(gk, r).cs], c.scale) for r in rots]
    assert all(isinstance(r, tf.she._PackedResult) and r._cs is None for r in rots[1:])
    mix = [rots[0], split[1], rots[2], split[3], rots[4]]
    mix[1].cs[0].coeffs_dual()                                   # one cached transform in between
    ctx = params.R_cipher().ctx
    tf.she.release_staging(ctx)
    for p_ in pts:
        p_.coeffs_dual()                                         # the plaintexts' transforms exist before anything is counted
    result_bytes = 2 * B * params.R_cipher().L * N * 8
    out = {}
    for call in (True, False):
        monkeypatch.setattr(tf.she, "_DOT_PLAIN_CALL", call)
        res = []
        for cts in (split, rots, mix):
            r = None                                             # (the previous result goes before anything is counted)
            gc.collect()
            live = native.alloc_stats()["live_bytes"]
            r = tf.CipherText.dot_plain(cts, pts)
            if call:
                assert getattr(ctx, "_ntt_stage", None) is None, "the call route stages nothing"
                # (the allocator may hand out a recycled block of up to twice the size asked for; a staging pair for five operands
                # would be ten components on top of the result's two)
                grown = native.alloc_stats()["live_bytes"] - live
                assert 0 < grown <= 2 * result_bytes, "only the result is left live"
            res.append([x.to_numpy("dual") for x in r.cs])
        assert all(r._cs is None for r in rots[1:]), "unsplit operands are still unsplit"
        out[call] = res
    for g, w in zip(out[True], out[False]):
        assert len(g) == len(w) == 2 and all(np.array_equal(x, y) for x, y in zip(g, w))
    want = None
    for ct, p in zip(mix, pts):
        t = ct.mul_plain(p)
        want = t if want is None else want + t
    for g, w in zip(out[True][2], want.cs):
        assert np.array_equal(g, w.to_numpy("dual"))
