"""tfhe_rotate_sum and tfhe_matmul_bsgs_fold through the raw C ABI against tests/rotate_sum_oracle.py (the C oracle's Galois map and key
switch around exact integer sums, on tests/matmul_oracle.py), word for word, at the modulus edges, past 32 limbs, at the group limits
and on every route of the fold: k_md_fold + one inverse transform with a special prime (both lift forms), the coefficient-domain sum
without one.

The input vocabulary is that of tests/test_gpu_matmul_oracle.py, by import: item 0 of a batch is the edge item, item 1 uniform; key r is
all q - 1 for even r and uniform for odd r; the Galois elements are 3^s mod 2N; the bias is q - 1 in every word.  Every case asserts
equality with the oracle, canonical output words, untouched operands, and the same words under a chunk cap of 1."""
import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import helpers as H
from tests import matmul_oracle as MO
from tests import rotate_sum_oracle as RO
from tests.test_gpu_matmul_oracle import _seam_ring, above, dev, galois_elements, make_diags, make_keys, mixed_policy, poison, uniform
from tests.test_gpu_modulus_edges import _ks_ct, edge

pytestmark = pytest.mark.gpu


def _groups(flat, sizes):
    out, off = [], 0
    for s in sizes:
        out.append(list(flat[off:off + s]))
        off += s
    return out


def run_case(qs, logn, special, groups, shape=None, bias=False, batch=2, level=None, variants=(0,), seed=0):
    """groups: the fold's group sizes.  shape None: tfhe_rotate_sum on a ciphertext; else (n_baby, n_giant, n_in): tfhe_matmul_bsgs_fold"""
    N = 1 << logn
    n_baby, n_giant, n_in = shape or (0, 0, 1)
    n_fold = sum(groups)
    Lk = len(qs)
    level = (Lk - 1 if special else Lk) if level is None else level
    cq = qs[:level]
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    assert ctx.psis == ref.psis
    rng = np.random.default_rng(1000 * logn + 10 * Lk + special + seed)
    gs, _ = galois_elements(N, n_baby + n_giant + n_fold, 0)
    keys = make_keys(qs, N, len(gs), rng)
    cts = [_ks_ct(qs, level, 2, N, rng)[:batch] for _ in range(n_in)]
    assert batch in (1, 2) and all(c.shape == (batch, 2, level, N) for c in cts)
    bias_h = np.broadcast_to((np.array(cq, dtype=np.uint64) - 1)[:, None], (level, N)).copy() if bias else None
    dkeys, prep = [dev(k) for k in keys], []
    for k, g in zip(dkeys, gs):
        p = tf.DeviceBuffer(k.n)
        ctx.galois_key_prepare(Lk, Lk, g, k.ptr, p.ptr)
        prep.append(p)
    prep_h = [p.to_numpy() for p in prep]
    ptrs = [p.ptr for p in prep]
    nbg = n_baby + n_giant
    fold_keys, fold_ptrs, fold_gs = _groups(keys[nbg:], groups), _groups(ptrs[nbg:], groups), _groups(gs[nbg:], groups)
    dcts = [dev(c) for c in cts]
    dbias = dev(bias_h) if bias else None
    out = tf.DeviceBuffer(batch * 2 * level * N)
    qv = np.array(cq, dtype=np.uint64).reshape(1, 1, level, 1)
    if shape is None:
        diags, ddiags = [], []
        want = RO.rotate_sum_ref(ref, level, special, fold_keys, fold_gs, cts[0])

        def call():
            ctx.rotate_sum(Lk, level, special, fold_ptrs, fold_gs, Lk, dcts[0].ptr, out.ptr, batch)
    else:
        diags = make_diags(cq, N, n_baby, n_giant, n_in, 7 + seed)
        ddiags = [dev(d) for d in diags]
        product = (ref, level, special, keys[:n_baby], gs[:n_baby], keys[n_baby:nbg], gs[n_baby:nbg], diags, cts)
        want = RO.matmul_bsgs_fold_ref(*product, fold_keys, fold_gs, bias_h)
        if not groups:                                                           # no fold step: the words of tfhe_matmul_bsgs_blocks
            assert np.array_equal(want, MO.matmul_bsgs_blocks_ref(*product, bias_h))

        def call():
            ctx.matmul_bsgs_fold(Lk, level, special, ptrs[:n_baby], gs[:n_baby], ptrs[n_baby:nbg], gs[n_baby:nbg], Lk, [d.ptr for d in ddiags],
                                 [c.ptr for c in dcts], fold_ptrs, fold_gs, dbias.ptr if bias else None, out.ptr, batch)

    def blocks():
        ctx.matmul_bsgs_blocks(Lk, level, special, ptrs[:n_baby], gs[:n_baby], ptrs[n_baby:nbg], gs[n_baby:nbg], Lk, [d.ptr for d in ddiags],
                               [c.ptr for c in dcts], dbias.ptr if bias else None, out.ptr, batch)
    calls = [call] + ([blocks] if shape is not None and not groups else [])
    try:
        for variant in variants:
            ctx.set_ntt_variant(variant)
            for cap in ((0, 1) if batch > 1 else (0,)):
                ctx.set_chunk(cap)
                for f in calls:
                    what = (f.__name__, "variant", variant, "chunk cap", cap)
                    poison(ctx, out)
                    f()
                    got = out.to_numpy((batch, 2, level, N))
                    assert np.array_equal(got, want), what
                    assert (got < qv).all(), what
                    for k, h in zip(dkeys, keys):
                        assert np.array_equal(k.to_numpy(h.shape), h), what
                    for p, h in zip(prep, prep_h):
                        assert np.array_equal(p.to_numpy(), h), what
                    for d, h in zip(dcts + ddiags, cts + list(diags)):
                        assert np.array_equal(d.to_numpy(h.shape), h), what
                    if bias:
                        assert np.array_equal(dbias.to_numpy(bias_h.shape), bias_h), what
    finally:
        ctx.set_chunk(0)
        ctx.set_ntt_variant(0)


def _case(group, ring, logn, groups, special, **kw):
    ident = f"{group}-logn{logn}-{'x'.join(map(str, groups)) or 'none'}-{'special' if special else 'plain'}"
    if "level" in kw:
        ident += f"-level{kw['level']}"
    if "shape" in kw:
        ident += "-product" + "x".join(map(str, kw["shape"]))
    return pytest.param(ring, logn, tuple(groups), special, kw, id=ident)


CASES = []
for sp in (True, False):
    # group shapes: one rotation, a chain of single rotations, several rotations in a step, both mixed
    CASES += [_case("groups", above(40, 3), 8, g, sp) for g in ((1,), (1, 1), (3,), (2, 1), (1, 3, 1))]
    # the admitted maxima: rot_tail_arg_t::g full in one step; 64 steps
    CASES += [_case("limits", above(40, 3), 6, g, sp) for g in ((64,), (1,) * 64)]
    # the modulus edges
    CASES += [_case(n, uniform(n, 3), 10, (3, 1), sp) for n in ("top62", "fold62")]
    CASES += [_case(n, uniform(n, 3), 12, (3, 1), sp) for n in ("fp-top", "u64-bottom")]
    CASES.append(_case("mixed", mixed_policy, 12, (3, 1), sp))
    # k_md_fold's team split: n / per = 0, below nslot, and the clamped lanes
    CASES += [_case("small-rows", above(50, 2), ln, (3, 1), sp) for ln in (4, 8, 11, 13)]
    # n_digits > level, the special-prime table of a lower level, one-limb rows
    CASES += [_case("below-key", uniform("top61", 4), 10, (3, 1), sp, level=lv) for lv in (1, 2)]
    # tfhe_matmul_bsgs_fold: a product feeding one-key steps and a three-key step, with the bias; the smallest product without one;
    # no fold step at all (the words of tfhe_matmul_bsgs_blocks)
    for ring, ln in ((uniform("top62", 3), 10), (above(40, 3), 8)):
        CASES += [_case("product", ring, ln, g, sp, shape=(2, 2, 2), bias=True) for g in ((1, 1), (3,), ())]
        CASES.append(_case("product", ring, ln, (1,), sp, shape=(1, 0, 1)))
# routes that exist only with the special prime.  All targets fp64-size and the special prime not: md_lift_is_fused false, k_md_lift,
# k_md_fold<false>
CASES += [_case("lift-unfused", lambda N, special: edge("fp-top", 3, N) + edge("top62", 1, N), ln, (3, 1), True) for ln in (12, 14)]
# the fused digit-lift mode: k_md_fold<true>
CASES.append(_case("lift-fused", uniform("fp-top", 3), 14, (3, 1), True))
# pair / quad lift and top-stage lift; once more under variant 2, the unfused route at N >= 2^15
for ln in (15, 16):
    for g in ((2,), (1,)):
        CASES.append(_case("large-fp", uniform("fp-top", 2), ln, g, True, batch=1, variants=(0, 2)))
        CASES.append(_case("large-mixed", lambda N, special: edge("fp-top", 1, N) + edge("top62", 2, N), ln, g, True, batch=1, variants=(0, 2)))


@pytest.mark.parametrize("ring,logn,groups,special,kw", CASES)
def test_fold_matches_the_oracle(ring, logn, groups, special, kw):
    run_case(ring(1 << logn, special), logn, special, groups, **kw)


# level > 32: the unfused lift, limb_sel_t past its first mask word; level 32 next to it on the fused side
@pytest.mark.parametrize("name,level,special", [(name, level, sp) for name in ("U40", "W40", "mixed")
                                                for level, sp in ((32, True), (33, True), (33, False), (40, False))])
def test_fold_matches_the_oracle_across_the_32_limb_seam(name, level, special):
    run_case(_seam_ring(name, level + special, 32), 5, special, (2, 1), seed=level)


@pytest.mark.parametrize("special", [True, False])
def test_a_bad_group_is_refused_without_a_launch(special):
    """a group of size 0, 65 keys in all or 65 groups: TFHE_E_BADARG (AssertionError through native.check), no transform launched, the
    output untouched"""
    N, level = 64, 3
    qs = H.primes_above(1 << 40, level + special, N)
    Lk = len(qs)
    ctx = tf.Context(N, qs)
    rng = np.random.default_rng(65)
    key = dev(H.uniform_evk(rng, qs, Lk, N))
    prep = tf.DeviceBuffer(key.n)
    ctx.galois_key_prepare(Lk, Lk, 3, key.ptr, prep.ptr)
    ct = dev(H.rand_residues(rng, qs[:level], (1, 2), N))
    out = tf.DeviceBuffer(2 * level * N)
    poison(ctx, out)
    before = out.to_numpy()
    ctx.prof_enable(True)
    try:
        for sizes, msg in (((1, 0), "below 1"), ((65,), "more than 64"), ((32, 33), "more than 64"), ((1,) * 65, "outside")):
            with pytest.raises(AssertionError, match=msg):
                ctx.rotate_sum(Lk, level, special, [[prep.ptr] * s for s in sizes], [[3] * s for s in sizes], Lk, ct.ptr, out.ptr, 1)
        assert ctx.prof_read()[0] == 0
    finally:
        ctx.prof_enable(False)
    assert np.array_equal(out.to_numpy(), before)
