"""Every entry point of the C ABI at 17 to 40 limbs, on both sides of the 32-limb routing-mask seam.

The per-limb routing masks of the host dispatch are 32 bits wide (toyfhe_hip.hip mask_all / mask_of): selections of 33 or
more limbs are never split by arithmetic policy, lose the two-lane key switch, the fused mul_relin / encrypt kernels and the
fused lift of matmul_diag, and the plain codec and BFV plans leave their unrolled / table-driven forms well before that.  The
kernels read mask 0 as "every limb", the host above 32 limbs uses 0 as "not every limb": a wrong turn at the seam drops limbs
without any error.  Every comparison is bit for bit against oracle/ref_cpu (pinned at these widths to the big-integer spec
by tests/test_many_limbs_cpu.py) or oracle/spec on seeded inputs; the CKKS codec reuses test_gpu_parity's rule."""
import random

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu, spec
from tests import enc_oracle as EO
from tests import helpers as H
from tests import many_limbs as ML
from tests import test_gpu_mul_relin as MR
from tests import test_gpu_parity as P
from tests.test_plain_codec_cpu import _inputs as codec_edge_inputs

pytestmark = pytest.mark.gpu


def compute_units():
    """the device's compute units, as tfhe_ctx_create reads them: launch.h cu_grid(items, per_cu) = min(items, per_cu * CUs)"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def dev(a):
    return tf.DeviceBuffer.from_numpy(a)


def fill(rng, qs, prefix, N):
    """uniform residues [*prefix][len(qs)][N] (H.rand_residues without the stacking copy: the 2^16 keys are 1 GiB)"""
    prefix = tuple(prefix)
    out = np.empty(prefix + (len(qs), N), dtype=np.uint64)
    for l, q in enumerate(qs):
        out[..., l, :] = rng.integers(0, int(q), size=prefix + (N,), dtype=np.uint64)
    return out


def centring_edges(ct, qs):
    """0, 1, q - 1, q / 2, q / 2 + 1 on every limb of the last component of the first ciphertext"""
    for l, q in enumerate(qs):
        ct[0, -1, l, :5] = [0, 1, q - 1, q // 2, q // 2 + 1]
    return ct


def galois_ref(ref, g, ct):
    level, N = ct.shape[-2], ct.shape[-1]
    return ref.galois(g, ct.reshape(-1, level, N), idx=range(level)).reshape(ct.shape)


# ---------------------------------------------------------------------------------------------------
# 1. transforms
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [5, 10, 12, 14, 15, 16, 17])
@pytest.mark.parametrize("name", ["U40", "W40", "N34", "M34", "M33e"])
def test_transforms_on_33_to_40_limbs(name, logn):
    """nntt / inntt / round trip, in place and out of place (N = 2^16: the one-kernel paths), on all limbs, on 33 limbs in an
    order that is neither ascending nor descending, and on the prefixes of 31, 32 and 33 limbs.  The mixed rings carry enough
    rows for the two-policy split ((rows << logN) >= 2^20 already at 31 limbs): the 31- and 32-limb prefixes split, 33 limbs
    and more must not.  Two things keep them off: mask_of collapses a mixed selection's policy masks to 0 above 32 limbs (so
    mixed_fp() is false) and run_ntt asks for `sel.n <= 32`; moving the second alone changes nothing.  What these cases do
    catch is a non-zero mask reaching the kernels with more than 32 limbs (dense_count / dense_item then drop limbs)."""
    N = 1 << logn
    qs = ML.ring(name, N)
    L = len(qs)
    mixed = name in ("M34", "M33e")
    count = max(2 if logn <= 14 else 1, -(-H.MIXED_MIN_WORDS // (31 * N))) if mixed and logn >= 10 else (2 if logn <= 14 else 1)
    rng = np.random.default_rng(logn * 41 + L)
    a = fill(rng, qs, (count,), N)
    a[0, :, 0] = np.array(qs, dtype=np.uint64) - 1
    ref, ctx = ref_cpu.RefCtx(N, qs), tf.Context(N, qs)
    assert ctx.psis == ref.psis
    want = ref.nntt(a)                                         # per limb: every selection below is a slice of it
    assert np.array_equal(P.run_ntt(ctx, a), want)             # in place, all limbs
    assert np.array_equal(P.run_ntt(ctx, want, inverse=True), a)
    d_in, d_out = dev(a), tf.DeviceBuffer(a.size)              # out of place
    ctx.nntt(d_in.ptr, d_out.ptr, count, L)
    assert np.array_equal(d_out.to_numpy(a.shape), want)
    assert np.array_equal(d_in.to_numpy(a.shape), a)           # source untouched
    ctx.inntt(d_out.ptr, d_in.ptr, count, L)
    assert np.array_equal(d_in.to_numpy(a.shape), a)
    sels = [ML.shuffled(L, 33, logn)] + [list(range(k)) for k in (31, 32, 33)]
    for idx in sels:
        sub, wsub = np.ascontiguousarray(a[:, idx]), np.ascontiguousarray(want[:, idx])
        assert np.array_equal(P.run_ntt(ctx, sub, idx=idx), wsub), idx
        s_in, s_out = dev(wsub), tf.DeviceBuffer(sub.size)
        ctx.inntt(s_in.ptr, s_out.ptr, count, len(idx), idx)
        assert np.array_equal(s_out.to_numpy(sub.shape), sub), idx
        ctx.nntt(s_out.ptr, s_in.ptr, count, len(idx), idx)    # ... and back, out of place
        assert np.array_equal(s_in.to_numpy(sub.shape), wsub), idx


# ---------------------------------------------------------------------------------------------------
# 2. limb-wise operations
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [5, 12])
@pytest.mark.parametrize("name", ["M34", "W40"])
def test_limbwise_ops_on_34_and_40_limbs(name, logn):
    """N = 2^12 with count * limbs >= 128 rows: the LDS-scatter automorphism (rows >= num_cus / 2); N = 2^5: the plain kernels"""
    N = 1 << logn
    qs = ML.ring(name, N)
    L, count = len(qs), (4 if logn == 12 else 3)
    assert logn != 12 or count * L >= compute_units() // 2
    ref, ctx = ref_cpu.RefCtx(N, qs), tf.Context(N, qs)
    rng = np.random.default_rng(N + L)
    a, b, c = (fill(rng, qs, (count,), N) for _ in range(3))
    qm1 = np.array(qs, dtype=np.uint64) - 1
    a[0, :, :2] = 0; b[0, :, 0] = qm1; a[1, :, 0] = qm1; b[1, :, 0] = qm1
    da, db, dc, do = dev(a), dev(b), dev(c), tf.DeviceBuffer(a.size)
    mul = lambda u, v: ref.pointwise("mul", u, v)
    add = lambda u, v: ref.pointwise("add", u, v)
    for op in ("add", "sub", "mul"):
        getattr(ctx, op)(da.ptr, db.ptr, do.ptr, count, L)
        assert np.array_equal(do.to_numpy(a.shape), ref.pointwise(op, a, b)), op
    ctx.neg(da.ptr, do.ptr, count, L)
    assert np.array_equal(do.to_numpy(a.shape), ref.pointwise("neg", a))
    ctx.mad(dc.ptr, da.ptr, db.ptr, do.ptr, count, L)
    assert np.array_equal(do.to_numpy(a.shape), add(c, mul(a, b)))
    s = 0x1234567890ABCDEF1234567890ABCDEF
    sc = [[(s >> k) % q for q in qs] for k in range(3)]
    ctx.scalar_mul(sc[0], da.ptr, do.ptr, count, L)
    assert np.array_equal(do.to_numpy(a.shape), ref.scalar_mul(sc[0], a))
    ctx.dot(None, [da.ptr, db.ptr, dc.ptr], [db.ptr, dc.ptr, da.ptr], do.ptr, count, L)          # 3 terms
    assert np.array_equal(do.to_numpy(a.shape), add(add(mul(a, b), mul(b, c)), mul(c, a)))
    ctx.dot(dc.ptr, [da.ptr, db.ptr, dc.ptr], [db.ptr, dc.ptr, da.ptr], do.ptr, count, L)
    assert np.array_equal(do.to_numpy(a.shape), add(c, add(add(mul(a, b), mul(b, c)), mul(c, a))))
    ctx.lincomb(sc, [da.ptr, db.ptr, dc.ptr], do.ptr, count, L)
    assert np.array_equal(do.to_numpy(a.shape), add(add(ref.scalar_mul(sc[0], a), ref.scalar_mul(sc[1], b)), ref.scalar_mul(sc[2], c)))
    # tensor (rlwe_she.jl:255-258) of two 2-component operands
    x, y = fill(rng, qs, (2, 2), N), fill(rng, qs, (2, 2), N)
    dx, dy, dt = dev(x), dev(y), tf.DeviceBuffer(2 * 3 * L * N)
    ctx.tensor(dx.ptr, dy.ptr, dt.ptr, 2, L)
    got = dt.to_numpy((2, 3, L, N))
    assert np.array_equal(got[:, 0], mul(x[:, 0], y[:, 0]))
    assert np.array_equal(got[:, 1], add(mul(x[:, 0], y[:, 1]), mul(x[:, 1], y[:, 0])))
    assert np.array_equal(got[:, 2], mul(x[:, 1], y[:, 1]))
    # rescale by the last limb, and by the last limb of 33 limbs in another order
    dr = tf.DeviceBuffer(count * (L - 1) * N)
    ctx.rescale(da.ptr, dr.ptr, count, L)
    assert np.array_equal(dr.to_numpy((count, L - 1, N)), ref.modswitch(a))
    idx = ML.shuffled(L, 33, N)
    sub = np.ascontiguousarray(a[:, idx])
    ctx.rescale(dev(sub).ptr, dr.ptr, count, 33, idx)
    assert np.array_equal(dr.to_numpy((count * (L - 1), N))[: count * 32].reshape(count, 32, N), ref.modswitch(sub, idx))
    rev = list(range(L))[::-1]                                 # select_limbs: all of them, reversed
    ctx.select_limbs(da.ptr, do.ptr, count, L, rev)
    assert np.array_equal(do.to_numpy(a.shape), a[:, rev])
    for g in (3, 2 * N - 1, pow(3, N // 4 + 1, 2 * N)):
        ctx.galois(da.ptr, do.ptr, g, count, L)
        assert np.array_equal(do.to_numpy(a.shape), ref.galois(g, a)), g
    ctx.galois(dev(sub).ptr, do.ptr, 5, count, 33, idx)
    assert np.array_equal(do.to_numpy((count * L, N))[: count * 33].reshape(sub.shape), ref.galois(5, sub, idx))


# ---------------------------------------------------------------------------------------------------
# 3. key switch and rotations
# ---------------------------------------------------------------------------------------------------
def ks_setup(N, qs, level, seed):
    rng = np.random.default_rng(seed)
    ref, ctx = ref_cpu.RefCtx(N, qs), tf.Context(N, qs)
    evk = fill(rng, qs, (level, 2), N)
    return rng, ref, ctx, evk, dev(evk)


@pytest.mark.parametrize("logn", [5, 10])
@pytest.mark.parametrize("name,level,special", [("U40", 39, True), ("U40", 40, False), ("W40", 40, False), ("W40", 39, True),
                                                ("M34", 33, True), ("M34", 34, False)])
def test_keyswitch_and_rotations_small_degrees(name, level, special, logn):
    """nw = 40 with the special prime in the last idx slot, level 40 plain, 34 mixed working limbs; 2 and 3 components;
    tfhe_rotate, tfhe_rotate_prepared and tfhe_rotate_many under three Galois elements, each against the oracle"""
    N, batch = 1 << logn, 3
    qs = ML.ring(name, N)
    Lk = len(qs)
    rng, ref, ctx, evk, devk = ks_setup(N, qs, level, logn + level + special)
    for polys in (2, 3):
        ct = centring_edges(fill(rng, qs[:level], (batch, polys), N), qs[:level])
        dct, dout = dev(ct), tf.DeviceBuffer(batch * 2 * level * N)
        ctx.keyswitch(Lk, level, special, devk.ptr, level, dct.ptr, polys, dout.ptr, batch)
        assert np.array_equal(dout.to_numpy((batch, 2, level, N)), ref.keyswitch(level, special, evk, ct)), polys
    check_rotations(ctx, ref, qs, Lk, level, special, N, batch, rng, [evk, fill(rng, qs, (level, 2), N), fill(rng, qs, (level, 2), N)],
                    picks=range(batch))


def check_rotations(ctx, ref, qs, Lk, level, special, N, batch, rng, evks, picks):
    """rotate, rotate_prepared and rotate_many under three Galois elements: rotate_many equals the one-by-one rotations, and
    those equal the oracle's keyswitch o apply_galois_element on ciphertext picks[r % len(picks)] .. (all of `picks` when the
    list is a range)"""
    gs = [pow(3, 5, 2 * N), 2 * N - 1, pow(3, N // 2 + 3, 2 * N)]
    devks = {id(e): dev(e) for e in evks}
    ptrs = [devks[id(e)].ptr for e in evks]
    ct = centring_edges(fill(rng, qs[:level], (batch, 2), N), qs[:level])
    dct = dev(ct)
    many = tf.DeviceBuffer(3 * batch * 2 * level * N)
    ctx.rotate_many(Lk, level, special, ptrs, level, gs, dct.ptr, many.ptr, batch)
    got = many.to_numpy((3, batch, 2, level, N))
    one, prep_out = tf.DeviceBuffer(batch * 2 * level * N), tf.DeviceBuffer(batch * 2 * level * N)
    prep = tf.DeviceBuffer(evks[0].size)
    for r, g in enumerate(gs):
        ctx.rotate(Lk, level, special, ptrs[r], level, g, dct.ptr, one.ptr, batch)
        assert np.array_equal(one.to_numpy(got[r].shape), got[r]), ("rotate_many", g)
        ctx.galois_key_prepare(Lk, level, g, ptrs[r], prep.ptr)
        ctx.rotate(Lk, level, special, prep.ptr, level, g, dct.ptr, prep_out.ptr, batch, prepared=True)
        assert np.array_equal(prep_out.to_numpy(got[r].shape), got[r]), ("rotate_prepared", g)
    pick = [list(picks) if isinstance(picks, range) else [picks[r % len(picks)]] for r in range(3)]
    rot = [galois_ref(ref, g, ct[pick[r]]) for r, g in enumerate(gs)]
    if all(e is evks[0] for e in evks):                       # one key: the three oracle key switches as one batch
        want = np.split(ref.keyswitch(level, special, evks[0], np.concatenate(rot)), np.cumsum([len(x) for x in pick])[:-1])
    else:
        want = [ref.keyswitch(level, special, evks[r], rot[r]) for r in range(3)]
    for r, g in enumerate(gs):
        assert np.array_equal(got[r][pick[r]], want[r]), ("oracle", g)


@pytest.mark.parametrize("special", [True, False])
@pytest.mark.parametrize("logn", [13, 14])
def test_fused_keyswitch_with_34_working_limbs_wraps_the_grid(logn, special):
    """k_ks_fused at nw = 34: level 33 + special prime (two launches, batch and batch * 33 items) and level 34 plain
    (batch * 34 items) on one (2^14) / two (2^13) workgroups per compute unit, so every workgroup of the larger launch walks more than one item.
    First and last ciphertext against the oracle, all of them against the same call on the batch permuted; rotations at 2^14
    (with the special prime: finished in the second launch's stores)."""
    N = 1 << logn
    qs = H.chain(40, 34, N)
    Lk, level = 34, 33 if special else 34
    wgs = compute_units() * (2 if logn == 13 else 1)
    batch = wgs // level + 1
    assert batch * level > wgs and batch >= 2
    rng, ref, ctx, evk, devk = ks_setup(N, qs, level, logn * 2 + special)
    ct = centring_edges(fill(rng, qs[:level], (batch, 3), N), qs[:level])
    dct, dout = dev(ct), tf.DeviceBuffer(batch * 2 * level * N)
    ctx.keyswitch(Lk, level, special, devk.ptr, level, dct.ptr, 3, dout.ptr, batch)
    got = dout.to_numpy((batch, 2, level, N))
    pick = [0, batch - 1]
    assert np.array_equal(got[pick], ref.keyswitch(level, special, evk, ct[pick]))
    perm = rng.permutation(batch)
    ctx.keyswitch(Lk, level, special, devk.ptr, level, dev(ct[perm]).ptr, 3, dout.ptr, batch)
    assert np.array_equal(dout.to_numpy(got.shape), got[perm])
    if logn == 14:
        check_rotations(ctx, ref, qs, Lk, level, special, N, batch, rng, [evk, evk, evk], picks=[0, batch - 1, batch // 2])


@pytest.mark.parametrize("nw", [32, 33])
@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("logn", [15, 16])
def test_keyswitch_sub_block_paths_on_both_sides_of_the_seam(logn, kind, nw):
    """N = 2^15 / 2^16 with the special prime at nw = 32 and 33 working limbs.  Uniform 40-bit ring: k_ks_fused_sub (X = 1 / 2,
    ArithFpS).  Mixed ring (60-bit q0 and special prime around 40-bit primes): at nw = 32 the last shape that takes lift_mixed,
    the two lanes and the tail16 form's masked walk, at nw = 33 the first that must stay on the unmasked u64 kernels.  One
    ciphertext (at 2^16 and nw = 33 the digit rows alone are 0.55 GB); 2 and 3 components at 2^15."""
    N, level = 1 << logn, nw - 1
    qs = H.chain(40, nw, N) if kind == "uniform" else ML.mixed(nw, N)
    rng, ref, ctx, evk, devk = ks_setup(N, qs, level, logn * 100 + nw)
    for polys in ((2, 3) if logn == 15 else (3,)):
        ct = centring_edges(fill(rng, qs[:level], (1, polys), N), qs[:level])
        dct, dout = dev(ct), tf.DeviceBuffer(2 * level * N)
        ctx.keyswitch(nw, level, True, devk.ptr, level, dct.ptr, polys, dout.ptr, 1)
        assert np.array_equal(dout.to_numpy((1, 2, level, N)), ref.keyswitch(level, True, evk, ct)), polys


@pytest.mark.parametrize("kind,nw,batch", [("uniform", 33, 8), ("mixed", 32, 1), ("mixed", 33, 1)])
def test_rotations_at_2_16_on_both_sides_of_the_seam(kind, nw, batch):
    """rotate / rotate_prepared / rotate_many at N = 2^16 under three Galois elements (one key: 1 GiB each): on the uniform ring
    with 8 ciphertexts tfhe_rotate finishes the rotation in the tail (k_ks_top_tail_rot) while rotate_many takes the hoisted
    path; every element against the oracle on one ciphertext"""
    N, level = 1 << 16, nw - 1
    qs = H.chain(40, nw, N) if kind == "uniform" else ML.mixed(nw, N)
    rng, ref, ctx, evk, devk = ks_setup(N, qs, level, 1600 + nw)
    check_rotations(ctx, ref, qs, nw, level, True, N, batch, rng, [evk, evk, evk], picks=[0, batch - 1, batch // 2])


@pytest.mark.parametrize("logn", [12, 16])
def test_matmul_diag_at_level_33_takes_the_unfused_lift(logn):
    """tfhe_matmul_diag with 2 diagonals at level 33 + special prime (md_lift_is_fused: level > 32 -> k_md_lift and plain
    transforms) against rotate + mul_plain + add through the same keys, word for word"""
    N = 1 << logn
    R = tf.NegacyclicRing(N, H.chain(40, 34, N))
    params = tf.ModulusRaised(tf.CKKSParams(R, 0, 3.2))
    assert params.R_cipher().L == 33
    rng = tf.DeviceRng(3300 + logn)
    kp = tf.keygen(rng, params)
    scale = 2**30
    nrng = np.random.default_rng(logn)
    batch = 2 if logn == 12 else None
    x = nrng.normal(0, 1, (N // 2,) if batch is None else (batch, N // 2)).astype(complex)
    c = tf.encrypt(rng, kp, tf.ckks_encode(x, params.R_cipher(), scale), scale=scale)
    gks = [tf.keygen_galois(rng, kp.priv, steps=1)]
    dv = nrng.normal(0, 1, (2, N // 2)).astype(complex)
    singles = [tf.ckks_encode(dv[k], params.R_cipher(), scale) for k in range(2)]
    bcast = [d if batch is None else d.broadcast_to(batch) for d in singles]
    want = c.mul_plain(bcast[0]) + tf.rotate(gks[0], c).mul_plain(bcast[1])
    got = tf.matmul_diag(gks, singles, c)
    assert got.scale == want.scale and len(got) == 2
    for a, b in zip(got.cs, want.cs):
        assert np.array_equal(a.to_numpy("dual"), b.to_numpy("dual"))
    dec = tf.ckks_decode(tf.decrypt(kp, got), got.scale)
    assert np.abs(dec - (dv[0] * x + dv[1] * np.roll(x, 1, axis=-1))).max() < 5e-2   # the bound of test_gpu_reference_mirrors at this scale


@pytest.mark.parametrize("special", [False, True])
def test_keyswitch_window_on_a_34_limb_key(special):
    """K14 with w = 16 at N = 2^6 on a 34-limb key ring: the exact reconstruction (conv_tab_t, window_digits_coeff) runs at 34
    words (33 under the special prime).  Digits from Python big integers (spec.window_digits), sums through the oracle."""
    N, w, Lk = 64, 16, 34
    qs = H.chain(40, Lk, N)
    level = Lk - 1 if special else Lk
    keyring, cring = spec.Ring(N, qs), spec.Ring(N, qs[:level])
    which = list(range(level)) + ([Lk - 1] if special else [])
    wring = keyring.select(which)
    ref, ctx = ref_cpu.RefCtx(N, qs), tf.Context(N, qs)
    nkey = spec.ndigits((cring.Q * qs[-1]) if special else cring.Q, 2 ** w)
    need = spec.ndigits(cring.Q, 2 ** w)
    rng = np.random.default_rng(34 + special)
    evk = fill(rng, qs, (nkey, 2), N)                                       # NTT domain
    devk = dev(evk)
    batch = 2
    for polys in (2, 3):
        ct = fill(rng, qs[:level], (batch, polys), N)
        ct[0, polys - 1, :, 0] = 0
        ct[0, polys - 1, :, 1] = [q - 1 for q in qs[:level]]
        ct[0, polys - 1, :, 2] = 1
        ct[0, polys - 1, :, 3] = [(cring.Q // 2) % q for q in qs[:level]]
        dct, dout = dev(ct), tf.DeviceBuffer(batch * 2 * level * N)
        ctx.keyswitch_window(level, w, devk.ptr, nkey, dct.ptr, polys, dout.ptr, batch, key_limbs=Lk, special=special)
        got = dout.to_numpy((batch, 2, level, N))
        for b in range(batch):
            digs = np.array(spec.window_digits([list(map(int, l)) for l in ct[b, -1]], cring, w, wring), dtype=np.uint64)
            assert digs.shape == (need, len(which), N)
            dh = ref.nntt(digs, which)
            S = np.zeros((2, len(which), N), dtype=np.uint64)
            for i in range(need):
                for s in (0, 1):
                    S[s] = ref.pointwise("add", S[s][None], ref.pointwise("mul", np.ascontiguousarray(evk[i, s][which])[None], dh[i][None], which), which)[0]
            S = ref.inntt(S, which)
            for s, comp in ((1, 0), (0, 1)):
                addend = ct[b, comp] if comp < polys - 1 else np.zeros((level, N), dtype=np.uint64)
                if special:
                    up = np.zeros((len(which), N), dtype=np.uint64)
                    up[:level] = ref.scalar_mul([qs[-1] % q for q in qs[:level]], addend[None], range(level))[0]
                    wantc = ref.modswitch(ref.pointwise("add", up[None], S[s][None], which), which)[0]
                else:
                    wantc = ref.pointwise("add", addend[None], S[s][None], which)[0]
                assert np.array_equal(got[b, comp], wantc), (polys, b, comp)


def test_keyswitch_window_oracle_composition_is_the_spec_at_a_small_size():
    """the composition used above (spec digits, oracle sums) against spec.keyswitch itself, where the spec is affordable"""
    N, w, Lk = 16, 16, 4
    qs = H.chain(40, Lk, N)
    keyring, cring = spec.Ring(N, qs), spec.Ring(N, qs[:3])
    ref, ctx = ref_cpu.RefCtx(N, qs), tf.Context(N, qs)
    nkey = spec.ndigits(cring.Q * qs[-1], 2 ** w)
    rng = np.random.default_rng(4)
    evk = fill(rng, qs, (nkey, 2), N)                                       # coefficient domain
    evk_ntt = ref.nntt(evk.reshape(-1, Lk, N)).reshape(evk.shape)
    ct = fill(rng, qs[:3], (1, 3), N)
    dout = tf.DeviceBuffer(2 * 3 * N)
    ctx.keyswitch_window(3, w, dev(evk_ntt).ptr, nkey, dev(ct).ptr, 3, dout.ptr, 1, key_limbs=Lk, special=True)
    L_ = lambda p: [list(map(int, l)) for l in p]
    want = spec.keyswitch([(L_(p[0]), L_(p[1])) for p in evk], [L_(c) for c in ct[0]], cring, keyring, True, relin_window=w)
    assert np.array_equal(dout.to_numpy((2, 3, N)), np.array(want, dtype=np.uint64))


# ---------------------------------------------------------------------------------------------------
# 4. mul_relin
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [32, 33])
@pytest.mark.parametrize("logn", [12, 14])
def test_mul_relin_fused_at_level_32_composed_at_level_33(logn, level):
    """tfhe_mul_relin on the 34-limb mixed key ring: level 32 runs the fused cores, level 33 the composition (mul_api.inc:
    level > 32).  Both equal the chain through the public entry points and the oracle's modswitch(keyswitch(ek, c1 * c2));
    with and without the rescale (CKKS / BGV rescale = True), ntt_in both ways, a square."""
    N = 1 << logn
    qs = ML.ring("M34", N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    evk = fill(np.random.default_rng(logn + level), qs, (level, 2), N)
    devk = dev(evk)
    k = 0
    for rescale in (0, 1):
        for ntt_in in (0, 1):
            k += 1
            MR.check_case(ctx, ref, qs, 34, level, True, evk, devk, 2, k == 4, ntt_in, rescale, 3200 + 10 * level + k, picks=[k % 2])


# ---------------------------------------------------------------------------------------------------
# 5. encrypt, decrypt phase, samplers
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc_ring():
    N = 1 << 12
    qs = ML.ring("M34", N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    assert ctx.psis == ref.psis
    return N, qs, ctx, ref


@pytest.mark.parametrize("level", [32, 33])
def test_encrypt_and_decrypt_phase_at_level_32_and_33(enc_ring, level):
    """tfhe_encrypt / tfhe_decrypt_phase on the 34-limb mixed key ring at N = 2^12: level 32 the fused kernels, level 33 the
    composition (enc_api.inc: level > 32); given randomness against tests/enc_oracle.py, the seeded form against the three
    tfhe_sample_gaussian draws it is defined by"""
    N, qs, ctx, ref_all = enc_ring
    Lk, batch = len(qs), 2
    ref = ref_cpu.RefCtx(N, qs[:level], ref_all.psis[:level])
    rng = np.random.default_rng(level)
    pk = fill(rng, qs, (2,), N)
    for mult, with_msg in ((1, True), (65537, False)):
        rand = np.rint(rng.normal(0.0, 3.2, size=(batch, 3, N))).astype(np.int64)
        rand[:, :, :5] = np.array([2**31 - 1, -2**31, 0, 1, -1])
        msg = fill(rng, qs[:level], (batch,), N) if with_msg else None
        out = tf.DeviceBuffer(batch * 2 * level * N)
        dm = None if msg is None else dev(msg)
        drand = dev(np.ascontiguousarray(rand, dtype=np.int32).reshape(-1).view(np.uint64))
        ctx.encrypt(Lk, level, dev(pk).ptr, out.ptr, batch, msg=None if dm is None else dm.ptr, rand=drand.ptr, mult_e=mult)
        got = out.to_numpy((batch, 2, level, N))
        assert np.array_equal(got, EO.encrypt_ref(ref, pk[:, :level], rand, mult, msg)), (mult, with_msg)
    # the counter convention: u, e1, e2 are the Gaussian polynomials first + b, first + batch + b, first + 2 batch + b
    first, seed, su, se, mult = 17, 0xC0FFEE, 3.2, 19.5, 257

    def gauss(first_poly, sigma, m):
        o = tf.DeviceBuffer(batch * level * N)
        ctx.sample_gaussian(level, sigma, m, seed, 1, first_poly, o.ptr, batch)
        return o.to_numpy((batch, level, N))
    u, e1, e2 = gauss(first, su, 1), gauss(first + batch, se, mult), gauss(first + 2 * batch, se, mult)
    one = np.zeros((2, Lk, N), dtype=np.uint64)
    one[1] = 1                                                            # masked = the NTT image of the constant 1, mask = 0
    out = tf.DeviceBuffer(batch * 2 * level * N)
    ctx.encrypt(Lk, level, dev(one).ptr, out.ptr, batch, sigma_u=su, sigma_e=se, mult_e=mult, seed=seed, stream=1, first_poly=first)
    got = out.to_numpy((batch, 2, level, N))
    assert np.array_equal(ref.pointwise("sub", got[:, 0], e1), u) and np.array_equal(got[:, 1], e2)
    # decryption phase, 2 and 3 components, both input domains
    s = fill(rng, qs, (), N)
    for polys in (2, 3):
        for ntt_in in (False, True):
            ct = fill(rng, qs[:level], (batch, polys), N)
            dph = tf.DeviceBuffer(batch * level * N)
            ctx.decrypt_phase(Lk, level, dev(s).ptr, dev(ct).ptr, polys, dph.ptr, batch, ntt_in=ntt_in)
            assert np.array_equal(dph.to_numpy((batch, level, N)), EO.decrypt_ref(ref, s[:level], ct, ntt_in)), (polys, ntt_in)


@pytest.mark.parametrize("L", [32, 33])
def test_mirror_encryption_leaves_the_generator_where_the_composition_does(L):
    """she.encrypt_zero through tfhe_encrypt against the term-by-term composition on ring elements, from the same generator
    state: the same residues and the same state afterwards (the statement of test_gpu_encrypt.py, in one process)"""
    N, batch = 1 << 12, 2
    R = tf.NegacyclicRing(N, ML.mixed(L, N))
    params = tf.CKKSParams(R, 0, 3.2)
    rng = tf.DeviceRng(77)
    kp = tf.keygen(rng, params)
    start = rng.next_poly
    a = tf.she.encrypt_zero(rng, kp.pub, batch)
    rng2 = tf.DeviceRng(77)
    rng2.next_poly = start
    b = tf.she._encrypt_zero_composed(rng2, kp.pub, batch)
    assert rng.next_poly == rng2.next_poly == start + 3 * batch
    for x, y in zip(a.cs, b.cs):
        assert np.array_equal(x.to_numpy(), y.to_numpy())


def test_samplers_at_level_40():
    """tfhe_sample_uniform / tfhe_sample_gaussian at 40 limbs: the Philox counter packs the limb index; sampled positions of
    every limb against oracle/spec.py's restatement of the stream"""
    N = 1 << 10
    qs = ML.mixed40(N)
    ctx = tf.Context(N, qs)
    seed, first, count = 0x1234567890ABCDEF, 5, 2
    out = tf.DeviceBuffer(count * 40 * N)
    ctx.sample_uniform(40, seed, 0, first, out.ptr, count)
    got = out.to_numpy((count, 40, N))
    ks = [0, 1, 2, 3, 511, N - 1]
    for p in range(count):
        for l, q in enumerate(qs):
            assert [int(got[p, l, k]) for k in ks] == [spec.sample_uniform_mod(((first + p) << 32) | k, l, 0, seed, q) for k in ks], (p, l)
    assert all(int(got[:, l].max()) < q for l, q in enumerate(qs))
    assert len({got[0, l].tobytes() for l in range(40)}) == 40                # no two limbs share a stream
    ctx.sample_gaussian(40, 3.2, 1, seed, 1, first, out.ptr, count)
    g = out.to_numpy((count, 40, N))
    want = np.array([[spec.sample_gauss_int(((first + p) << 32) | k, 1, seed, 3.2) for k in range(N)] for p in range(count)])
    cent = np.where(g[:, 1] > qs[1] // 2, g[:, 1].astype(np.int64) - qs[1], g[:, 1].astype(np.int64))
    assert (cent != want).mean() < 0.01                                       # (the rule of test_device_samplers_match_the_stream_definition)
    for l, q in enumerate(qs):                                                # the same integer in every one of the 40 limbs
        assert np.array_equal(g[:, l], np.mod(cent, q).astype(np.uint64)), l


# ---------------------------------------------------------------------------------------------------
# 6. plain codec
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [65537, 257])
@pytest.mark.parametrize("k", [17, 32, 33, 40])
@pytest.mark.parametrize("name", ["W40", "mixed40"])
def test_plain_codec_on_17_to_40_limbs(name, k, t):
    """tfhe_plain_encode / tfhe_plain_decode (BFV and BGV) and tfhe_bfv_noise_max on prefixes of 17, 32, 33 and 40 limbs (the
    rolled KM = 40 bodies): random residues and the edge inputs of tests/test_plain_codec_cpu.py (multiples of Delta +- 1, exact
    ties, Q / 2 +- 1) against spec.bfv_decode / bgv_decode / bfv_encode and the big-integer noise remainder"""
    N, count = 1 << 10, 2
    full = ML.ring("W40", N) if name == "W40" else ML.mixed40(N)
    qs = full[:k]
    ctx = tf.Context(N, full)
    plan = tf.PlainPlan(ctx, t, list(range(k)))
    Q = 1
    for q in qs:
        Q *= q
    delta = Q // t
    prng = random.Random(k * 1000 + t)
    xs = codec_edge_inputs(Q, delta, prng)
    assert len(xs) < N
    rng = np.random.default_rng(k + t)
    res = fill(rng, qs, (count,), N)
    res[0, :, :len(xs)] = np.array([[x % q for x in xs] for q in qs], dtype=np.uint64)
    src = dev(res)
    ring = spec.Ring(N, qs, [1] * k)
    out = tf.DeviceBuffer(count * N)
    words = tf.DeviceBuffer(count * plan.delta_words)
    plan.noise_max(src.ptr, words.ptr, count)
    got_words = words.to_numpy((count, plan.delta_words))
    for scheme, dec in ((tf.native.PLAIN_BFV, spec.bfv_decode), (tf.native.PLAIN_BGV, spec.bgv_decode)):
        plan.decode(scheme, src.ptr, out.ptr, count)
        got = out.to_numpy((count, N))
        for b in range(count):
            assert got[b].tolist() == dec([[int(v) for v in l] for l in res[b]], ring, t), (scheme, b)
    for b in range(count):
        ints = spec.poly_to_ints([[int(v) for v in l] for l in res[b]], ring)
        worst = max((delta - x % delta) if x % delta > delta // 2 else x % delta for x in ints)
        assert sum(int(wd) << (64 * i) for i, wd in enumerate(got_words[b])) == worst, b
    m = rng.integers(0, 2**63, size=(count, N), dtype=np.uint64)
    m[0, :8] = [0, 1, t - 1, t, t + 1, 2 * t - 1, 2**63, 2**64 - 1]
    dm, enc = dev(m), tf.DeviceBuffer(count * k * N)
    for scheme in (tf.native.PLAIN_BFV, tf.native.PLAIN_BGV):
        plan.encode(scheme, dm.ptr, enc.ptr, count)
        got = enc.to_numpy((count, k, N))
        for b in range(count):
            mi = [int(v) for v in m[b]]
            want = spec.bfv_encode(mi, ring, t) if scheme == tf.native.PLAIN_BFV else [[x % t % q for x in mi] for q in qs]
            assert got[b].tolist() == want, (scheme, b)
    plan.close()


# ---------------------------------------------------------------------------------------------------
# 7. CKKS encode / decode
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2**40, 2**80])
@pytest.mark.parametrize("L", [17, 33, 40])
@pytest.mark.parametrize("bits", [40, 61])
@pytest.mark.parametrize("logn", [6, 12])
def test_ckks_encode_decode_on_17_to_40_limbs(logn, bits, L, scale):
    """the comparison of test_gpu_parity.test_ckks_encode_decode_match_oracle, rule and tolerances unchanged, at 17, 33 and
    40 limbs: xi[40] / w[41] of the decode's reconstruction in full use.  encode: integer coefficients equal to the oracle's
    except +-1 at rounding boundaries (beyond 53 bits of scale a last-place difference of the double scales up with it);
    decode: per-slot error <= 8 log2(N) eps max|slot| (x 4).  One element at N = 2^12 (the big-integer oracle takes a second
    per 40-limb polynomial), three at N = 2^6."""
    N = 1 << logn
    qs = H.chain(bits, L, N)
    ring = spec.Ring(N, qs)
    ctx = tf.Context(N, qs)
    rng = np.random.default_rng(N + L)
    batch = 1 if logn == 12 else 3
    slots = rng.normal(size=(batch, N // 2)) * 3 + 1j * rng.normal(size=(batch, N // 2))
    slots[0, :4] = [1.0, -2.5, 0.0, 1j]
    mant, exp2 = tf.she.scale_parts(scale)
    dz = tf.DeviceBuffer.from_numpy(np.ascontiguousarray(slots).view(np.uint64))
    dout = tf.DeviceBuffer(batch * L * N)
    ctx.ckks_encode(L, mant, exp2, dz.ptr, dout.ptr, batch)
    res = dout.to_numpy((batch, L, N))
    eps = 2.0 ** -53
    for b in range(batch):
        want = spec.poly_to_ints(spec.ckks_encode(list(slots[b]), ring, scale), ring)
        got = spec.poly_to_ints([list(map(int, l)) for l in res[b]], ring)
        diff = [spec.centred(g - w, ring.Q) for g, w in zip(got, want)]
        allowed = max(1, int(8 * np.log2(N) * eps * np.abs(slots[b]).max() * float(scale)))
        assert max(abs(d) for d in diff) <= allowed, (max(abs(d) for d in diff), allowed)
        if allowed == 1:
            assert sum(1 for d in diff if d) <= max(2, N // 20)      # boundary flips are rare
        dslots = tf.DeviceBuffer(N)
        one = tf.DeviceBuffer.from_numpy(res[b])
        ctx.ckks_decode(L, mant, exp2, one.ptr, dslots.ptr, 1)
        dec = dslots.to_numpy().view(np.complex128)
        ref = spec.ckks_decode([list(map(int, l)) for l in res[b]], ring, scale)
        tol = 8 * np.log2(N) * eps * max(1.0, np.abs(ref).max()) * 4
        assert np.abs(dec - ref).max() <= tol, (np.abs(dec - ref).max(), tol)
        assert np.abs(dec - slots[b]).max() <= N * 2.0 / float(scale) + tol   # round trip: quantisation 1/scale per coefficient
    # decode of arbitrary ring elements: centred magnitudes up to Q / 2 -- as far as the quotient by the scale is a double at
    # all (Q passes 2^1024 at 17 limbs of 61 bits; 2^1000 leaves the sum over N coefficients finite)
    bound = min(ring.Q // 2, (1 << 1000) * int(scale))
    prng = random.Random(N + L)
    xs = [prng.randrange(-bound, bound + 1) for _ in range(N)]
    xs[:4] = [bound, -bound, 1, -1]
    a = np.array([[x % q for x in xs] for q in qs], dtype=np.uint64)[None]
    da, dslots = dev(a), tf.DeviceBuffer(N)
    ctx.ckks_decode(L, mant, exp2, da.ptr, dslots.ptr, 1)
    dec = dslots.to_numpy().view(np.complex128)
    ref = spec.ckks_decode([list(map(int, l)) for l in a[0]], ring, scale)
    assert np.abs(dec - ref).max() <= 32 * np.log2(N) * eps * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------
# 8. BFV outside the fast-path tables
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["superset", "disjoint"])
@pytest.mark.parametrize("logn,bits,ns,nb", [(6, 50, 13, 27), (6, 61, 19, 40), (12, 50, 19, 40), (12, 61, 13, 27)])
def test_bfv_beyond_the_fast_path_tables(mode, logn, bits, ns, nb):
    """bfv_expand / bfv_contract / bfv_mul / bfv_mul_relin with (ns, nb) = (13, 27) and (19, 40): past TFHE_FAST_MAX = 12, the
    general conversion kernels at up to 40 extension limbs"""
    N, t = 1 << logn, 65537
    ch = H.chain(bits, ns + nb, N)
    qs = ch[:ns]
    pb = ch[:nb] if mode == "superset" else ch[ns:]
    rs, rb = ref_cpu.RefCtx(N, qs), ref_cpu.RefCtx(N, pb)
    small, big = spec.Ring(N, qs, [1] * ns), spec.Ring(N, pb, [1] * nb)      # (moduli only: the edge values below)
    if mode == "superset":
        cbig = tf.Context(N, pb); csmall = cbig
        plan = tf.BfvPlan(csmall, cbig, t, idx_s=list(range(ns)), idx_b=None)
    else:
        csmall, cbig = tf.Context(N, qs), tf.Context(N, pb)
        plan = tf.BfvPlan(csmall, cbig, t)
    rng = np.random.default_rng(N + ns)
    a = fill(rng, qs, (2,), N)
    for k, x in enumerate([0, 1, small.Q - 1, small.Q // 2, small.Q // 2 + 1]):
        a[0, :, k] = [x % q for q in qs]
    da, de = dev(a), tf.DeviceBuffer(2 * nb * N)
    plan.expand(da.ptr, de.ptr, 2)
    assert np.array_equal(de.to_numpy((2, nb, N)), ref_cpu.switch(rs, rb, a))
    y = fill(rng, pb, (2,), N)
    tinv = pow(t, -1, big.Q)
    edges = [0, 1, big.Q - 1, big.Q // 2, big.Q // 2 + 1, small.Q // 2, small.Q // 2 + 1, small.Q,
             5 * small.Q + small.Q // 2, 5 * small.Q + small.Q // 2 + 1, big.Q - small.Q // 2 - 1]
    for k, x in enumerate(edges):
        y[0, :, k] = [(x * tinv) % big.Q % p for p in pb]
    dy, dc = dev(y), tf.DeviceBuffer(2 * ns * N)
    plan.contract(dy.ptr, dc.ptr, 2)
    assert np.array_equal(dc.to_numpy((2, ns, N)), ref_cpu.contract(rb, rs, t, y))
    batch = 3
    plan.set_chunk(2)                                                       # a ragged last chunk
    c1, c2 = fill(rng, qs, (batch, 2), N), fill(rng, qs, (batch, 2), N)
    evk = fill(rng, qs, (ns, 2), N)
    d1, d2, devk, do = dev(c1), dev(c2), dev(evk), tf.DeviceBuffer(batch * 3 * ns * N)
    plan.mul(d1.ptr, d2.ptr, do.ptr, batch)
    prod = ref_cpu.bfv_mul(rs, rb, t, c1, c2)
    assert np.array_equal(do.to_numpy((batch, 3, ns, N)), prod)
    do2 = tf.DeviceBuffer(batch * 2 * ns * N)
    plan.mul_relin(devk.ptr, ns, d1.ptr, d2.ptr, do2.ptr, batch)
    assert np.array_equal(do2.to_numpy((batch, 2, ns, N)), rs.keyswitch(ns, False, evk, prod))


def test_bfv_mul_relin_with_13_of_27_limbs_decrypts():
    """test_bfv_mul_relin_matches_oracle_and_decrypts at (ns, nb) = (13, 27): genuine encryptions of 6, 3 and 7, 5 under a
    genuine relinearisation key"""
    N, t, ns, nb = 64, 65537, 13, 27
    pb = H.chain(50, nb, N)
    qs = pb[:ns]
    rs, rb = ref_cpu.RefCtx(N, qs), ref_cpu.RefCtx(N, pb)
    ring = spec.Ring(N, qs)
    secret, evk = H.real_evk(5, N, qs, special=False)
    prng = random.Random(6)
    s_l = [[int(v) for v in l] for l in secret]

    def enc(m):
        mask = [[prng.randrange(q) for _ in range(N)] for q in qs]
        e = spec.poly_from_ints(spec.sample_gauss_ints(prng, N, 3.2), ring)
        c0 = spec.poly_sub(spec.poly_add(spec.bfv_encode([m] + [0] * (N - 1), ring, t), e, ring), spec.poly_mul(mask, s_l, ring), ring)
        return [c0, mask]
    c1 = np.array([enc(6), enc(3)], dtype=np.uint64); c2 = np.array([enc(7), enc(5)], dtype=np.uint64)
    ctx = tf.Context(N, pb)
    plan = tf.BfvPlan(ctx, ctx, t, idx_s=list(range(ns)))
    d1, d2, devk, do = dev(c1), dev(c2), dev(evk), tf.DeviceBuffer(2 * 2 * ns * N)
    plan.mul_relin(devk.ptr, ns, d1.ptr, d2.ptr, do.ptr, 2)
    got = do.to_numpy((2, 2, ns, N))
    assert np.array_equal(got, rs.keyswitch(ns, False, evk, ref_cpu.bfv_mul(rs, rb, t, c1, c2)))
    for b, m in enumerate((42, 15)):
        dec = spec.bfv_decode(spec.decrypt_raw(s_l, [[[int(v) for v in l] for l in p] for p in got[b]], ring), ring, t)
        assert dec[0] == m and not any(dec[1:])


# ---------------------------------------------------------------------------------------------------
# 9. argument edges
# ---------------------------------------------------------------------------------------------------
def test_argument_edges_at_the_limb_limit():
    N = 32
    ch = H.chain(40, 41, N)
    with pytest.raises(AssertionError, match=r"L=41 out of range \[1,40\]"):
        tf.Context(N, ch)                                                   # L = 41: TFHE_E_BADARG
    ctx = tf.Context(N, ch[:40])
    buf = tf.DeviceBuffer(2 * 41 * 40 * N)
    with pytest.raises(AssertionError, match=r"limbs=41 out of range \[1,40\]"):
        ctx.nntt(buf.ptr, buf.ptr, 1, 41)                                   # limbs = 41: the cap, before any look at the ring
    with pytest.raises(AssertionError, match=r"limbs=41 out of range \[1,40\]"):
        ctx.add(buf.ptr, buf.ptr, buf.ptr, 1, 41, list(range(40)) + [0])
    with pytest.raises(AssertionError, match="bad limb count"):
        ctx.select_limbs(buf.ptr, buf.ptr, 1, 40, list(range(40)) + [0])    # 41 selected limbs
    with pytest.raises(tf.UsageError, match=r"level=40 outside \[1,39\]"):
        ctx.keyswitch(40, 40, True, buf.ptr, 40, buf.ptr, 2, buf.ptr, 1)    # level 40 + special on a 40-limb key: LEVEL_MISMATCH
    with pytest.raises(tf.UsageError, match=r"level=40 outside \[1,39\]"):
        ctx.rotate(40, 40, True, buf.ptr, 40, 3, buf.ptr, buf.ptr, 1)
    with pytest.raises(tf.UsageError, match=r"level=41 outside \[1,40\]"):
        ctx.keyswitch(40, 41, False, buf.ptr, 41, buf.ptr, 2, buf.ptr, 1)
    a = np.arange(40 * N, dtype=np.uint64).reshape(1, 40, N) % 1000         # the context still works
    assert np.array_equal(P.run_ntt(ctx, P.run_ntt(ctx, a), inverse=True), a)


# ---------------------------------------------------------------------------------------------------
# the randomised sweep of test_gpu_parity, widened: 18 to 40 limbs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_random_shapes_against_the_oracle(seed):
    rng = np.random.default_rng(9100 + seed)
    logn = int(rng.choice([5, 10, 12, 13, 14]))
    L = int(rng.integers(18, 41))
    N, qs = P._random_ring(rng, logn, L)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    batch = int(rng.integers(1, 3))
    a = fill(rng, qs, (batch,), N)
    f = P.run_ntt(ctx, a)
    assert np.array_equal(f, ref.nntt(a)), ("nntt", logn, qs)
    assert np.array_equal(P.run_ntt(ctx, f, inverse=True), a), ("inntt", logn, qs)
    idx = rng.permutation(L)[: int(rng.integers(1, L + 1))].tolist()
    sub = np.ascontiguousarray(a[:, idx])
    assert np.array_equal(P.run_ntt(ctx, sub, idx=idx), ref.nntt(sub, idx=idx)), ("nntt subset", idx)
    g = int(rng.choice([3, 5, 2 * N - 1, pow(3, int(rng.integers(1, N)), 2 * N)]))
    da, dg = dev(a), tf.DeviceBuffer(a.size)
    ctx.galois(da.ptr, dg.ptr, g, batch, L)
    assert np.array_equal(dg.to_numpy(a.shape), ref.galois(g, a)), ("galois", g)
    dr = tf.DeviceBuffer(batch * (L - 1) * N)
    ctx.rescale(da.ptr, dr.ptr, batch, L)
    assert np.array_equal(dr.to_numpy((batch, L - 1, N)), ref.modswitch(a)), "rescale"
    special = bool(rng.integers(0, 2))
    maxlevel = L - 1 if special else L
    level = int(rng.integers(17, maxlevel + 1))
    polys = int(rng.choice([2, 3]))
    evk = fill(rng, qs, (level, 2), N)
    ct = fill(rng, qs[:level], (batch, polys), N)
    devk, dct, dout = dev(evk), dev(ct), tf.DeviceBuffer(batch * 2 * level * N)
    ctx.keyswitch(L, level, special, devk.ptr, level, dct.ptr, polys, dout.ptr, batch)
    assert np.array_equal(dout.to_numpy((batch, 2, level, N)), ref.keyswitch(level, special, evk, ct)), ("keyswitch", level, special, polys, qs)
    ct2 = np.ascontiguousarray(ct[:, :2])
    dct2 = dev(ct2)
    ctx.rotate(L, level, special, devk.ptr, level, g, dct2.ptr, dout.ptr, batch)
    assert np.array_equal(dout.to_numpy((batch, 2, level, N)), ref.keyswitch(level, special, evk, galois_ref(ref, g, ct2))), ("rotate", g, level, special)
    gs = [g, int(pow(3, int(rng.integers(1, N)), 2 * N)), 2 * N - 1]
    many = tf.DeviceBuffer(len(gs) * batch * 2 * level * N)
    ctx.rotate_many(L, level, special, [devk.ptr] * len(gs), level, gs, dct2.ptr, many.ptr, batch)
    got = many.to_numpy((len(gs), batch, 2, level, N))
    for r, gr in enumerate(gs):
        ctx.rotate(L, level, special, devk.ptr, level, gr, dct2.ptr, dout.ptr, batch)
        assert np.array_equal(got[r], dout.to_numpy((batch, 2, level, N))), ("rotate_many", gr, level, special)
