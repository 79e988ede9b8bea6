"""tfhe_rotate_many_grouped / tfhe_matmul_diag_grouped on the device against tests/rotate_many_grouped_oracle.py, word for word, every
word read back below its modulus and `out` pre-filled with 0xA5..: the seams of the XCD-cooperative walk and of the 64-key tile; the
signs of the scatter; the shape matrix of tests/test_gpu_ks_grouped.py and N = 2^15; parity with the unhoisted tfhe_rotate_grouped and,
in the two degenerate cases, with tfhe_rotate_many; edge words; chunks; the product against the oracle and against rotate_many_grouped
-> nntt -> dot; every host check with a context; a dirty workspace; and the mirror end to end.  The keys reach the device through
tfhe_galois_key_prepare; the oracle gets the plain key."""
import math

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import helpers as H
from tests import ks_grouped_oracle as KO
from tests import rotate_many_grouped_oracle as RO
from tests.dirty_ws import on_dirty_workspace
from tests.test_gpu_chunk_seams import cap
from tests.test_gpu_ks_grouped import SHAPES, _mixed13, dev, operands, pair, plant, poisoned, qcol

pytestmark = pytest.mark.gpu
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)


def g_many(N):
    return pow(3, N // 2 + 3, 2 * N)


def prepare(ctx, Lk, evk, g):
    """the device copy of a plain key [nd][2][Lk][N] as tfhe_galois_key_prepare leaves it for g"""
    src, dst = dev(evk), tf.DeviceBuffer(evk.size)
    ctx.galois_key_prepare(Lk, evk.shape[0], g, src.ptr, dst.ptr)
    return dst


def key_set(N, qs, k, alpha, level, gs, n_keys=None, edge=False, seed=0):
    """plain keys (n_keys distinct ones, dealt round robin over the Galois elements `gs`) and their prepared device copies: a key used
    with two different elements is prepared once per element"""
    ctx, _ = pair(N, qs)
    n_keys = len(gs) if n_keys is None else n_keys
    plain = [operands(N, qs, k, alpha, level, 2, 1, seed=seed + 17 * i, edge=edge)[0] for i in range(n_keys)]
    evks = [plain[r % n_keys] for r in range(len(gs))]
    made = {}
    devs = []
    for r, g in enumerate(gs):
        key = (r % n_keys, int(g))
        if key not in made:
            made[key] = prepare(ctx, len(qs), evks[r], g)
        devs.append(made[key])
    return evks, devs


def run_many(N, qs, k, alpha, level, evks, devs, gs, ct, want=None):
    ctx, ref = pair(N, qs)
    batch = ct.shape[0]
    dct, out = dev(ct), poisoned(len(gs) * batch * 2 * level * N)
    ctx.rotate_many_grouped(len(qs), level, k, alpha, [d.ptr for d in devs], evks[0].shape[0], gs, dct.ptr, out.ptr, batch)
    got = out.to_numpy((len(gs), batch, 2, level, N))
    assert (got < qcol(qs[:level])).all()
    if want is None:
        want = RO.rotate_many_grouped_ref(ref, level, k, alpha, evks, gs, ct)
    assert np.array_equal(got, want), (N, k, alpha, level, batch, len(gs), int((got != want).sum()))
    return got


def run_diag(N, qs, k, alpha, level, evks, devs, gs, diags, ct, want=None):
    ctx, ref = pair(N, qs)
    batch = ct.shape[0]
    dct, dd, out = dev(ct), dev(diags), poisoned(batch * 2 * level * N)
    ctx.matmul_diag_grouped(len(qs), level, k, alpha, [d.ptr for d in devs], evks[0].shape[0] if evks else level, gs, dd.ptr, dct.ptr, out.ptr, batch)
    got = out.to_numpy((batch, 2, level, N))
    assert (got < qcol(qs[:level])).all()
    if want is None:
        want = RO.matmul_diag_grouped_ref(ref, level, k, alpha, evks, gs, diags, ct)
    assert np.array_equal(got, want), (N, k, alpha, level, batch, len(gs), int((got != want).sum()))
    return got


# ---- 1. the seams of the walk and of the tile ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rot,batch", [(1, 1), (3, 1), (5, 3), (65, 1)])
def test_walk_and_tile_seams(n_rot, batch):
    """2 and 6 row groups (fewer than the 8 XCDs, idle slots), 30 (not a multiple of 8), and 65 rotations over three keys repeated:
    across the 64-key tile"""
    N, k, alpha, level = 64, 2, 2, 5
    qs = H.chain(30, 8, N)
    steps = [pow(5, r + 1, 2 * N) for r in range(n_rot)]
    evks, devs = key_set(N, qs, k, alpha, level, steps, n_keys=min(n_rot, 3))
    _, ct = operands(N, qs, k, alpha, level, 2, batch, seed=n_rot)
    run_many(N, qs, k, alpha, level, evks, devs, steps, ct)


# ---- 2. the signs ------------------------------------------------------------------------------------------------------------------

def test_signs_of_the_scatter():
    """g = 1 never flips a sign, g = 2N - 1 flips every one but index 0; 5 and its inverse; many wraps -- in one call"""
    N, k, alpha, level = 64, 2, 2, 5
    qs = H.chain(30, 8, N)
    gs = [1, 2 * N - 1, 5, pow(5, -1, 2 * N), g_many(N)]
    evks, devs = key_set(N, qs, k, alpha, level, gs)
    _, ct = operands(N, qs, k, alpha, level, 2, 2, seed=3)
    run_many(N, qs, k, alpha, level, evks, devs, gs, ct)


# ---- 3. the shape matrix ---------------------------------------------------------------------------------------------------------

SMALL = [p for p in SHAPES if p.values[0] <= 1 << 13]


@pytest.mark.parametrize("N,ring,k,alpha,level,batch", SMALL)
def test_shape_matrix_matches_the_oracle(N, ring, k, alpha, level, batch):
    qs = ring(N)
    gs = [g_many(N), 2 * N - 1, 3]
    evks, devs = key_set(N, qs, k, alpha, level, gs)
    _, ct = operands(N, qs, k, alpha, level, 2, batch, seed=5)
    run_many(N, qs, k, alpha, level, evks, devs, gs, plant(ct, qs, level, alpha))


def test_at_2_to_15_the_transforms_take_region_0():
    N, k, alpha, level, batch = 1 << 15, 2, 2, 4, 2
    qs = H.chain(40, 6, N)
    gs = [g_many(N), 2 * N - 1]
    evks, devs = key_set(N, qs, k, alpha, level, gs)
    _, ct = operands(N, qs, k, alpha, level, 2, batch, seed=6)
    run_many(N, qs, k, alpha, level, evks, devs, gs, ct)


# ---- 4. parity with the unhoisted route, device against device -----------------------------------------------------------------

@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (1 << 12, lambda N: H.chain(50, 7, N), 2, 2, 5),
                                                  (1 << 13, _mixed13, 2, 2, 4)])
def test_every_rotation_is_tfhe_rotate_grouped_on_the_plain_key(N, ring, k, alpha, level):
    qs = ring(N)
    ctx, _ = pair(N, qs)
    batch = 3
    gs = [g_many(N), 2 * N - 1, 5]
    evks, devs = key_set(N, qs, k, alpha, level, gs)
    _, ct = operands(N, qs, k, alpha, level, 2, batch, seed=8)
    dct, one = dev(ct), poisoned(batch * 2 * level * N)
    want = np.empty((len(gs), batch, 2, level, N), dtype=np.uint64)
    for r, g in enumerate(gs):
        plain = dev(evks[r])
        ctx.rotate_grouped(len(qs), level, k, alpha, plain.ptr, evks[r].shape[0], g, dct.ptr, one.ptr, batch)
        want[r] = one.to_numpy((batch, 2, level, N))
    run_many(N, qs, k, alpha, level, evks, devs, gs, ct, want=want)


@pytest.mark.parametrize("special", [1, 0])
@pytest.mark.parametrize("N,bits", [(64, 30), (1 << 12, 50)])
def test_one_limb_per_digit_is_tfhe_rotate_many_on_the_same_prepared_keys(N, bits, special):
    Lk = 4
    qs = H.chain(bits, Lk, N)
    ctx, _ = pair(N, qs)
    level, batch = Lk - special, 2
    gs = [g_many(N), 2 * N - 1, 3]
    evks, devs = key_set(N, qs, special, 1, level, gs)     # (tfhe_rotate_many reads `level` components: operands' spare one is the special prime's)
    evks = [e[:level] for e in evks]
    devs = [prepare(ctx, Lk, e, g) for e, g in zip(evks, gs)]
    _, ct = operands(N, qs, special, 1, level, 2, batch, seed=2)
    dct, a = dev(ct), poisoned(len(gs) * batch * 2 * level * N)
    ctx.rotate_many(Lk, level, special, [d.ptr for d in devs], level, gs, dct.ptr, a.ptr, batch, prepared=True)
    run_many(N, qs, special, 1, level, evks, devs, gs, ct, want=a.to_numpy((len(gs), batch, 2, level, N)))


# ---- 5. edge words -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (256, lambda N: H.chain(61, 6, N), 2, 4, 4)])
def test_every_word_q_minus_1_and_the_planted_group_integers(N, ring, k, alpha, level):
    qs = ring(N)
    gs = [2 * N - 1, g_many(N)]
    evks, devs = key_set(N, qs, k, alpha, level, gs, edge=True)
    _, ct = operands(N, qs, k, alpha, level, 2, 2, edge=True)
    run_many(N, qs, k, alpha, level, evks, devs, gs, ct)
    run_many(N, qs, k, alpha, level, evks, devs, gs, plant(ct.copy(), qs, level, alpha))
    evks, devs = key_set(N, qs, k, alpha, level, gs, seed=1)
    run_many(N, qs, k, alpha, level, evks, devs, gs, plant(ct, qs, level, alpha))


# ---- 6. chunks ----------------------------------------------------------------------------------------------------------------------

def _diagonals(N, qs, level, n_rot, seed=0):
    return H.rand_residues(np.random.default_rng(seed + n_rot), qs[:level], (n_rot + 1,), N)


@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (1 << 12, lambda N: H.chain(50, 6, N), 2, 3, 4)])
def test_batch_five_under_every_chunk_cap(N, ring, k, alpha, level):
    """the rotations of a chunk land a whole batch apart in the caller's array: identical words under caps 1, 2 and none"""
    qs = ring(N)
    ctx, ref = pair(N, qs)
    gs = [g_many(N), 2 * N - 1, 5]
    evks, devs = key_set(N, qs, k, alpha, level, gs)
    _, ct = operands(N, qs, k, alpha, level, 2, 5, seed=2)
    diags = _diagonals(N, qs, level, len(gs))
    want = RO.rotate_many_grouped_ref(ref, level, k, alpha, evks, gs, ct)
    want_d = RO.matmul_diag_grouped_ref(ref, level, k, alpha, evks, gs, diags, ct)
    for c in (1, 2, 0):
        with cap(ctx, c):
            run_many(N, qs, k, alpha, level, evks, devs, gs, ct, want=want)
            run_diag(N, qs, k, alpha, level, evks, devs, gs, diags, ct, want=want_d)
    # an empty batch and no rotation leave `out` untouched
    out = poisoned(2 * level * N)
    ptrs = [d.ptr for d in devs]
    ctx.rotate_many_grouped(len(qs), level, k, alpha, ptrs, evks[0].shape[0], gs, devs[0].ptr, out.ptr, 0)
    ctx.matmul_diag_grouped(len(qs), level, k, alpha, ptrs, evks[0].shape[0], gs, devs[1].ptr, devs[0].ptr, out.ptr, 0)
    ctx.rotate_many_grouped(len(qs), level, k, alpha, [], evks[0].shape[0], [], devs[0].ptr, out.ptr, 1)
    ctx.sync()
    assert (out.to_numpy() == POISON).all()


# ---- 7. the product ----------------------------------------------------------------------------------------------------------------

def _composition(N, qs, level, rots, ct, diags):
    """rotate_many_grouped -> nntt -> dot on the device: [batch][2][level][N]"""
    ctx, _ = pair(N, qs)
    batch, sz = ct.shape[0], 2 * level * N
    terms = np.concatenate([ct[None], rots])                                   # [R + 1][batch][2][level][N]
    img = dev(terms)
    ctx.nntt(img.ptr, img.ptr, terms.shape[0] * batch * 2, level)
    out, dd = poisoned(batch * sz), dev(diags)
    bd = [tf.DeviceBuffer(batch * sz) for _ in range(terms.shape[0])]          # every diagonal against every component of the batch
    for r, b in enumerate(bd):
        tf.native.check(tf.native.lib().tfhe_broadcast_poly(ctx.h, b.ptr, dd.ptr + r * level * N * 8, level * N, batch * 2))
    ctx.dot(None, [img.ptr + r * batch * sz * 8 for r in range(terms.shape[0])], [b.ptr for b in bd], out.ptr, batch * 2, level)
    return out.to_numpy((batch, 2, level, N))


@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (1 << 12, lambda N: H.chain(50, 7, N), 2, 2, 5),
                                                  (1 << 13, _mixed13, 2, 2, 4)])
@pytest.mark.parametrize("n_rot", [0, 1, 6])
def test_product_matches_the_oracle_and_the_composition(N, ring, k, alpha, level, n_rot):
    qs = ring(N)
    batch = 2
    gs = [pow(5, r + 1, 2 * N) for r in range(n_rot)]
    evks, devs = key_set(N, qs, k, alpha, level, gs, n_keys=min(n_rot, 2)) if n_rot else ([], [])
    _, ct = operands(N, qs, k, alpha, level, 2, batch, seed=4)
    diags = _diagonals(N, qs, level, n_rot)
    got = run_diag(N, qs, k, alpha, level, evks, devs, gs, diags, ct)
    rots = run_many(N, qs, k, alpha, level, evks, devs, gs, ct, want=None) if n_rot else np.empty((0,) + ct.shape, dtype=np.uint64)
    assert np.array_equal(got, _composition(N, qs, level, rots, ct, diags))


def test_product_of_64_rotations_and_the_refusal_of_65():
    N, k, alpha, level = 64, 2, 2, 5
    qs = H.chain(30, 8, N)
    ctx, _ = pair(N, qs)
    gs = [pow(5, r + 1, 2 * N) for r in range(64)]
    evks, devs = key_set(N, qs, k, alpha, level, gs, n_keys=3)
    _, ct = operands(N, qs, k, alpha, level, 2, 1, seed=7)
    run_diag(N, qs, k, alpha, level, evks, devs, gs, _diagonals(N, qs, level, 64), ct)
    out = poisoned(2 * level * N)
    dct = dev(ct)
    dd = dev(_diagonals(N, qs, level, 65))
    with pytest.raises(NotImplementedError, match="at most 64 rotations"):
        ctx.matmul_diag_grouped(len(qs), level, k, alpha, [devs[0].ptr] * 65, evks[0].shape[0], [5] * 65, dd.ptr, dct.ptr, out.ptr, 1)
    ctx.sync()
    assert (out.to_numpy() == POISON).all()


# ---- 8. the host checks, with a context --------------------------------------------------------------------------------------------

def test_host_checks_in_the_headers_order_leave_the_output_untouched():
    N = 64
    qs = H.chain(30, 6, N)
    ctx, _ = pair(N, qs)
    words = 2 * 4 * N                                       # one ciphertext at level 4
    buf, other = poisoned(4 * words), poisoned(8 * words)
    p, o = buf.ptr, other.ptr

    def many(keys=(p, p, p), gs=(3, 5, 127), Lk=6, level=4, k=2, group=2, nd=2, ct=p, out=o, batch=1):
        ctx.rotate_many_grouped(Lk, level, k, group, list(keys), nd, list(gs), ct, out, batch)

    def diag(keys=(p, p, p), gs=(3, 5, 127), Lk=6, level=4, k=2, group=2, nd=2, diags=p, ct=p, out=o, batch=1):
        ctx.matmul_diag_grouped(Lk, level, k, group, list(keys), nd, list(gs), diags, ct, out, batch)
    for f in (many, diag):
        for kw in (dict(ct=None, Lk=0), dict(out=None, gs=(4, 4, 4))):
            with pytest.raises(AssertionError, match="null argument"):
                f(**kw)
        with pytest.raises(AssertionError, match="key_limbs"):
            f(keys=(p, None, p), Lk=7)                      # key 0's shape ahead of the null key 1
        with pytest.raises(AssertionError, match="null argument"):
            f(keys=(p, None, p), gs=(3, 4, 4))              # a null key in the middle: its own null argument, ahead of its even g
        for g in (4, 2 * N, 2 * N + 1):
            with pytest.raises(AssertionError, match="odd and below 2N"):
                f(keys=(p, p, None), gs=(3, g, 3))          # an even g / g >= 2N at r = 1, ahead of the null key 2
        with pytest.raises(AssertionError, match="n_special"):
            f(k=5, group=0)
        with pytest.raises(AssertionError, match="group"):
            f(group=0, level=0)
        with pytest.raises(tf.UsageError, match="level"):
            f(level=5, nd=0)
        with pytest.raises(tf.UsageError, match="components"):
            f(nd=1, batch=-1)
        with pytest.raises(AssertionError, match="negative batch"):
            f(batch=-1, gs=(3, 5, 4))
        with pytest.raises(AssertionError, match="odd and below 2N"):
            f(gs=(3, 5, 4), out=p)                          # ahead of the overlap
        with pytest.raises(AssertionError, match="overlaps"):
            f(out=p + (words - 1) * 8)                      # the last word of ct
        with pytest.raises(AssertionError, match="overlaps"):
            f(out=p)
    with pytest.raises(AssertionError, match="null argument"):
        diag(diags=None, Lk=0)
    with pytest.raises(AssertionError, match="overlaps"):
        diag(diags=o + 8 * (words - 1))                     # the last word of out is the first of the diagonals
    with pytest.raises(tf.UsageError, match="level"):
        diag(keys=(), gs=(), level=5)                       # no rotation: the shape checks run once
    ctx.sync()
    assert (buf.to_numpy() == POISON).all() and (other.to_numpy() == POISON).all()


# ---- 9. on a dirty workspace -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["rotate_many", "matmul_diag"])
@pytest.mark.parametrize("N,ring,k,alpha,level", [(1 << 12, lambda N: H.chain(50, 6, N), 2, 2, 3), (1 << 15, lambda N: H.chain(40, 5, N), 2, 2, 3)])
def test_on_a_dirty_workspace(N, ring, k, alpha, level, entry):
    qs = ring(N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)      # a context of its own: the block is this call's
    batch, Lk = 3, len(qs)
    gs = [g_many(N), 2 * N - 1]
    evks = [operands(N, qs, k, alpha, level, 2, 1, seed=17 * i)[0] for i in range(len(gs))]
    devs = [prepare(ctx, Lk, e, g) for e, g in zip(evks, gs)]
    _, ct = operands(N, qs, k, alpha, level, 2, batch)
    dct = dev(ct)
    ptrs, nd = [d.ptr for d in devs], evks[0].shape[0]
    if entry == "rotate_many":
        out = tf.DeviceBuffer(len(gs) * batch * 2 * level * N)
        want = RO.rotate_many_grouped_ref(ref, level, k, alpha, evks, gs, ct).reshape(-1, 2, level, N)
        call = lambda: ctx.rotate_many_grouped(Lk, level, k, alpha, ptrs, nd, gs, dct.ptr, out.ptr, batch)
    else:
        diags = _diagonals(N, qs, level, len(gs))
        dd = dev(diags)
        out = tf.DeviceBuffer(batch * 2 * level * N)
        want = RO.matmul_diag_grouped_ref(ref, level, k, alpha, evks, gs, diags, ct)
        call = lambda: ctx.matmul_diag_grouped(Lk, level, k, alpha, ptrs, nd, gs, dd.ptr, dct.ptr, out.ptr, batch)
    on_dirty_workspace(ctx, call, out, want, moduli=qcol(qs[:level]))
    with cap(ctx, 2):
        on_dirty_workspace(ctx, call, out, want, moduli=qcol(qs[:level]))


# ---- 10. the mirror, end to end ------------------------------------------------------------------------------------------------------

def test_mirror_product_decrypts_within_the_per_limb_products_error():
    """GroupedRaised(CKKSParams, 2, 2) at N = 2^12: a 4 x 4 matrix in blocks of N / 8 slots, three rotations.  tf.matmul_diag_grouped
    decrypts to the plain product.  Tolerance: 4 x the error tf.matmul_diag makes on a ModulusRaised key set of the same ciphertext ring
    and scale, measured here, plus what one grouped key-switch step may add per rotation by the bound
    tests/test_gpu_ks_grouped.py::test_key_switch_step_is_within_the_derived_bound_with_host_supplied_noise derives,
        d N (max Q_g // 2 + 1) max|e| // P + 1 + k (1 + N max|s|)      coefficient units of the rotated ciphertext,
    with max|e|, max|s| <= 20 (6.25 sigma at sigma = 3.2: the draws behind the mirror's keys are not exposed), carried to the slots:
    a coefficient error of at most B moves a slot by at most N B / scale, and rotation r enters the sum weighted by max |diagonal r|."""
    N = 1 << 12
    qs = H.chain(40, 3, N) + H.chain(41, 2, N)
    scale = 2**40
    n = 4
    B = N // 2 // n
    rng = np.random.default_rng(33)
    x = rng.normal(0, 1, N // 2)
    Wm = rng.normal(0, 1, (n, n))
    dv = np.array([np.repeat(np.array([Wm[i, (i - k) % n] for i in range(n)]), B) for k in range(n)])
    want = Wm @ x.reshape(n, B)

    def product(params, matmul):
        kp = tf.keygen(rng, params)
        c = tf.encrypt(rng, kp, tf.ckks_encode(x.astype(complex), params.R_cipher(), scale), scale=scale)
        gks = [tf.keygen_galois(rng, kp.priv, steps=s * B) for s in range(1, n)]
        res = matmul(gks, tf.ckks_encode(dv.astype(complex), params.R_cipher(), scale), c)
        got = tf.ckks_decode(tf.decrypt(kp, res), res.scale).real.reshape(n, B)
        return float(np.abs(got - want).max()), gks, c

    grouped = tf.GroupedRaised(tf.CKKSParams(tf.NegacyclicRing(N, qs), 0, 3.2), 2, 2)
    raised = tf.ModulusRaised(tf.CKKSParams(tf.NegacyclicRing(N, qs[:4]), 0, 3.2))
    assert grouped.R_cipher().moduli == raised.R_cipher().moduli == qs[:3]
    err_g, gks, c = product(grouped, tf.matmul_diag_grouped)
    err_m, _, _ = product(raised, tf.matmul_diag)
    level, k, alpha = 3, 2, 2
    groups = KO.groups(level, alpha)
    step = len(groups) * N * (max(math.prod(qs[i] for i in G) for G in groups) // 2 + 1) * 20 // math.prod(qs[-k:]) + 1 + k * (1 + N * 20)
    bound = 4 * err_m + sum(float(np.abs(dv[r]).max()) for r in range(1, n)) * N * step / scale
    print(f"max |error|: matmul_diag_grouped {err_g:.3e}, matmul_diag (ModulusRaised) {err_m:.3e}, bound {bound:.3e}")
    assert err_g <= bound, (err_g, err_m, bound)
    # the same words as the hoisted rotations followed by the plaintext sum
    rots = tf.rotate_many_grouped(gks, c)
    for r, gk in zip(rots, gks):
        one = tf.rotate(gk, c)
        assert all(np.array_equal(a.coeffs_primal().to_numpy(), b.coeffs_primal().to_numpy()) for a, b in zip(r.cs, one.cs))
    for refused in (lambda: tf.rotate_many([gks[0]], c), lambda: gks[0].prepared()):
        with pytest.raises(tf.UsageError, match="grouped digits"):
            refused()
