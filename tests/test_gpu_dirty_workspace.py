"""Every entry point that works in a long-lived workspace, run on a dirty one.

A context owns one scratch block (tfhe_ctx::ws, handed out by ensure_ws: it grows, it is never cleared), a BFV plan a second one
(plan_ws).  The other GPU modules poison OUTPUTS; the workspace they leave in one of two kind states: fresh from the driver (zeros,
in practice) or holding the correct intermediates of the very operands being checked (the same call again, capped or in another
variant).  Here tests/dirty_ws.py fills the whole block between calls with 0x00, 0xA5 (words far above every modulus) and 0xFF (NaN to
the fp64 policy) and asks for the oracle's words each time: an accumulation that starts from scratch it never wrote, a fold step
that adds into an unwritten row, a capped run that reads a row a chunk too early all change words here and nowhere else.

The entry points are the callers of ensure_ws and plan_ws, one case per entry point and route:
  tfhe_nntt / tfhe_inntt above 2^14 (the top stages' intermediate, both lanes of a mixed ring);
  tfhe_keyswitch, tfhe_rotate, tfhe_rotate_prepared, tfhe_rotate_many, tfhe_keyswitch_window (digits, key sums, the prepared key);
  tfhe_matmul_diag, tfhe_matmul_bsgs, tfhe_matmul_bsgs_blocks, tfhe_rotate_sum, tfhe_matmul_bsgs_fold (the baby phase, the INNER sums,
  the giant results, the fold's ping-pong rows, the nested key switch in region 0);
  tfhe_mul_relin (transform images, tensor rows, parked rows);
  tfhe_encrypt, tfhe_decrypt_phase (staging rows of the composed path), tfhe_evalkey_gen (the transforms' scratch above 2^14);
  tfhe_dot_plain (gathered terms and images; the fused path's partial sums);
  tfhe_bfv_noise_max (partial maxima), tfhe_plain_encode, tfhe_plain_decode;
  tfhe_ckks_encode, tfhe_ckks_decode (the complex buffer of the scatter, the FFT passes and the closing kernel);
  tfhe_bfv_mul, tfhe_bfv_mul_relin, tfhe_bfv_expand, tfhe_bfv_contract (the plan's block and both contexts');
  tfhe_dot, tfhe_lincomb, tfhe_lincomb_many.
Some of these take no block of their own on some routes -- the fused tfhe_encrypt / tfhe_decrypt_phase at N = 2^12 .. 2^14,
tfhe_evalkey_gen up to 2^14, the plain encode / decode, the stand-alone BFV conversions, tfhe_dot and the two tfhe_lincomb -- and
would not belong here alone (dirty_ws refuses a call that leaves no workspace).  They run on a block that a one-ciphertext key
switch (presize) or the plan's own multiplication left behind: what they must not do is start to depend on it.

Operands and oracles are the other modules', by import; shapes are the smallest that select each route: one N per rung (2^10 or
2^11 composed, 2^12 / 2^13 fused, 2^14, 2^15, 2^16 -- KS_RINGS of tests/test_gpu_chunk_seams.py), an fp64-size ring and a mixed one
where the entry point forks lanes, with and without the special prime where the paths differ.  Every case runs a batch of 3 uncapped
and under set_chunk(2): the second chunk, one ciphertext, then runs over the rows the full chunk left.  The products take two inputs
(the unseeded and the seeded accumulation), five giant steps (a second output tile) and a two-step fold on every ring.  At N >= 2^14
they take one baby step and compare ciphertexts 0 and 2 only -- one of each chunk under the cap -- because the oracle's exact integer
sums are slow there (2.7 s per case at 2^16 on an 8-core CPU as it is).

Two sequences on one context close the file: small -> large -> small (the block grows and moves; the small call then runs in the
start of the large call's leftovers) and five different entry points back to back, each over the others' layout.

Out of scope: the pooled per-call workspaces above TFHE_WS_KEEP_GIB (4 GiB by default), which these shapes do not reach, and the
blocks tfhe_malloc recycles for results, which the callers own."""
from types import SimpleNamespace

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu, spec
from tests import dot_plain_oracle as DO
from tests import enc_oracle as EO
from tests import helpers as H
from tests import keygen_oracle as KO
from tests import matmul_oracle as MO
from tests import rotate_sum_oracle as RO
from tests.dirty_ws import fill, memset, on_dirty_workspace
from tests.test_gpu_bfv_folded import BATCH as BFV_BATCH, T as BFV_T, case as bfv_case
from tests.test_gpu_chunk_seams import KS_RINGS, cap, ckks_decoding_close, ckks_encoding_close, galois_elements as ks_galois, ring_of, window_oracle
from tests.test_gpu_encrypt import dev_i32, rand_ints, ring as ring_of_bits
from tests.test_gpu_keygen import gadget_of, secret_ntt
from tests.test_gpu_matmul_oracle import above, dev, galois_elements, make_diags, make_keys, mixed_policy, uniform
from tests.test_gpu_modulus_edges import _ks_ct, edge
from tests.test_gpu_mul_relin import oracle as mul_relin_oracle
from tests.test_gpu_rotate_sum import _groups

pytestmark = pytest.mark.gpu

BATCH, CAP = 3, 2                       # chunks 2, 1 under the cap: the ragged last chunk runs over the full chunk's rows
assert BFV_BATCH == BATCH


def qcol(qs):
    """the moduli against [..][limbs][N]"""
    return np.array([int(q) for q in qs], dtype=np.uint64).reshape(-1, 1)


def case(call, out, want, moduli=None, picks=None):
    return SimpleNamespace(call=call, out=out, want=want, moduli=moduli, picks=picks)


def both_caps(ctx, k, **kw):
    """the case uncapped, then under the chunk cap (the block keeps the size the uncapped run gave it)"""
    on_dirty_workspace(ctx, k.call, k.out, k.want, moduli=k.moduli, picks=k.picks, **kw)
    with cap(ctx, CAP):
        on_dirty_workspace(ctx, k.call, k.out, k.want, moduli=k.moduli, picks=k.picks, **kw)


def pair(N, qs):
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    assert ctx.psis == ref.psis
    return ctx, ref


def presize(ctx, qs):
    """a one-ciphertext key switch over the whole ring: the context owns a workspace afterwards, whatever runs next"""
    N, L = ctx.N, len(qs)
    rng = np.random.default_rng(L)
    k, c, o = dev(H.uniform_evk(rng, qs, L, N)), dev(H.rand_residues(rng, qs, (1, 2), N)), tf.DeviceBuffer(2 * L * N)
    ctx.keyswitch(L, L, False, k.ptr, L, c.ptr, 2, o.ptr, 1)
    ctx.sync()
    assert ctx.workspace()[1] > 0


# ---------------------------------------------------------------------------------------------------
# tfhe_nntt / tfhe_inntt above 2^14: the routes of run_ntt_large that go through the out-of-place intermediate -- the u64 policy at
# either size, the fp64 policy at 2^16 in place, and a mixed ring with enough rows (2^20 words) to run its two policies side by side
# ---------------------------------------------------------------------------------------------------
NTT_CASES = [(15, "60x2", 3, False), (15, "mixed", 7, False), (15, "mixed", 3, True), (16, "50x3", 3, True), (16, "60x2", 3, False),
             (16, "mixed", 4, False)]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("logn,qspec,count,inplace", NTT_CASES)
def test_large_transforms(logn, qspec, count, inplace, inverse):
    N = 1 << logn
    qs = ring_of(N, qspec)
    L = len(qs)
    ctx, ref = pair(N, qs)
    a = H.rand_residues(np.random.default_rng(logn + count), qs, (count,), N)
    want = (ref.inntt if inverse else ref.nntt)(a)
    src, out = dev(a), tf.DeviceBuffer(a.size)
    f = ctx.inntt if inverse else ctx.nntt

    def call():
        if inplace:
            tf.native.check(tf.native.lib().tfhe_memcpy_d2d(ctx.h, out.ptr, src.ptr, a.size * 8))
            f(out.ptr, out.ptr, count, L)
        else:
            f(src.ptr, out.ptr, count, L)
    both_caps(ctx, case(call, out, want, qcol(qs)))


# ---------------------------------------------------------------------------------------------------
# key switch and rotations: every route of keyswitch_impl / tfhe_rotate_many (KS_RINGS)
# ---------------------------------------------------------------------------------------------------
KS_ENTRIES = ("keyswitch-2", "keyswitch-3", "rotate", "rotate_prepared", "rotate_many", "rotate_many_prepared")


def ks_case(ctx, ref, qs, special, entry, batch=BATCH, level=None, seed=0):
    N, Lk = ctx.N, len(qs)
    level = (Lk - 1 if special else Lk) if level is None else level
    rng = np.random.default_rng(N % 997 + 7 * Lk + special + seed)
    gs = ks_galois(N)[:2]                                               # many sign wraps, the conjugation
    evks = [H.uniform_evk(rng, qs, Lk, N) for _ in gs]
    devks = [dev(e) for e in evks]
    words = batch * 2 * level * N
    mod = qcol(qs[:level])
    if entry.startswith("keyswitch"):
        polys = int(entry[-1])
        ct = H.rand_residues(rng, qs[:level], (batch, polys), N)
        dct, out = dev(ct), tf.DeviceBuffer(words)
        return case(lambda: ctx.keyswitch(Lk, level, special, devks[0].ptr, Lk, dct.ptr, polys, out.ptr, batch), out,
                    ref.keyswitch(level, special, evks[0], ct), mod)
    ct = H.rand_residues(rng, qs[:level], (batch, 2), N)
    dct = dev(ct)
    prepared = entry.endswith("prepared")
    keys = devks
    if prepared:
        keys = [tf.DeviceBuffer(e.size) for e in evks]
        for k, d, g in zip(keys, devks, gs):
            ctx.galois_key_prepare(Lk, Lk, g, d.ptr, k.ptr)
    if entry.startswith("rotate_many"):
        out = tf.DeviceBuffer(len(gs) * words)
        want = np.stack([MO.rotate(ref, level, special, e, g, ct) for e, g in zip(evks, gs)])     # [n_rot][batch][2][level][N]
        return case(lambda: ctx.rotate_many(Lk, level, special, [k.ptr for k in keys], Lk, gs, dct.ptr, out.ptr, batch, prepared=prepared),
                    out, want, mod)
    out = tf.DeviceBuffer(words)
    return case(lambda: ctx.rotate(Lk, level, special, keys[0].ptr, Lk, gs[0], dct.ptr, out.ptr, batch, prepared=prepared), out,
                MO.rotate(ref, level, special, evks[0], gs[0], ct), mod)


@pytest.mark.parametrize("entry", KS_ENTRIES)
@pytest.mark.parametrize("special", [True, False])
@pytest.mark.parametrize("N,qspec", KS_RINGS)
def test_key_switch_and_rotations(N, qspec, special, entry):
    qs = ring_of(N, qspec)
    ctx, ref = pair(N, qs)
    both_caps(ctx, ks_case(ctx, ref, qs, special, entry))


@pytest.mark.parametrize("N,bits,Lk,level,special,w", [(64, 50, 3, 3, False, 16), (2048, 50, 4, 3, True, 20), (1 << 15, 50, 2, 2, False, 20)])
def test_keyswitch_window(N, bits, Lk, level, special, w):
    qs = H.chain(bits, Lk, N)
    ctx, ref = pair(N, qs)
    rng = np.random.default_rng(N % 977 + w)
    nkey = spec.ndigits(int(np.prod([int(q) for q in qs], dtype=object)), 2 ** w)
    evk = H.uniform_evk(rng, qs, nkey, N)
    devk = dev(evk)
    for polys in (2, 3):
        ct = H.rand_residues(rng, qs[:level], (BATCH, polys), N)
        dct, out = dev(ct), tf.DeviceBuffer(BATCH * 2 * level * N)
        want = window_oracle(ref, qs, level, special, w, evk, ct)
        both_caps(ctx, case(lambda: ctx.keyswitch_window(level, w, devk.ptr, nkey, dct.ptr, polys, out.ptr, BATCH, key_limbs=Lk, special=special),
                            out, want, qcol(qs[:level])))


# ---------------------------------------------------------------------------------------------------
# the diagonal products and the fold.  Operands are run_case's of tests/test_gpu_matmul_oracle.py / test_gpu_rotate_sum.py, piece by
# piece (edge ciphertext first, keys of q - 1 and uniform keys in turn, the six kinds of diagonals, a bias of q - 1), for a batch of 3
# ---------------------------------------------------------------------------------------------------
PRODUCT_ENTRIES = ("diag", "bsgs", "blocks", "rotate_sum", "fold")


def product_case(ctx, ref, qs, special, entry, shape=(2, 5, 2), groups=(1, 1), batch=BATCH, picks=None, level=None, seed=0):
    N, Lk = ctx.N, len(qs)
    n_baby, n_giant, n_in = shape
    level = (Lk - 1 if special else Lk) if level is None else level
    cq = qs[:level]
    rng = np.random.default_rng(1000 * ctx.N.bit_length() + 10 * Lk + special + seed)
    nbg = n_baby + n_giant
    gs, _ = galois_elements(N, nbg + sum(groups), 0)
    keys = make_keys(qs, N, len(gs), rng)
    cts = [np.concatenate([_ks_ct(qs, level, 2, N, rng) for _ in range(-(-batch // 2))])[:batch] for _ in range(n_in)]
    diags = make_diags(cq, N, n_baby, n_giant, n_in, 7 + seed)
    bias = np.broadcast_to((np.array(cq, dtype=np.uint64) - 1)[:, None], (level, N)).copy()
    prep = []
    for k, g in zip(keys, gs):
        d, p = dev(k), tf.DeviceBuffer(k.size)
        ctx.galois_key_prepare(Lk, Lk, g, d.ptr, p.ptr)
        prep.append(p)
    ctx.sync()                                                          # (the plain keys' device copies go out of scope here)
    ptrs = [p.ptr for p in prep]
    fold_keys, fold_ptrs, fold_gs = _groups(keys[nbg:], groups), _groups(ptrs[nbg:], groups), _groups(gs[nbg:], groups)
    dcts, ddiags, dbias = [dev(c) for c in cts], [dev(d) for d in diags], dev(bias)
    out = tf.DeviceBuffer(batch * 2 * level * N)
    sub = cts if picks is None else [c[picks] for c in cts]
    baby, giant = (keys[:n_baby], gs[:n_baby]), (keys[n_baby:nbg], gs[n_baby:nbg])
    bp, gp = ptrs[:n_baby], ptrs[n_baby:nbg]
    if entry == "diag":                                                 # inner_0 of input 0 alone, in the NTT domain
        want = MO.matmul_diag_ref(ref, level, special, *baby, diags[0][0], sub[0])

        def call():
            ctx.matmul_diag(Lk, level, special, bp, Lk, baby[1], ddiags[0].ptr, dcts[0].ptr, out.ptr, batch)
    elif entry == "bsgs":
        want = MO.matmul_bsgs_ref(ref, level, special, *baby, *giant, diags[0], sub[0])

        def call():
            ctx.matmul_bsgs(Lk, level, special, bp, baby[1], gp, giant[1], Lk, ddiags[0].ptr, dcts[0].ptr, out.ptr, batch)
    elif entry == "blocks":
        want = MO.matmul_bsgs_blocks_ref(ref, level, special, *baby, *giant, diags, sub, bias)

        def call():
            ctx.matmul_bsgs_blocks(Lk, level, special, bp, baby[1], gp, giant[1], Lk, [d.ptr for d in ddiags], [c.ptr for c in dcts], dbias.ptr,
                                   out.ptr, batch)
    elif entry == "rotate_sum":
        want = RO.rotate_sum_ref(ref, level, special, fold_keys, fold_gs, sub[0])

        def call():
            ctx.rotate_sum(Lk, level, special, fold_ptrs, fold_gs, Lk, dcts[0].ptr, out.ptr, batch)
    else:
        want = RO.matmul_bsgs_fold_ref(ref, level, special, *baby, *giant, diags, sub, fold_keys, fold_gs, bias)

        def call():
            ctx.matmul_bsgs_fold(Lk, level, special, bp, baby[1], gp, giant[1], Lk, [d.ptr for d in ddiags], [c.ptr for c in dcts], fold_ptrs,
                                 fold_gs, dbias.ptr, out.ptr, batch)
    return case(call, out, want, qcol(cq), picks)


def _large_mixed(N, special):
    return edge("fp-top", 1, N) + edge("top62", 2, N)


# name, ring, log2 N, special, (n_baby, n_giant, n_in), picks.  Everywhere two inputs and five giant steps (output tiles of 4 + 2 sums).  From
# 2^14 on the oracle's exact integer sums set the rest: one baby step, and ciphertexts 0 and 2 (one of each chunk under the cap) compared
PRODUCT_RINGS = [("composed", above(40, 3), 10, sp, (2, 5, 2), None) for sp in (True, False)]
PRODUCT_RINGS += [("fp", uniform("fp-top", 3), 12, sp, (2, 5, 2), None) for sp in (True, False)]
PRODUCT_RINGS += [("mixed", mixed_policy, 12, sp, (2, 5, 2), None) for sp in (True, False)]
PRODUCT_RINGS += [("lift-fused", uniform("fp-top", 3), 14, True, (1, 5, 2), [0, 2]),
                  ("large-fp", uniform("fp-top", 2), 15, True, (1, 5, 2), [0, 2]), ("large-fp", uniform("fp-top", 2), 15, False, (1, 5, 2), [0, 2]),
                  ("large-mixed", _large_mixed, 16, True, (1, 5, 2), [0, 2])]


@pytest.mark.parametrize("entry", PRODUCT_ENTRIES)
@pytest.mark.parametrize("name,ring,logn,special,shape,picks",
                         [pytest.param(*r, id=f"{r[0]}-logn{r[2]}-{'special' if r[3] else 'plain'}") for r in PRODUCT_RINGS])
def test_diagonal_products_and_fold(name, ring, logn, special, shape, picks, entry):
    N = 1 << logn
    qs = ring(N, special)
    ctx, ref = pair(N, qs)
    both_caps(ctx, product_case(ctx, ref, qs, special, entry, shape=shape, picks=picks))


# ---------------------------------------------------------------------------------------------------
# tfhe_mul_relin: composed below the fused sizes, the fused product on an fp64-size ring, the packed kernels on a mixed ring, 2^14,
# and composed again above
# ---------------------------------------------------------------------------------------------------
def mul_relin_case(ctx, ref, qs, special, square, rescale, batch=BATCH, seed=0):
    N, Lk = ctx.N, len(qs)
    level = Lk - 1 if special else Lk
    rng = np.random.default_rng(N % 971 + special + 2 * square + seed)
    evk = H.uniform_evk(rng, qs, Lk, N)
    c1 = H.rand_residues(rng, qs[:level], (batch, 2), N)
    c2 = c1 if square else H.rand_residues(rng, qs[:level], (batch, 2), N)
    devk, d1 = dev(evk), dev(c1)
    d2 = d1 if square else dev(c2)
    lo = level - rescale
    out = tf.DeviceBuffer(batch * 2 * lo * N)
    return case(lambda: ctx.mul_relin(Lk, level, special, devk.ptr, Lk, d1.ptr, d2.ptr, out.ptr, batch, rescale=bool(rescale)), out,
                mul_relin_oracle(ref, level, special, evk, c1, c2, 0, rescale), qcol(qs[:lo]))


@pytest.mark.parametrize("square,rescale", [(False, 1), (True, 0)])
@pytest.mark.parametrize("N,qspec,special", [(1 << 11, "40x3", False), (1 << 12, "40x3", False), (1 << 13, "mixed", True), (1 << 14, "50x4", True),
                                             (1 << 15, "40x4", True), (1 << 16, "mixed", True)])
def test_mul_relin(N, qspec, special, square, rescale):
    qs = ring_of(N, qspec)
    ctx, ref = pair(N, qs)
    both_caps(ctx, mul_relin_case(ctx, ref, qs, special, square, rescale))


# ---------------------------------------------------------------------------------------------------
# tfhe_encrypt / tfhe_decrypt_phase / tfhe_evalkey_gen.  The composed paths (N < 2^12, N >= 2^15, variant 1) stage their rows in the
# workspace; the fused kernels take none and run on a key switch's leftovers
# ---------------------------------------------------------------------------------------------------
ENC_SIZES = [(11, (50, 60)), (12, (50, 50)), (12, (60, 40, 60)), (14, (60, 50)), (15, (50, 60)), (16, (60, 50))]


def encrypt_case(ctx, ref, qs, batch=BATCH, seed=0):
    N, L = ctx.N, len(qs)
    rng = np.random.default_rng(400 + N % 991 + seed)
    pk, rand, msg = H.rand_residues(rng, qs, (2,), N), rand_ints(rng, batch, N), H.rand_residues(rng, qs, (batch,), N)
    dpk, drand, dmsg, out = dev(pk), dev_i32(rand), dev(msg), tf.DeviceBuffer(batch * 2 * L * N)
    return case(lambda: ctx.encrypt(L, L, dpk.ptr, out.ptr, batch, msg=dmsg.ptr, rand=drand.ptr, mult_e=65537), out,
                EO.encrypt_ref(ref, pk, rand, 65537, msg), qcol(qs))


def decrypt_case(ctx, ref, qs, polys, ntt_in, batch=BATCH):
    N, L = ctx.N, len(qs)
    rng = np.random.default_rng(500 + N % 991 + polys)
    s, ct = H.rand_residues(rng, qs, (), N), H.rand_residues(rng, qs, (batch, polys), N)
    ds, dct, out = dev(s), dev(ct), tf.DeviceBuffer(batch * L * N)
    return case(lambda: ctx.decrypt_phase(L, L, ds.ptr, dct.ptr, polys, out.ptr, batch, ntt_in=ntt_in), out, EO.decrypt_ref(ref, s, ct, ntt_in),
                qcol(qs))


def _variants(ctx, logn, k):
    """a fused size: the fused kernels, then the composed path of variant 1 at the same size"""
    for variant in ((0, 1) if 12 <= logn <= 14 else (0,)):
        ctx.set_ntt_variant(variant)
        try:
            both_caps(ctx, k)
        finally:
            ctx.set_ntt_variant(0)


@pytest.mark.parametrize("logn,bits", ENC_SIZES)
def test_encrypt(logn, bits):
    N = 1 << logn
    qs = ring_of_bits(N, bits)
    ctx, ref = pair(N, qs)
    if 12 <= logn <= 14:
        presize(ctx, qs)
    _variants(ctx, logn, encrypt_case(ctx, ref, qs))


@pytest.mark.parametrize("polys,ntt_in", [(3, False), (2, True)])
@pytest.mark.parametrize("logn,bits", ENC_SIZES)
def test_decrypt_phase(logn, bits, polys, ntt_in):
    N = 1 << logn
    qs = ring_of_bits(N, bits)
    ctx, ref = pair(N, qs)
    if 12 <= logn <= 14:
        presize(ctx, qs)
    _variants(ctx, logn, decrypt_case(ctx, ref, qs, polys, ntt_in))


@pytest.mark.parametrize("logn,bits", [(11, (50, 60, 50)), (12, (60, 50, 50)), (14, (60, 50, 50)), (15, (60, 50, 50)), (16, (60, 50, 50))])
def test_evalkey_gen(logn, bits):
    """two keys (the relinearisation key and a Galois key) of three digits each: six components, chunks of two under the cap"""
    N = 1 << logn
    qs = ring_of_bits(N, bits)
    L = D = len(qs)
    ctx, ref = pair(N, qs)
    rng = np.random.default_rng(7000 + logn)
    s, gadget, galois = secret_ntt(ref, rng), gadget_of("rns", qs), [0, 3]
    K = len(galois)
    mask = H.rand_residues(rng, qs, (K, D), N)
    noise = np.rint(rng.normal(0.0, 3.2, size=(K, D, N))).astype(np.int64)
    want = KO.evalkey_ref(ref, s, mask, noise, 65537, gadget=gadget, galois=galois)
    ds, dmask, dnoise = dev(s), dev(mask), dev_i32(noise)
    bufs = [tf.DeviceBuffer(D * 2 * L * N) for _ in range(K)]
    presize(ctx, qs)                                                    # (up to 2^14 the call takes no block; above, the transforms' scratch)

    def call():
        ctx.evalkey_gen(L, ds.ptr, [b.ptr for b in bufs], D, gadget=gadget, galois_elements=galois, mask_rand=dmask.ptr, noise_rand=dnoise.ptr,
                        mult_e=65537)
    both_caps(ctx, case(call, bufs, [want[k] for k in range(K)], qcol(qs)))


# ---------------------------------------------------------------------------------------------------
# tfhe_dot_plain: the composed path's gathered terms and images (below and above the fused sizes), the fused path's partial sums (more
# than four terms over a few items), one and two policies.  Dense views, shared and per-item plaintexts in turn, the last term
# already transformed.  dot_split cuts 6 terms into two ranges (one row of partial sums per item) and 13 into four
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,bits,n_terms", [(11, (50, 60), 3), (15, (50, 60), 3), (16, (50, 60), 3), (12, (50, 50), 13), (12, (60, 40, 60), 6),
                                               (14, (60, 50), 6)])
def test_dot_plain(logn, bits, n_terms):
    N = 1 << logn
    qs = ring_of_bits(N, bits)
    L = len(qs)
    ctx, ref = pair(N, qs)
    rng = np.random.default_rng(logn + n_terms)
    a = [H.rand_residues(rng, qs, (BATCH,), N) for _ in range(n_terms)]
    b = [H.rand_residues(rng, qs, (BATCH,) if k % 2 else (), N) for k in range(n_terms)]
    a_ntt = [0] * (n_terms - 1) + [1]
    want = DO.dot_plain_ref(ref, None, a, a_ntt, b)
    da, db, out = [dev(x) for x in a], [dev(x) for x in b], tf.DeviceBuffer(BATCH * L * N)
    row = L * N

    def call():
        ctx.dot_plain(None, [(d.ptr, row, f) for d, f in zip(da, a_ntt)], [(d.ptr, row if k % 2 else 0) for k, d in enumerate(db)], (out.ptr, row),
                      BATCH, L)
    both_caps(ctx, case(call, out, want, qcol(qs)))


# ---------------------------------------------------------------------------------------------------
# tfhe_ckks_encode / tfhe_ckks_decode: scatter, FFT passes and the closing kernel all work in one complex buffer in the workspace.  A float
# path: the oracle bounds the words (the tolerances of tests/test_gpu_chunk_seams.py) and does not fix them, so every fill is judged
# against the oracle AND must give the bits of the first -- the same operations on the same inputs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["encode", "decode"])
@pytest.mark.parametrize("N", [64, 4096])
def test_ckks_codec(N, entry):
    L, scale = 2, 2 ** 40
    qs = H.chain(50, L, N)
    ring = spec.Ring(N, qs)
    ctx = tf.Context(N, qs)
    rng = np.random.default_rng(N + 19)
    slots = rng.normal(size=(BATCH, N // 2)) * 3 + 1j * rng.normal(size=(BATCH, N // 2))
    mant, exp2 = tf.she.scale_parts(scale)
    dz, denc, dslots = dev(np.ascontiguousarray(slots).view(np.uint64)), tf.DeviceBuffer(BATCH * L * N), tf.DeviceBuffer(BATCH * N)
    seen = []

    def same_bits(words):
        seen.append(words.copy())
        assert np.array_equal(words, seen[0]), "the words changed with the fill"
    if entry == "encode":
        def judge(k, words, want, byte):
            for b in range(BATCH):
                ckks_encoding_close(slots[b], words.reshape(BATCH, L, N)[b], ring, scale, (hex(byte), b))
            same_bits(words)
        k = case(lambda: ctx.ckks_encode(L, mant, exp2, dz.ptr, denc.ptr, BATCH), denc, None)
    else:
        ctx.ckks_encode(L, mant, exp2, dz.ptr, denc.ptr, BATCH)        # the input of the decoding, itself judged in the other case
        enc = [[list(map(int, l)) for l in e] for e in denc.to_numpy((BATCH, L, N))]

        def judge(k, words, want, byte):
            for b in range(BATCH):
                ckks_decoding_close(slots[b], enc[b], words.view(np.complex128).reshape(BATCH, N // 2)[b], ring, scale, (hex(byte), b))
            same_bits(words)
        k = case(lambda: ctx.ckks_decode(L, mant, exp2, denc.ptr, dslots.ptr, BATCH), dslots, None)
    both_caps(ctx, k, compare=judge)


# ---------------------------------------------------------------------------------------------------
# the plaintext codec: tfhe_bfv_noise_max reduces through partial maxima in the workspace; encode and decode take none
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["noise_max", "decode-bfv", "decode-bgv", "encode-bfv", "encode-bgv"])
def test_plain_codec(entry):
    N, t, L = 1 << 12, 65537, 3
    qs = H.chain(50, L, N)
    ctx = tf.Context(N, qs)
    plan = tf.PlainPlan(ctx, t)
    ring = spec.Ring(N, qs, [1] * L)
    delta = ring.Q // t
    rng = np.random.default_rng(4096)
    res = H.rand_residues(rng, qs, (BATCH,), N)
    m = rng.integers(0, 2 ** 63, size=(BATCH, N), dtype=np.uint64)
    src, dm = dev(res), dev(m)
    rows = [[[int(v) for v in l] for l in res[b]] for b in range(BATCH)]
    scheme = tf.native.PLAIN_BGV if entry.endswith("bgv") else tf.native.PLAIN_BFV
    try:
        if entry == "noise_max":
            out = tf.DeviceBuffer(BATCH * plan.delta_words)
            worst = [max((delta - x % delta) if x % delta > delta // 2 else x % delta for x in spec.poly_to_ints(r, ring)) for r in rows]
            want = np.array([[(w >> (64 * i)) & (2 ** 64 - 1) for i in range(plan.delta_words)] for w in worst], dtype=np.uint64)
            k = case(lambda: plan.noise_max(src.ptr, out.ptr, BATCH), out, want)
        elif entry.startswith("decode"):
            presize(ctx, qs)
            out = tf.DeviceBuffer(BATCH * N)
            decode = spec.bgv_decode if entry.endswith("bgv") else spec.bfv_decode
            want = np.array([decode(r, ring, t) for r in rows], dtype=np.uint64)
            k = case(lambda: plan.decode(scheme, src.ptr, out.ptr, BATCH), out, want, np.uint64(t))
        else:
            presize(ctx, qs)
            out = tf.DeviceBuffer(BATCH * L * N)
            ints = [[int(v) for v in m[b]] for b in range(BATCH)]
            want = np.array([spec.bfv_encode(x, ring, t) if scheme == tf.native.PLAIN_BFV else [[v % t % q for v in x] for q in qs] for x in ints],
                            dtype=np.uint64)
            k = case(lambda: plan.encode(scheme, dm.ptr, out.ptr, BATCH), out, want, qcol(qs))
        both_caps(ctx, k)
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------
# BFV: the plan's block (expanded rows, tensor rows, the contraction's output, the fused core's scratch rows) and the contexts' (the
# prepared key, the key switch, the transforms above 2^14).  Inputs and oracle words are test_gpu_bfv_folded.case's, computed once per
# shape: below the fused sizes, the folded route at (2, 3) and (8, 9) limbs, above the fused sizes; the general kernels (variant 1);
# the two rings in two contexts.  The stand-alone conversions take no block: they run on the one a multiplication left
# ---------------------------------------------------------------------------------------------------
BFV_CASES = [(2048, 2, 3, 0, False), (4096, 2, 3, 0, False), (4096, 2, 3, 1, False), (4096, 2, 3, 0, True), (16384, 8, 9, 0, False),
             (32768, 2, 3, 0, False)]


@pytest.mark.parametrize("entry", ["mul", "mul_relin", "expand", "contract"])
@pytest.mark.parametrize("N,ns,np_,variant,two", BFV_CASES)
def test_bfv(N, ns, np_, variant, two, entry):
    K = bfv_case(N, ns, np_)
    nb = ns + np_
    if two:
        small, big = tf.Context(N, K["qs"]), tf.Context(N, K["ch"])
        plan, owners = tf.BfvPlan(small, big, BFV_T), (small, big)
    else:
        small = tf.Context(N, K["ch"])
        plan, owners = tf.BfvPlan(small, small, BFV_T, idx_s=list(range(ns))), (small,)
    plan.set_variant(variant)
    d1, d2, dk = dev(K["c1"]), dev(K["c2"]), dev(K["evk"])
    relin_out = tf.DeviceBuffer(BATCH * 2 * ns * N)

    def relin():
        plan.mul_relin(dk.ptr, ns, d1.ptr, d2.ptr, relin_out.ptr, BATCH)
    if entry == "mul":
        out = tf.DeviceBuffer(BATCH * 3 * ns * N)
        k = case(lambda: plan.mul(d1.ptr, d2.ptr, out.ptr, BATCH), out, K["prod"], qcol(K["qs"]))
    elif entry == "mul_relin":
        k = case(relin, relin_out, K["relin"], qcol(K["qs"]))
    elif entry == "expand":
        da, out = dev(K["a"]), tf.DeviceBuffer(K["expand"].size)
        k = case(lambda: plan.expand(da.ptr, out.ptr, len(K["a"])), out, K["expand"], qcol(K["ch"]))
    else:
        dy, out = dev(K["y"]), tf.DeviceBuffer(K["contract"].size)
        k = case(lambda: plan.contract(dy.ptr, out.ptr, len(K["y"])), out, K["contract"], qcol(K["qs"]))
    assert K["expand"].shape[1] == nb
    try:
        relin()                                                         # the plan and its contexts own their blocks from here on
        for chunk in (0, CAP):                                          # the plan's chunk and the contexts' (the nested key switch, the transforms)
            plan.set_chunk(chunk)
            for o in owners:
                o.set_chunk(chunk)
            on_dirty_workspace(plan, k.call, k.out, k.want, moduli=k.moduli, also=owners)
    finally:
        for o in owners:
            o.set_chunk(0)
        plan.close()


# ---------------------------------------------------------------------------------------------------
# tfhe_dot, tfhe_lincomb, tfhe_lincomb_many: one term count on each side of TFHE_DOT_MAX = 64 (tfhe_dot's second launch accumulates
# onto dst; the other two refuse a 65th term).  They take no workspace: they run on a key switch's
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["dot", "lincomb", "lincomb_many"])
@pytest.mark.parametrize("terms", [64, 65])
def test_sums(terms, entry):
    N = 1 << 10
    qs = edge("top61", 2, N)
    L = len(qs)
    ctx = tf.Context(N, qs)
    rng = np.random.default_rng(terms)
    ops = [H.rand_residues(rng, qs, (BATCH,), N) for _ in range(terms)]
    dops = [dev(x) for x in ops]
    ptrs = [d.ptr for d in dops]
    A = [x.astype(object) for x in ops]
    qv = np.array(qs, dtype=object)[None, :, None]
    scal = [[[int(rng.integers(0, q)) if (k + o) % 2 else q - 1 for q in qs] for k in range(terms)] for o in range(2)]
    lin = [(sum(x * np.array(s, dtype=object)[None, :, None] for x, s in zip(A, scal[o])) % qv).astype(np.uint64) for o in range(2)]
    outs = [tf.DeviceBuffer(BATCH * L * N) for _ in range(2)]
    presize(ctx, qs)
    if entry == "dot":
        want = (sum(x * y for x, y in zip(A, A[::-1])) % qv).astype(np.uint64)
        k = case(lambda: ctx.dot(None, ptrs, ptrs[::-1], outs[0].ptr, BATCH, L), outs[0], want, qcol(qs))
    elif entry == "lincomb":
        k = case(lambda: ctx.lincomb(scal[0], ptrs, outs[0].ptr, BATCH, L), outs[0], lin[0], qcol(qs))
    else:
        k = case(lambda: ctx.lincomb_many(scal, ptrs, [o.ptr for o in outs], BATCH, L), outs, lin, qcol(qs))
    if terms > 64 and entry != "dot":
        with pytest.raises(NotImplementedError, match="at most 64"):
            k.call()
        return
    both_caps(ctx, k)


# ---------------------------------------------------------------------------------------------------
# sequences on one context
# ---------------------------------------------------------------------------------------------------
def _run(k):
    k.call()


def _check(k, what):
    got = k.out.to_numpy().reshape((-1,) + k.want.shape[1:])
    got = got if k.picks is None else got[k.picks]
    assert np.array_equal(got, k.want), what
    assert (got < k.moduli).all(), what


@pytest.mark.parametrize("N,qspec", [(1 << 10, "40x4"), (1 << 13, "50x4"), (1 << 15, "40x4")])
def test_small_large_small(N, qspec):
    """a key switch of one ciphertext at level 2, one of six at level 3, the first again: the block grows (the old one is freed) and
    the small call then works in the start of what the large one left -- as it left it, and filled with 0xA5 and 0xFF"""
    qs = ring_of(N, qspec)
    ctx, ref = pair(N, qs)
    small = ks_case(ctx, ref, qs, True, "keyswitch-3", batch=1, level=2, seed=1)
    large = ks_case(ctx, ref, qs, True, "rotate_many_prepared", batch=6, seed=2)
    _run(small)
    _check(small, "fresh")
    first = ctx.workspace()
    for byte in (None, 0xA5, 0xFF):
        _run(large)
        _check(large, ("large", byte))
        grown = ctx.workspace()
        assert grown[1] > first[1] > 0
        if byte is not None:
            assert fill(ctx, byte) == grown
        memset(ctx, small.out.ptr, 0x5A, small.out.n * 8)
        _run(small)
        _check(small, ("small after large", byte))
        assert ctx.workspace() == grown                                 # (a block is never given back for a smaller one)


@pytest.mark.parametrize("N,qspec", [(1 << 12, "mixed"), (1 << 13, "50x4")])
def test_entry_points_back_to_back(N, qspec):
    """tfhe_mul_relin -> tfhe_rotate_many -> tfhe_matmul_bsgs_blocks -> tfhe_encrypt -> tfhe_keyswitch with nothing in between, twice
    over (the second round's product runs on the key switch's leftovers), then once more from a block of 0xFF: every call works over
    the layout of the one before it"""
    qs = ring_of(N, qspec)
    ctx, ref = pair(N, qs)
    ref_low = ref_cpu.RefCtx(N, qs[:-1], ref.psis[:-1])                 # encryption over the ciphertext ring
    chain = [("mul_relin", mul_relin_case(ctx, ref, qs, True, False, 1)),
             ("rotate_many", ks_case(ctx, ref, qs, True, "rotate_many_prepared")),
             ("blocks", product_case(ctx, ref, qs, True, "blocks", shape=(2, 5, 2))),
             ("encrypt", encrypt_case(ctx, ref_low, qs[:-1])),
             ("keyswitch", ks_case(ctx, ref, qs, True, "keyswitch-3", batch=1, seed=3))]
    for rnd in (0, 1, "0xFF"):
        if rnd == "0xFF":
            fill(ctx, 0xFF)
        for _, k in chain:
            memset(ctx, k.out.ptr, 0x5A, k.out.n * 8)
        for _, k in chain:
            _run(k)
        for name, k in chain:
            _check(k, (name, "round", rnd))
