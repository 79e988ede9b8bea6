"""Every batched entry point across its internal chunk boundary.

The chunked entry points split their batch on the host: pointer offsets from b0, a workspace carved by `chunk` and filled at `nb`
strides, state prepared once and reused by later chunks, Philox counters offset by b0, routes chosen on the whole batch and run per
chunk.  tfhe_ctx_set_chunk (Context.set_chunk) caps the chunk, so a batch of 19 crosses two or three boundaries with a ragged last
chunk at every N.  Each case applies two checks:
  (a) the oracle (oracle/ref_cpu, oracle/spec, tests/enc_oracle) on ciphertexts that straddle every boundary and on both ends;
  (b) the capped call against the uncapped one, bit for bit over the whole batch (ciphertexts are independent).
Inputs are a fresh uniform row per ciphertext (a wrong offset never lands on an identical ciphertext).  The last section runs the
default chunk sizes themselves (512, 4096, 32768, 65535) where that is cheap."""
import contextlib

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu, spec
from tests import enc_oracle as EO
from tests import helpers as H
from tests.matmul_oracle import rotate as ref_rotate
from tests.test_gpu_encrypt import check_decrypt, check_encrypt, context as enc_context, dev_i32, rand_ints
from tests.test_gpu_mul_relin import oracle as mul_relin_oracle

pytestmark = pytest.mark.gpu

BATCH, CAPS = 19, (8, 5)                    # chunks 8, 8, 3 (a last chunk below 8) and 5, 5, 5, 4
PICKS = [0, 4, 5, 7, 8, 15, 16, 18]         # both sides of every boundary of either cap, and the ends
BATCH16, CAPS16 = 11, (8, 3)                # N = 2^16: chunks 8, 3 and 3, 3, 3, 2
PICKS16 = [0, 2, 3, 7, 8, 9, 10]


def dev(a):
    return tf.DeviceBuffer.from_numpy(a)


@contextlib.contextmanager
def cap(ctx, n):
    ctx.set_chunk(n)
    try:
        yield
    finally:
        ctx.set_chunk(0)


def poison(ctx, *bufs):
    """overwrite output buffers before a call: a row the call does not write must not keep the right words of an earlier run"""
    for b in bufs:
        tf.native.check(tf.native.lib().tfhe_memset(ctx.h, b.ptr, 0xA5, b.n * 8))


def same_at_every_cap(ctx, call, out, caps=CAPS):
    """call() -> the words it left in `out`; the words at cap 0, after every capped run (into the poisoned buffer) has been
    compared with them"""
    poison(ctx, out)
    base = call()
    for n in caps:
        poison(ctx, out)
        with cap(ctx, n):
            got = call()
        assert got.dtype == base.dtype and np.array_equal(got, base), ("cap", n)
    return base


def ring_of(N, spec_):
    if spec_ == "mixed":                    # 60 + 40 x 3 + 60: the reference's CKKS ring shape (tests/test_gpu_lanes.py)
        return H.chain(60, 1, N) + H.chain(40, 3, N) + [H.chain(60, 2, N)[1]]
    bits, n = spec_.split("x")
    return H.chain(int(bits), int(n), N)


def sizes(N):
    return (BATCH16, CAPS16, PICKS16) if N == 1 << 16 else (BATCH, CAPS, PICKS)


def galois_elements(N):
    return [pow(3, N // 2 + 3, 2 * N), 2 * N - 1, 3]   # many sign wraps, the conjugation, one step


# every route of keyswitch_impl / tfhe_rotate_many: generic, k_ks_fused<13>, the two-launch fused form at 2^14, the sub-block fused
# kernel at 2^15 (ArithFpS at 40 bits, ArithFp at 50), the three-kernel path with two lanes at 2^16
KS_RINGS = [(1 << 10, "40x4"), (1 << 13, "50x4"), (1 << 14, "50x4"), (1 << 15, "40x4"), (1 << 15, "50x3"), (1 << 16, "mixed")]


# ---------------------------------------------------------------------------------------------------
# key switch and rotations
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("special", [True, False])
@pytest.mark.parametrize("N,qspec", KS_RINGS)
def test_keyswitch_across_chunks(N, qspec, special):
    qs = ring_of(N, qspec)
    Lk = len(qs)
    level = Lk - 1 if special else Lk
    batch, caps, picks = sizes(N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(N % 997 + 2 * len(qspec) + special)
    evk = H.uniform_evk(rng, qs, Lk, N)
    devk = dev(evk)
    out = tf.DeviceBuffer(batch * 2 * level * N)
    for polys in (2, 3):
        ct = H.rand_residues(rng, qs[:level], (batch, polys), N)
        dct = dev(ct)

        def call():
            ctx.keyswitch(Lk, level, special, devk.ptr, Lk, dct.ptr, polys, out.ptr, batch)
            return out.to_numpy((batch, 2, level, N))
        got = same_at_every_cap(ctx, call, out, caps)
        assert np.array_equal(got[picks], ref.keyswitch(level, special, evk, ct[picks])), polys


@pytest.mark.parametrize("special", [True, False])
@pytest.mark.parametrize("N,qspec", KS_RINGS)
def test_rotations_across_chunks(N, qspec, special):
    """tfhe_rotate, tfhe_rotate_prepared and tfhe_rotate_many (plain and prepared keys): the key prepared once outside the chunk
    loop (k_evk_to_f64 with the rotation folded in, the k_ntt_perm copy of the key), the rotation finished in the tail on a last chunk
    below 8 ciphertexts, and the [n_rot][batch] layout of tfhe_rotate_many -- got[r, b] is rotation r of ciphertext b."""
    qs = ring_of(N, qspec)
    Lk = len(qs)
    level = Lk - 1 if special else Lk
    batch, caps, picks = sizes(N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(N % 991 + 3 * len(qspec) + special)
    gs = galois_elements(N)
    evks = [H.uniform_evk(rng, qs, Lk, N) for _ in gs]
    devks = [dev(e) for e in evks]
    prep = [tf.DeviceBuffer(e.size) for e in evks]
    for r, g in enumerate(gs):
        ctx.galois_key_prepare(Lk, Lk, g, devks[r].ptr, prep[r].ptr)
    ct = H.rand_residues(rng, qs[:level], (batch, 2), N)
    dct = dev(ct)
    one, many = tf.DeviceBuffer(batch * 2 * level * N), tf.DeviceBuffer(len(gs) * batch * 2 * level * N)
    single = []
    for r, g in enumerate(gs):

        def rot(prepared, r=r, g=g):
            ctx.rotate(Lk, level, special, (prep if prepared else devks)[r].ptr, Lk, g, dct.ptr, one.ptr, batch, prepared=prepared)
            return one.to_numpy((batch, 2, level, N))
        got = same_at_every_cap(ctx, lambda: rot(False), one, caps)
        assert np.array_equal(got[picks], ref_rotate(ref, level, special, evks[r], g, ct[picks])), ("oracle", g)
        assert np.array_equal(same_at_every_cap(ctx, lambda: rot(True), one, caps), got), ("prepared", g)
        single.append(got)
    for prepared in (False, True):

        def rot_many():
            ctx.rotate_many(Lk, level, special, [d.ptr for d in (prep if prepared else devks)], Lk, gs, dct.ptr, many.ptr, batch,
                            prepared=prepared)
            return many.to_numpy((len(gs), batch, 2, level, N))
        got = same_at_every_cap(ctx, rot_many, many, caps)
        for r in range(len(gs)):
            for b in range(batch):
                assert np.array_equal(got[r, b], single[r][b]), ("rotate_many", prepared, r, b)


# ---------------------------------------------------------------------------------------------------
# tfhe_matmul_diag: the evaluation-domain form (special prime) and the coefficient tail
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("special", [True, False])
@pytest.mark.parametrize("N,qspec", [(1 << 10, "40x4"), (1 << 14, "50x4"), (1 << 16, "mixed")])
def test_matmul_diag_across_chunks(N, qspec, special):
    qs = ring_of(N, qspec)
    Lk = len(qs)
    level = Lk - 1 if special else Lk
    batch, caps, picks = sizes(N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(N % 983 + 5 * len(qspec) + special)
    gs = galois_elements(N)
    R = len(gs)
    evks = [H.uniform_evk(rng, qs, Lk, N) for _ in gs]
    prep = [tf.DeviceBuffer(e.size) for e in evks]
    for r, g in enumerate(gs):
        ctx.galois_key_prepare(Lk, Lk, g, dev(evks[r]).ptr, prep[r].ptr)
    keys = [p.ptr for p in prep]
    diags = H.rand_residues(rng, qs[:level], (R + 1,), N)               # NTT domain, shared by the batch
    ddiag = dev(diags)
    ct = H.rand_residues(rng, qs[:level], (batch, 2), N)
    dct = dev(ct)
    words = batch * 2 * level * N
    out = tf.DeviceBuffer(words)

    def call():
        ctx.matmul_diag(Lk, level, special, keys, Lk, gs, ddiag.ptr, dct.ptr, out.ptr, batch)
        return out.to_numpy((batch, 2, level, N))
    got = same_at_every_cap(ctx, call, out, caps)
    # rotate_many -> nntt -> dot through the public entry points at the default chunk
    rots, x, chain = tf.DeviceBuffer(R * words), tf.DeviceBuffer(words), tf.DeviceBuffer(words)
    ctx.rotate_many(Lk, level, special, keys, Lk, gs, dct.ptr, rots.ptr, batch, prepared=True)
    ctx.nntt(rots.ptr, rots.ptr, R * batch * 2, level)
    ctx.nntt(dct.ptr, x.ptr, batch * 2, level)
    bd = [tf.DeviceBuffer(words) for _ in range(R + 1)]
    for r in range(R + 1):
        tf.native.check(tf.native.lib().tfhe_broadcast_poly(ctx.h, bd[r].ptr, ddiag.ptr + r * level * N * 8, level * N, batch * 2))
    ctx.dot(None, [x.ptr] + [rots.ptr + r * words * 8 for r in range(R)], [b.ptr for b in bd], chain.ptr, batch * 2, level)
    assert np.array_equal(got, chain.to_numpy((batch, 2, level, N)))
    # the oracle on the picks: diag_0 . NTT(c) + sum_r diag_{r+1} . NTT(rotate(gk_r, c))
    idx = range(level)
    sub = ct[picks]
    terms = [sub] + [ref_rotate(ref, level, special, evks[r], g, sub) for r, g in enumerate(gs)]
    want = None
    for r, term in enumerate(terms):
        img = ref.nntt(term.reshape(-1, level, N), idx=idx)
        prod = ref.pointwise("mul", img, np.ascontiguousarray(np.broadcast_to(diags[r], img.shape)), idx=idx)
        want = prod if want is None else ref.pointwise("add", want, prod, idx=idx)
    assert np.array_equal(got[picks], want.reshape(sub.shape))


# ---------------------------------------------------------------------------------------------------
# tfhe_keyswitch_window
# ---------------------------------------------------------------------------------------------------
def window_oracle(ref, qs, level, special, w, evk, ct):
    """rlwe_she.jl:330-347 (under modulusraising.jl:35-49 with the special prime) from the oracle's parts: the base-2^w digits of
    the integer c[end] (exact CRT), the transforms, limb-wise products and the modswitch of oracle/ref_cpu.
    evk [n][2][Lk][N] NTT domain, ct [n][polys][level][N] -> [n][2][level][N]"""
    N, Lk = ref.N, len(qs)
    which = list(range(level)) + ([Lk - 1] if special else [])
    cq = [int(q) for q in qs[:level]]
    Q = int(np.prod(cq, dtype=object))
    need = spec.ndigits(Q, 2 ** w)
    crt = [(Q // q) * pow(Q // q, -1, q) for q in cq]                   # convert(Integer, ::CRTEncoded), crt.jl:98-112
    n, polys = ct.shape[:2]
    nw = len(which)
    ints = sum(ct[:, -1, l].astype(object) * crt[l] for l in range(level)) % Q          # [n][N]
    digs = np.stack([((ints >> (i * w)) & ((1 << w) - 1)).astype(np.uint64) for i in range(need)], axis=1)   # [n][need][N]
    digs = np.ascontiguousarray(np.broadcast_to(digs[:, :, None, :], (n, need, nw, N)))  # every digit is below 2^w < q
    dimg = ref.nntt(digs.reshape(-1, nw, N), idx=which).reshape(n, need, nw, N)
    out = np.empty((n, 2, level, N), dtype=np.uint64)
    for s in range(2):                                                  # component 0 takes the masked rows, 1 the mask
        key = np.ascontiguousarray(np.broadcast_to(evk[:need, 1 - s][:, which][None], (n, need, nw, N)))
        prod = ref.pointwise("mul", key.reshape(-1, nw, N), dimg.reshape(-1, nw, N), idx=which).reshape(n, need, nw, N)
        acc = np.ascontiguousarray(prod[:, 0])
        for i in range(1, need):
            acc = ref.pointwise("add", acc, np.ascontiguousarray(prod[:, i]), idx=which)
        acc = ref.inntt(acc, idx=which)
        c = np.ascontiguousarray(ct[:, s]) if s < polys - 1 else np.zeros((n, level, N), dtype=np.uint64)
        if special:
            raised = np.zeros((n, level + 1, N), dtype=np.uint64)       # P c over [q_0 .. q_{level-1}, P]
            raised[:, :level] = ref.scalar_mul([qs[-1] % q for q in qs[:level]], c, idx=range(level))
            out[:, s] = ref.modswitch(ref.pointwise("add", acc, raised, idx=which), idx=which)
        else:
            out[:, s] = ref.pointwise("add", acc, c, idx=which)
    return out


def spec_window(qs, level, special, w, evk_coeff, ct_b):
    cring = spec.Ring(len(ct_b[0][0]), qs[:level])
    keyring = spec.Ring(cring.N, qs) if special else cring
    want = spec.keyswitch([([list(map(int, l)) for l in p[0]], [list(map(int, l)) for l in p[1]]) for p in evk_coeff],
                          [[list(map(int, l)) for l in c] for c in ct_b], cring, keyring, special, relin_window=w)
    return np.array(want, dtype=np.uint64)


@pytest.mark.parametrize("N,bits,Lk,level,special,w", [(64, 50, 3, 3, False, 16), (64, 50, 4, 3, True, 16), (2048, 50, 4, 3, True, 20),
                                                       (1 << 15, 50, 2, 2, False, 20)])
def test_keyswitch_window_across_chunks(N, bits, Lk, level, special, w):
    """ksw_table built once outside the loop; N = 2^15 takes the transform scratch in region 0 of its layout.  The oracle is the
    composition window_oracle, itself checked here against spec.keyswitch at N = 64, with and without the special prime."""
    qs = H.chain(bits, Lk, N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(N % 977 + w)
    nkey = spec.ndigits(int(np.prod([int(q) for q in qs], dtype=object)), 2 ** w)   # a key made over the whole key ring
    evk = H.uniform_evk(rng, qs, nkey, N)
    devk = dev(evk)
    out = tf.DeviceBuffer(BATCH * 2 * level * N)
    for polys in (2, 3):
        ct = H.rand_residues(rng, qs[:level], (BATCH, polys), N)
        ct[0, polys - 1, :, 0] = 0                                      # x = 0, Q - 1, 1
        ct[0, polys - 1, :, 1] = [q - 1 for q in qs[:level]]
        ct[0, polys - 1, :, 2] = 1
        dct = dev(ct)

        def call():
            ctx.keyswitch_window(level, w, devk.ptr, nkey, dct.ptr, polys, out.ptr, BATCH, key_limbs=Lk, special=special)
            return out.to_numpy((BATCH, 2, level, N))
        got = same_at_every_cap(ctx, call, out)
        want = window_oracle(ref, qs, level, special, w, evk, ct[PICKS])
        assert np.array_equal(got[PICKS], want), polys
        if N == 64:                                                     # the composition is the specification's key switch
            evk_coeff = ref.inntt(evk.reshape(-1, Lk, N)).reshape(evk.shape)
            for k in range(len(PICKS)):
                assert np.array_equal(want[k], spec_window(qs, level, special, w, evk_coeff, ct[PICKS[k]])), k


# ---------------------------------------------------------------------------------------------------
# tfhe_mul_relin, composed path (below and above the fused sizes): its own chunk loop around keyswitch_impl's, one workspace
# sized for both (region 0 of its layout is the key switch's span)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,qspec,special", [(1 << 11, "40x3", False), (1 << 15, "40x4", True)])
def test_mul_relin_composed_across_chunks(N, qspec, special):
    qs = ring_of(N, qspec)
    Lk = len(qs)
    level = Lk - 1 if special else Lk
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(N % 971 + special)
    evk = H.uniform_evk(rng, qs, Lk, N)
    devk = dev(evk)
    for square, rescale in ((False, 1), (True, 0), (False, 0), (True, 1)):
        c1 = H.rand_residues(rng, qs[:level], (BATCH, 2), N)
        c2 = c1 if square else H.rand_residues(rng, qs[:level], (BATCH, 2), N)
        d1 = dev(c1)
        d2 = d1 if square else dev(c2)
        lo = level - rescale
        out = tf.DeviceBuffer(BATCH * 2 * lo * N)

        def call():
            ctx.mul_relin(Lk, level, special, devk.ptr, Lk, d1.ptr, d2.ptr, out.ptr, BATCH, rescale=bool(rescale))
            return out.to_numpy((BATCH, 2, lo, N))
        got = same_at_every_cap(ctx, call, out)
        assert np.array_equal(got[PICKS], mul_relin_oracle(ref, level, special, evk, c1[PICKS], c2[PICKS], 0, rescale)), (square, rescale)


# ---------------------------------------------------------------------------------------------------
# tfhe_encrypt / tfhe_decrypt_phase: the fused kernels (two lanes on the mixed ring) and the composed path on both sides of them
# ---------------------------------------------------------------------------------------------------
ENC_SIZES = [(12, (60, 40, 60)), (11, (50, 60)), (15, (50, 60))]


@pytest.mark.parametrize("logn,bits", ENC_SIZES)
def test_encrypt_given_randomness_across_chunks(logn, bits):
    N = 1 << logn
    qs, ctx, ref = enc_context(N, bits)
    L = len(qs)
    rng = np.random.default_rng(400 + logn)
    pk = H.rand_residues(rng, qs, (2,), N)
    rand = rand_ints(rng, BATCH, N)
    msg = H.rand_residues(rng, qs, (BATCH,), N)
    dpk, drand, dmsg, out = dev(pk), dev_i32(rand), dev(msg), tf.DeviceBuffer(BATCH * 2 * L * N)

    def call():
        ctx.encrypt(L, L, dpk.ptr, out.ptr, BATCH, msg=dmsg.ptr, rand=drand.ptr, mult_e=65537)
        return out.to_numpy((BATCH, 2, L, N))
    got = same_at_every_cap(ctx, call, out)
    assert np.array_equal(got[PICKS], EO.encrypt_ref(ref, pk, rand[PICKS], 65537, msg[PICKS]))
    if logn <= 12:                                                      # the suite's own check of the whole batch, chunked
        with cap(ctx, 5):
            check_encrypt(N, bits, L, BATCH, 410 + logn, with_msg=True, mult=65537)


@pytest.mark.parametrize("logn,bits", ENC_SIZES)
def test_encrypt_counter_convention_across_chunks(logn, bits):
    """rand == NULL: u, e1, e2 of ciphertext b are the polynomials first_poly + b, + batch + b, + 2 batch + b of the Gaussian
    stream -- three tfhe_sample_gaussian calls over the WHOLE batch -- whatever chunk b falls into"""
    N, first, seed, su, se, mult = 1 << logn, 17, 0xC0FFEE, 3.2, 19.5, 65537
    qs, ctx, ref = enc_context(N, bits)
    L = len(qs)

    def gauss(first_poly, sigma, m):
        o = tf.DeviceBuffer(BATCH * L * N)
        ctx.sample_gaussian(L, sigma, m, seed, 1, first_poly, o.ptr, BATCH)
        return o.to_numpy((BATCH, L, N))
    u, e1, e2 = gauss(first, su, 1), gauss(first + BATCH, se, mult), gauss(first + 2 * BATCH, se, mult)
    assert len({e1[b].tobytes() for b in range(BATCH)}) == BATCH
    out = tf.DeviceBuffer(BATCH * 2 * L * N)
    one = np.zeros((2, L, N), dtype=np.uint64)
    one[1] = 1                                                          # masked = the NTT image of the constant 1: c0 = u + e1, c1 = e2
    dkey = dev(one)

    def call():
        ctx.encrypt(L, L, dkey.ptr, out.ptr, BATCH, sigma_u=su, sigma_e=se, mult_e=mult, seed=seed, stream=1, first_poly=first)
        return out.to_numpy((BATCH, 2, L, N))
    for n in (0,) + CAPS:
        poison(ctx, out)
        with cap(ctx, n):
            got = call()
        assert np.array_equal(ref.pointwise("sub", got[:, 0], e1), u), n
        assert np.array_equal(got[:, 1], e2), n


@pytest.mark.parametrize("logn,bits,combos", [(12, (60, 40, 60), None), (11, (50, 60), None), (15, (50, 60), None),
                                              (14, (60, 50), [(3, True)])])   # (three NTT-domain components at 2^14: composed)
def test_decrypt_phase_across_chunks(logn, bits, combos):
    N = 1 << logn
    qs, ctx, ref = enc_context(N, bits)
    L = len(qs)
    rng = np.random.default_rng(500 + logn)
    s = H.rand_residues(rng, qs, (), N)
    ds, out = dev(s), tf.DeviceBuffer(BATCH * L * N)
    for polys, ntt_in in combos or [(2, False), (2, True), (3, False), (3, True)]:
        ct = H.rand_residues(rng, qs, (BATCH, polys), N)
        dct = dev(ct)

        def call():
            ctx.decrypt_phase(L, L, ds.ptr, dct.ptr, polys, out.ptr, BATCH, ntt_in=ntt_in)
            return out.to_numpy((BATCH, L, N))
        got = same_at_every_cap(ctx, call, out)
        assert np.array_equal(got[PICKS], EO.decrypt_ref(ref, s, ct[PICKS], ntt_in)), (polys, ntt_in)
        if logn <= 12:
            with cap(ctx, 5):
                check_decrypt(N, bits, L, polys, ntt_in, BATCH, 510 + logn)


# ---------------------------------------------------------------------------------------------------
# CKKS encode / decode, the plain codec, the samplers
# ---------------------------------------------------------------------------------------------------
def ckks_encoding_close(slot_row, words, ring, scale, what=None):
    """one encoding [L][N] against spec.ckks_encode: integers equal up to the rounding of the float transform; -> the words as lists"""
    N, eps = ring.N, 2.0 ** -53
    want = spec.poly_to_ints(spec.ckks_encode(list(slot_row), ring, scale), ring)
    enc = [list(map(int, l)) for l in words]
    diff = [spec.centred(g - w_, ring.Q) for g, w_ in zip(spec.poly_to_ints(enc, ring), want)]
    allowed = max(1, int(8 * np.log2(N) * eps * np.abs(slot_row).max() * float(scale)))
    assert max(abs(d) for d in diff) <= allowed, (what, max(abs(d) for d in diff), allowed)
    if allowed == 1:
        assert sum(1 for d in diff if d) <= max(2, N // 20), what
    return enc


def ckks_decoding_close(slot_row, enc, dec_row, ring, scale, what=None):
    """the device's decoding of `enc` against spec.ckks_decode of the same words, and against the slots that were encoded"""
    N, eps = ring.N, 2.0 ** -53
    ref = spec.ckks_decode(enc, ring, scale)
    tol = 8 * np.log2(N) * eps * max(1.0, np.abs(ref).max()) * 4
    assert np.abs(dec_row - ref).max() <= tol, (what, np.abs(dec_row - ref).max(), tol)
    assert np.abs(dec_row - slot_row).max() <= N * 2.0 / float(scale) + tol, what


@pytest.mark.parametrize("N", [64, 4096])
def test_ckks_codec_across_chunks(N):
    """(a): the tolerances of test_ckks_encode_decode_match_oracle on the picks; (b): identical words, the slot doubles as uint64"""
    L, scale = 2, 2 ** 40
    qs = H.chain(50, L, N)
    ring = spec.Ring(N, qs)
    ctx = tf.Context(N, qs)
    rng = np.random.default_rng(N + 19)
    slots = rng.normal(size=(BATCH, N // 2)) * 3 + 1j * rng.normal(size=(BATCH, N // 2))
    mant, exp2 = tf.she.scale_parts(scale)
    dz, denc, dslots = dev(np.ascontiguousarray(slots).view(np.uint64)), tf.DeviceBuffer(BATCH * L * N), tf.DeviceBuffer(BATCH * N)

    def encode():
        ctx.ckks_encode(L, mant, exp2, dz.ptr, denc.ptr, BATCH)
        return denc.to_numpy((BATCH, L, N))

    def decode():
        ctx.ckks_decode(L, mant, exp2, denc.ptr, dslots.ptr, BATCH)
        return dslots.to_numpy((BATCH, N))
    res = same_at_every_cap(ctx, encode, denc)
    dec = same_at_every_cap(ctx, decode, dslots).view(np.complex128)            # of the device encoding (denc holds `res` again)
    for b in PICKS:
        ckks_decoding_close(slots[b], ckks_encoding_close(slots[b], res[b], ring, scale, b), dec[b], ring, scale, b)


def test_plain_codec_across_chunks():
    """tfhe_plain_encode / tfhe_plain_decode / tfhe_bfv_noise_max: the plan chunks by its context's cap"""
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
    out, enc, words = tf.DeviceBuffer(BATCH * N), tf.DeviceBuffer(BATCH * L * N), tf.DeviceBuffer(BATCH * plan.delta_words)
    try:
        for scheme, decode in ((tf.native.PLAIN_BFV, spec.bfv_decode), (tf.native.PLAIN_BGV, spec.bgv_decode)):

            def dec():
                plan.decode(scheme, src.ptr, out.ptr, BATCH)
                return out.to_numpy((BATCH, N))

            def encode():
                plan.encode(scheme, dm.ptr, enc.ptr, BATCH)
                return enc.to_numpy((BATCH, L, N))
            got, gote = same_at_every_cap(ctx, dec, out), same_at_every_cap(ctx, encode, enc)
            for b in PICKS:
                assert got[b].tolist() == decode([[int(v) for v in l] for l in res[b]], ring, t), (scheme, b)
                mi = [int(v) for v in m[b]]
                want = spec.bfv_encode(mi, ring, t) if scheme == tf.native.PLAIN_BFV else [[x % t % q for x in mi] for q in qs]
                assert gote[b].tolist() == want, (scheme, b)

        def noise():
            plan.noise_max(src.ptr, words.ptr, BATCH)
            return words.to_numpy((BATCH, plan.delta_words))
        gotw = same_at_every_cap(ctx, noise, words)
        for b in PICKS:
            ints = spec.poly_to_ints([[int(v) for v in l] for l in res[b]], ring)
            worst = max((delta - x % delta) if x % delta > delta // 2 else x % delta for x in ints)
            assert sum(int(wd) << (64 * i) for i, wd in enumerate(gotw[b])) == worst, b
    finally:
        plan.close()


def test_samplers_across_chunks():
    N, level, seed, first = 64, 2, 0x5EED5EED, 5
    qs = H.chain(50, level, N)
    ctx = tf.Context(N, qs)
    out = tf.DeviceBuffer(BATCH * level * N)

    def uniform():
        ctx.sample_uniform(level, seed, 0, first, out.ptr, BATCH)
        return out.to_numpy((BATCH, level, N))

    def gaussian(first_poly=first, count=BATCH):
        ctx.sample_gaussian(level, 3.2, 1, seed, 1, first_poly, out.ptr, count)
        return out.to_numpy((BATCH, level, N))[:count]
    got = same_at_every_cap(ctx, uniform, out)
    for p in PICKS:
        for l, q in enumerate(qs):
            assert [int(v) for v in got[p, l]] == [spec.sample_uniform_mod(((first + p) << 32) | k, l, 0, seed, q) for k in range(N)], (p, l)
    g = same_at_every_cap(ctx, gaussian, out)
    assert len({g[p].tobytes() for p in range(BATCH)}) == BATCH
    for p in PICKS:                                                     # polynomial p is polynomial 0 of a call that starts p later
        assert np.array_equal(gaussian(first + p, 1)[0], g[p]), p


# ---------------------------------------------------------------------------------------------------
# the knob itself
# ---------------------------------------------------------------------------------------------------
def test_chunk_cap_cuts_the_batch_and_zero_restores_the_default():
    N, Lk, level = 1 << 10, 4, 3
    qs = H.chain(40, Lk, N)
    ctx = tf.Context(N, qs)
    rng = np.random.default_rng(10)
    devk, dct = dev(H.uniform_evk(rng, qs, Lk, N)), dev(H.rand_residues(rng, qs[:level], (BATCH, 2), N))
    out = tf.DeviceBuffer(BATCH * 2 * level * N)

    def call():
        poison(ctx, out)
        ctx.keyswitch(Lk, level, True, devk.ptr, Lk, dct.ptr, 2, out.ptr, BATCH)
        return out.to_numpy()

    def launches():                                                     # profiled (transform) launches of one call
        ctx.prof_enable(True)
        try:
            call()
            return ctx.prof_read()[0]
        finally:
            ctx.prof_enable(False)
    try:
        base, n0 = call(), launches()
        assert n0 > 0
        for n in CAPS:
            ctx.set_chunk(n)
            assert np.array_equal(call(), base)
            assert launches() == n0 * -(-BATCH // n), n                  # the cap is in force: every chunk launches its own transforms
            ctx.set_chunk(0)
            assert np.array_equal(call(), base) and launches() == n0     # 0 restores the default: the same words, one chunk
        for n in (BATCH, BATCH + 1, 1000):                              # a cap at or above the batch changes nothing
            ctx.set_chunk(n)
            assert np.array_equal(call(), base) and launches() == n0, n
    finally:
        ctx.set_chunk(0)
    with pytest.raises(AssertionError):
        ctx.set_chunk(-1)
    assert np.array_equal(call(), base) and launches() == n0            # a rejected value leaves the cap as it was


# ---------------------------------------------------------------------------------------------------
# the default seams themselves (no cap): 512 ciphertexts per key-switch chunk, 4096 per codec / composed encryption chunk, 32768
# polynomials per sampler launch, 65535 rows per broadcast
# ---------------------------------------------------------------------------------------------------
def stitched(call, batch, step=256):
    """call(b0, nb) -> words of ciphertexts b0 .. b0 + nb of the batch, from sub-batches that never reach a chunk boundary"""
    return np.concatenate([call(b0, min(step, batch - b0)) for b0 in range(0, batch, step)], axis=0)


def test_default_seam_of_the_key_switches_at_512():
    N, Lk, level, batch, w = 1 << 10, 4, 2, 1030, 16
    qs = H.chain(40, Lk, N)
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    rng = np.random.default_rng(1030)
    picks = [0, 511, 512, 513, 1023, 1024, 1029]
    ct = H.rand_residues(rng, qs[:level], (batch, 2), N)
    dct = dev(ct)
    row = 2 * level * N
    gs = galois_elements(N)[:2]
    evks = [H.uniform_evk(rng, qs, Lk, N) for _ in gs]
    devks = [dev(e) for e in evks]
    out, many = tf.DeviceBuffer(batch * row), tf.DeviceBuffer(2 * batch * row)

    def ks(b0, nb):
        ctx.keyswitch(Lk, level, True, devks[0].ptr, Lk, dct.ptr + b0 * row * 8, 2, out.ptr, nb)
        return out.to_numpy()[:nb * row].reshape(nb, 2, level, N)

    def rot(b0, nb):
        ctx.rotate(Lk, level, True, devks[1].ptr, Lk, gs[1], dct.ptr + b0 * row * 8, out.ptr, nb)
        return out.to_numpy()[:nb * row].reshape(nb, 2, level, N)

    def rot_many(b0, nb):
        ctx.rotate_many(Lk, level, True, [d.ptr for d in devks], Lk, gs, dct.ptr + b0 * row * 8, many.ptr, nb)
        return many.to_numpy()[:2 * nb * row].reshape(2, nb, 2, level, N).transpose(1, 0, 2, 3, 4)
    poison(ctx, out, many)
    got = ks(0, batch)
    assert np.array_equal(got[picks], ref.keyswitch(level, True, evks[0], ct[picks]))
    assert np.array_equal(got, stitched(ks, batch))
    poison(ctx, out)
    got = rot(0, batch)
    assert np.array_equal(got[picks], ref_rotate(ref, level, True, evks[1], gs[1], ct[picks]))
    assert np.array_equal(got, stitched(rot, batch))
    gotm = rot_many(0, batch)                                           # [batch][2 rotations]...
    assert np.array_equal(gotm[:, 1], got)
    assert np.array_equal(gotm[picks, 0], ref_rotate(ref, level, True, evks[0], gs[0], ct[picks]))
    assert np.array_equal(gotm, stitched(rot_many, batch))
    nkey = spec.ndigits(int(np.prod([int(q) for q in qs], dtype=object)), 2 ** w)
    wkey = H.uniform_evk(rng, qs, nkey, N)
    dwkey = dev(wkey)

    def ksw(b0, nb):
        ctx.keyswitch_window(level, w, dwkey.ptr, nkey, dct.ptr + b0 * row * 8, 2, out.ptr, nb, key_limbs=Lk, special=True)
        return out.to_numpy()[:nb * row].reshape(nb, 2, level, N)
    poison(ctx, out)
    got = ksw(0, batch)
    assert np.array_equal(got[picks], window_oracle(ref, qs, level, True, w, wkey, ct[picks]))
    assert np.array_equal(got, stitched(ksw, batch))


def test_default_seam_of_the_ckks_codec_at_4096():
    N, L, batch, scale = 16, 2, 4097, 2 ** 40
    qs = H.chain(50, L, N)
    ring = spec.Ring(N, qs)
    ctx = tf.Context(N, qs)
    rng = np.random.default_rng(4097)
    slots = rng.normal(size=(batch, N // 2)) * 3 + 1j * rng.normal(size=(batch, N // 2))
    mant, exp2 = tf.she.scale_parts(scale)
    dz, denc, dslots = dev(np.ascontiguousarray(slots).view(np.uint64)), tf.DeviceBuffer(batch * L * N), tf.DeviceBuffer(batch * N)

    def encode(b0, nb):
        ctx.ckks_encode(L, mant, exp2, dz.ptr + b0 * N * 8, denc.ptr + b0 * L * N * 8, nb)
        return denc.to_numpy((batch, L, N))[b0:b0 + nb]

    def decode(b0, nb):
        ctx.ckks_decode(L, mant, exp2, denc.ptr + b0 * L * N * 8, dslots.ptr + b0 * N * 8, nb)
        return dslots.to_numpy((batch, N))[b0:b0 + nb]
    poison(ctx, denc, dslots)
    res = encode(0, batch).copy()
    dec = decode(0, batch).copy()
    assert np.array_equal(res, stitched(encode, batch, 1000))           # (writes the same words back)
    assert np.array_equal(dec, stitched(decode, batch, 1000))
    eps, dec = 2.0 ** -53, dec.view(np.complex128)
    for b in (0, 4095, 4096):
        want = spec.poly_to_ints(spec.ckks_encode(list(slots[b]), ring, scale), ring)
        enc = [list(map(int, l)) for l in res[b]]
        diff = [spec.centred(g - w_, ring.Q) for g, w_ in zip(spec.poly_to_ints(enc, ring), want)]
        assert max(abs(d) for d in diff) <= max(1, int(8 * np.log2(N) * eps * np.abs(slots[b]).max() * float(scale))), b
        ref = spec.ckks_decode(enc, ring, scale)
        assert np.abs(dec[b] - ref).max() <= 8 * np.log2(N) * eps * max(1.0, np.abs(ref).max()) * 4, b


def test_default_seam_of_composed_encryption_at_4096():
    N, batch, bits = 32, 4097, (50, 60)
    qs, ctx, ref = enc_context(N, bits)
    L = len(qs)
    check_encrypt(N, bits, L, batch, 4097, with_msg=True, mult=65537)   # given randomness against the oracle, every ciphertext
    for polys, ntt_in in ((2, False), (3, True)):
        check_decrypt(N, bits, L, polys, ntt_in, batch, 4098 + polys)
    # rand == NULL: the counter convention with b0 = 4096
    first, seed, su, se = 9, 0xABCDEF, 3.2, 19.5

    def gauss(first_poly, sigma):
        o = tf.DeviceBuffer(batch * L * N)
        ctx.sample_gaussian(L, sigma, 1, seed, 1, first_poly, o.ptr, batch)
        return o.to_numpy((batch, L, N))
    u, e1, e2 = gauss(first, su), gauss(first + batch, se), gauss(first + 2 * batch, se)
    one = np.zeros((2, L, N), dtype=np.uint64)
    one[1] = 1
    out = tf.DeviceBuffer(batch * 2 * L * N)
    poison(ctx, out)
    ctx.encrypt(L, L, dev(one).ptr, out.ptr, batch, sigma_u=su, sigma_e=se, seed=seed, stream=1, first_poly=first)
    got = out.to_numpy((batch, 2, L, N))
    assert np.array_equal(ref.pointwise("sub", got[:, 0], e1), u) and np.array_equal(got[:, 1], e2)


def test_default_seam_of_the_samplers_at_32768():
    N, level, count, first, seed = 16, 2, 32770, 5, 0x0DDBA11
    qs = H.chain(50, level, N)
    ctx = tf.Context(N, qs)
    out, one = tf.DeviceBuffer(count * level * N), tf.DeviceBuffer(level * N)
    rows = [0, 32767, 32768, 32769]
    assert rows[-1] == count - 1
    poison(ctx, out)
    ctx.sample_uniform(level, seed, 0, first, out.ptr, count)
    got = out.to_numpy((count, level, N))
    for p in rows:
        for l, q in enumerate(qs):
            assert [int(v) for v in got[p, l]] == [spec.sample_uniform_mod(((first + p) << 32) | k, l, 0, seed, q) for k in range(N)], (p, l)
    poison(ctx, out)
    ctx.sample_gaussian(level, 3.2, 1, seed, 1, first, out.ptr, count)
    g = out.to_numpy((count, level, N))
    for p in rows:
        ctx.sample_gaussian(level, 3.2, 1, seed, 1, first + p, one.ptr, 1)
        assert np.array_equal(one.to_numpy((level, N)), g[p]), p
    assert len({g[p].tobytes() for p in rows}) == len(rows)


def test_broadcast_poly_at_its_row_limit():
    words, count = 32, 65535
    ctx = tf.Context(16, H.chain(50, 2, 16))
    src = np.arange(1, words + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    dsrc, dst = dev(src), tf.DeviceBuffer((count + 1) * words)
    lib = tf.native.lib()
    tf.native.check(lib.tfhe_memset(ctx.h, dst.ptr, 0, (count + 1) * words * 8))
    tf.native.check(lib.tfhe_broadcast_poly(ctx.h, dst.ptr, dsrc.ptr, words, count))
    got = dst.to_numpy((count + 1, words))
    for row in (0, count // 2, count - 1):
        assert np.array_equal(got[row], src), row
    assert not got[count].any()                                         # nothing past the last row
    assert lib.tfhe_broadcast_poly(ctx.h, dst.ptr, dsrc.ptr, words, count + 1) == tf.native.E_BADARG
