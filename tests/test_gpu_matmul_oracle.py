"""tfhe_matmul_bsgs_blocks, tfhe_matmul_bsgs and tfhe_matmul_diag through the raw C ABI against tests/matmul_oracle.py (the C oracle's
Galois map, key switch and transforms around exact integer sums; pinned to oracle/spec.py by tests/test_matmul_oracle_cpu.py), word
for word, at the modulus edges, past 32 limbs and at the term limits.

The other tests of these entry points compare the one call with a composition of the device's own calls through the mirror, on
comfortable primes and Gaussian slots.  Here nothing but tf.Context and device buffers stands between the arrays and the ABI: no
mirror, no DeviceRng, no encoder.  Inputs are deterministic and growth-maximising (the vocabulary of tests/test_gpu_modulus_edges.py):
  ciphertexts  item 0 of a batch is _ks_ct's edge item (last component at the centring edges 0, 1, q - 1, floor(q/2), floor(q/2) + 1, the
               other all q - 1), item 1 uniform;
  keys         key r (baby keys first, then the giant ones) is all q - 1 for even r and uniform for odd r;
  diagonals    one of the six edge_rows kinds each: the first two terms of every inner sum are all q - 1 and a uniform row, the
               others cycle through the six kinds, shifted by the giant step;
  bias         q - 1 in every word;
  Galois       3^s mod 2N for s = 1, 2, ... (past s = N/2 - 1, where the powers repeat, 2N - 3^s), the last giant step 2N - 1.
run_case asserts equality with the oracle, canonical output words, untouched operands, and the same words under a chunk cap of 1.

Wall time of the oracle on an 8-core CPU, per case: 2.1 s at level 33 of N = 2^12 (the object-dtype sums) and for 64 inputs (64 small key
switches), 1.6 s for 64 baby steps, 0.7 - 1.0 s at N = 2^14 .. 2^16, below 0.5 s elsewhere; no case was cut down.  On the MI355X machine
the whole file takes 9 s."""
import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import helpers as H
from tests import many_limbs as ML
from tests import matmul_oracle as MO
from tests.test_gpu_modulus_edges import _ks_ct, edge, edge_rows

pytestmark = pytest.mark.gpu


def dev(a):
    return tf.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.uint64))


def poison(ctx, buf):
    tf.native.check(tf.native.lib().tfhe_memset(ctx.h, buf.ptr, 0xA5, buf.n * 8))


def galois_elements(N, n_baby, n_giant):
    """distinct steps: 3^s mod 2N, then 2N - 3^s (neither 1 nor 2N - 1 among them; more than N - 2 keys repeat elements); the last
    giant step is the conjugation 2N - 1"""
    pool = [pow(3, s, 2 * N) for s in range(1, N // 2)] + [2 * N - pow(3, s, 2 * N) for s in range(1, N // 2)]
    assert len(set(pool)) == len(pool) and 1 not in pool and 2 * N - 1 not in pool
    gs = [pool[k % len(pool)] for k in range(n_baby + n_giant)]
    if n_giant:
        gs[-1] = 2 * N - 1
    return gs[:n_baby], gs[n_baby:]


def make_keys(qs, N, n, rng):
    """[Lk][2][Lk][N] each: all q - 1 for even r, uniform for odd r (all q - 1 alone would make every rotation's key sum a multiple of
    one value and could hide a swapped key)"""
    Lk = len(qs)
    ones = np.broadcast_to((np.array(qs, dtype=np.uint64) - 1)[None, None, :, None], (Lk, 2, Lk, N))
    return [H.uniform_evk(rng, qs, Lk, N) if r % 2 else ones.copy() for r in range(n)]


def make_diags(cq, N, n_baby, n_giant, n_in, seed):
    """[n_in][n_giant + 1][n_baby + 1][level][N]: term t = m (n_baby + 1) + i of inner sum j is all q - 1 for t = 0, uniform for t = 1, and
    kind (t + j) mod 6 of edge_rows after that; every uniform row is its own draw"""
    nb1, ng1 = n_baby + 1, n_giant + 1
    E = edge_rows(cq, N, seed, n_in * ng1 * nb1)                        # one copy of the six kinds per diagonal
    out = np.empty((n_in, ng1, nb1, len(cq), N), dtype=np.uint64)
    c = 0
    for m in range(n_in):
        for j in range(ng1):
            for i in range(nb1):
                t = m * nb1 + i
                out[m, j, i] = E[6 * c + ((0, 5)[t] if t < 2 else (t + j) % 6)]
                c += 1
    return out


def run_case(qs, logn, special, shape, bias=False, batch=2, level=None, variants=(0,), seed=0):
    N = 1 << logn
    n_baby, n_giant, n_in = shape
    Lk = len(qs)
    level = (Lk - 1 if special else Lk) if level is None else level
    cq = qs[:level]
    ctx, ref = tf.Context(N, qs), ref_cpu.RefCtx(N, qs)
    assert ctx.psis == ref.psis
    rng = np.random.default_rng(1000 * logn + 10 * Lk + special + seed)
    baby_gs, giant_gs = galois_elements(N, n_baby, n_giant)
    keys = make_keys(qs, N, n_baby + n_giant, rng)
    cts = [_ks_ct(qs, level, 2, N, rng)[:batch] for _ in range(n_in)]
    assert batch in (1, 2) and all(c.shape == (batch, 2, level, N) for c in cts)
    diags = make_diags(cq, N, n_baby, n_giant, n_in, 7 + seed)
    bias_h = np.broadcast_to((np.array(cq, dtype=np.uint64) - 1)[:, None], (level, N)).copy() if bias else None
    # device operands; the keys go through tfhe_galois_key_prepare, as the ABI asks
    dkeys, prep = [dev(k) for k in keys], []
    for k, g in zip(dkeys, baby_gs + giant_gs):
        p = tf.DeviceBuffer(k.n)
        ctx.galois_key_prepare(Lk, Lk, g, k.ptr, p.ptr)
        prep.append(p)
    prep_h = [p.to_numpy() for p in prep]
    bk, gk = [p.ptr for p in prep[:n_baby]], [p.ptr for p in prep[n_baby:]]
    dcts, ddiags = [dev(c) for c in cts], [dev(d) for d in diags]
    dbias = dev(bias_h) if bias else None
    words = batch * 2 * level * N
    out = tf.DeviceBuffer(words)
    qv = np.array(cq, dtype=np.uint64).reshape(1, 1, level, 1)

    def result(call, want, what):
        poison(ctx, out)
        call()
        got = out.to_numpy((batch, 2, level, N))
        assert np.array_equal(got, want), what
        assert (got < qv).all(), what

    def operands_unchanged(what):
        for k, h in zip(dkeys, keys):
            assert np.array_equal(k.to_numpy(h.shape), h), what
        for p, h in zip(prep, prep_h):
            assert np.array_equal(p.to_numpy(), h), what
        for d, h in zip(dcts + ddiags, cts + list(diags)):
            assert np.array_equal(d.to_numpy(h.shape), h), what
        if bias:
            assert np.array_equal(dbias.to_numpy(bias_h.shape), bias_h), what

    def blocks():
        ctx.matmul_bsgs_blocks(Lk, level, special, bk, baby_gs, gk, giant_gs, Lk, [d.ptr for d in ddiags], [c.ptr for c in dcts],
                               dbias.ptr if bias else None, out.ptr, batch)

    def one():
        ctx.matmul_bsgs(Lk, level, special, bk, baby_gs, gk, giant_gs, Lk, ddiags[0].ptr, dcts[0].ptr, out.ptr, batch)
    calls = [("blocks", blocks, MO.matmul_bsgs_blocks_ref(ref, level, special, keys[:n_baby], baby_gs, keys[n_baby:], giant_gs, diags, cts, bias_h))]
    if n_in == 1 and not bias:
        calls.append(("bsgs", one, calls[0][2]))                             # one input, no bias: the same words
    if n_giant == 0:
        for m in range(n_in):                                                # inner_0 of every input alone, in the NTT domain
            def diag(m=m):
                ctx.matmul_diag(Lk, level, special, bk, Lk, baby_gs, ddiags[m].ptr, dcts[m].ptr, out.ptr, batch)
            calls.append((f"diag {m}", diag, MO.matmul_diag_ref(ref, level, special, keys[:n_baby], baby_gs, diags[m][0], cts[m])))
    try:
        for variant in variants:
            ctx.set_ntt_variant(variant)
            for cap in ((0, 1) if batch > 1 else (0,)):
                ctx.set_chunk(cap)
                for name, call, want in calls:
                    result(call, want, (name, "variant", variant, "chunk cap", cap))
                    operands_unchanged((name, variant, cap))
    finally:
        ctx.set_chunk(0)
        ctx.set_ntt_variant(0)


def uniform(name, n):
    """n ciphertext limbs at the named edge (+ one more as the special prime)"""
    return lambda N, special: edge(name, n + special, N)


def above(bits, n):
    return lambda N, special: H.primes_above(1 << bits, n + special, N)


def mixed_policy(N, special):
    """the top fp64 prime, the bottom u64 prime, a fold prime and the top of the narrow class, special prime = the top 62-bit one: both
    lanes in one call, and a fused lift because the target limbs are not all fp64-size"""
    return edge("fp-top", 1, N) + edge("u64-bottom", 1, N) + edge("fold62", 1, N) + edge("top52", 1, N) + edge("top62", 1, N)


def _case(group, ring, logn, shape, special, **kw):
    ident = f"{group}-logn{logn}-{'x'.join(map(str, shape))}-{'special' if special else 'plain'}"
    if "level" in kw:
        ident += f"-level{kw['level']}"
    return pytest.param(ring, logn, shape, special, kw, id=ident)


CASES = []
for sp in (True, False):
    # the window top: chunk 1 at 62 bits (a fold before every rotated term, seeded from input 1 on, in k_md_acc and k_md_acc_dense);
    # chunks 2 and 4 crossed inside a sum and across two seeds
    CASES.append(_case("top62", uniform("top62", 3), 10, (3, 2, 3), sp, bias=True))
    CASES += [_case(n, uniform(n, 3), 10, (5, 1, 3), sp) for n in ("top61", "top60")]
    # 2^64 mod q close to q: the nested key switch's k_ks_inner fold and the Barrett folds of the sums
    CASES += [_case(n, uniform(n, 3), 10, (3, 2, 2), sp, bias=True) for n in ("fold62", "fold61")]
    # ArithFp at its class limit and u64 just above it through md_rotations
    CASES += [_case(n, uniform(n, 3), 12, (2, 2, 2), sp) for n in ("fp-top", "u64-bottom")]
    CASES.append(_case("mixed", mixed_policy, 12, (2, 2, 2), sp, bias=True))
    # n_digits > level, the special-prime table of a lower level, one-limb rows
    CASES += [_case("below-key", uniform("top61", 4), 10, (2, 2, 2), sp, level=lv) for lv in (1, 2)]
    # output tiles: NG = 1, 2, 4; whole tiles; a ragged last tile of 1, 2 and 3 live lanes; seeded loads of a dead lane
    CASES += [_case("tiles", above(40, 3), 8, (2, ng, 2), sp) for ng in (0, 1, 2, 3, 4, 7, 8)]
    # the admitted maxima: rot_tail_arg_t::g full, 17 tiles, 63 seeded launches
    CASES += [_case("limits", above(40, 3), 6, s, sp) for s in ((64, 1, 1), (1, 64, 1), (1, 1, 64), (64, 0, 2))]
    # k_md_acc's team split: n / per = 0, below nslot, and the clamped lanes at NG = 4
    CASES += [_case("small-rows", above(50, 2), ln, (2, 3, 2), sp) for ln in (4, 8, 11, 13)]
# routes that exist only with the special prime.  All targets fp64-size and the special prime not: md_lift_is_fused false, k_md_lift,
# k_md_acc<false, 4, SEED>
CASES += [_case("lift-unfused", lambda N, special: edge("fp-top", 3, N) + edge("top62", 1, N), ln, (2, 2, 2), True) for ln in (12, 14)]
# the fused digit-lift mode: k_md_acc<true, 2, SEED>
CASES.append(_case("lift-fused", uniform("fp-top", 3), 14, (2, 1, 2), True))
# pair / quad lift and top-stage lift; once more under variant 2, the unfused route at N >= 2^15
for ln in (15, 16):
    CASES.append(_case("large-fp", uniform("fp-top", 2), ln, (1, 1, 2), True, batch=1, variants=(0, 2)))
    CASES.append(_case("large-mixed", lambda N, special: edge("fp-top", 1, N) + edge("top62", 2, N), ln, (1, 1, 2), True, batch=1, variants=(0, 2)))


@pytest.mark.parametrize("ring,logn,shape,special,kw", CASES)
def test_products_match_the_oracle(ring, logn, shape, special, kw):
    run_case(ring(1 << logn, special), logn, special, shape, **kw)


# level > 32: the unfused lift, limb_sel_t past its first mask word, 33 digits in the nested key switch; level 32 next to it on the
# fused side
def _seam_ring(name, n, N):
    return ML.mixed(n, N) if name == "mixed" else ML.ring(name, N)[:n]


SEAM = [(name, 5, level, sp, (2, 2, 2)) for name in ("U40", "W40", "mixed") for level, sp in ((32, True), (33, True), (33, False), (40, False))]
SEAM += [(name, 12, 33, True, (1, 1, 2)) for name in ("U40", "W40", "mixed")]


@pytest.mark.parametrize("name,logn,level,special,shape", SEAM)
def test_products_match_the_oracle_across_the_32_limb_seam(name, logn, level, special, shape):
    N = 1 << logn
    run_case(_seam_ring(name, level + special, N), logn, special, shape, bias=True, seed=level)


@pytest.mark.parametrize("special", [True, False])
def test_one_step_or_input_too_many_is_refused_without_a_launch(special):
    """65 baby steps, 65 giant steps or 65 inputs: TFHE_E_BADARG (AssertionError through native.check), no transform launched, the
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
    for n_baby, n_giant, n_in in ((65, 1, 1), (1, 65, 1), (1, 1, 65)):
        d = dev(H.rand_residues(rng, qs[:level], (n_giant + 1, n_baby + 1), N))
        poison(ctx, out)
        before = out.to_numpy()
        ctx.prof_enable(True)
        try:
            with pytest.raises(AssertionError, match="outside"):
                ctx.matmul_bsgs_blocks(Lk, level, special, [prep.ptr] * n_baby, [3] * n_baby, [prep.ptr] * n_giant, [3] * n_giant, Lk,
                                       [d.ptr] * n_in, [ct.ptr] * n_in, None, out.ptr, 1)
            if n_in == 1:
                with pytest.raises(AssertionError, match="outside"):
                    ctx.matmul_bsgs(Lk, level, special, [prep.ptr] * n_baby, [3] * n_baby, [prep.ptr] * n_giant, [3] * n_giant, Lk, d.ptr, ct.ptr,
                                    out.ptr, 1)
            assert ctx.prof_read()[0] == 0
        finally:
            ctx.prof_enable(False)
        assert np.array_equal(out.to_numpy(), before)
