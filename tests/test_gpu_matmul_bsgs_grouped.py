"""tfhe_matmul_bsgs_grouped on the device against tests/matmul_bsgs_grouped_oracle.py and against the C-ABI chain it states --
tfhe_rotate_many_grouped per input -> tfhe_nntt -> one tfhe_dot per giant step over all terms -> tfhe_inntt -> tfhe_rotate_grouped on the
plain key -> tfhe_add (-> + bias) -- word for word, every word read back below its modulus and `out` pre-filled with 0xA5..: the counts
of baby steps, giant steps (a full output tile of four plus a ragged one), inputs (the seeded accumulation), bias and batch; every
number of special primes 0 .. 4, one digit, two arithmetic policies side by side, N = 2^15; the identities with
tfhe_matmul_diag_grouped and tfhe_matmul_bsgs_blocks; chunks and a dirty workspace; edge words; the limits; the refusals; the
coefficient route in a process of its own; and the mirror."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import helpers as H
from tests import ks_grouped_oracle as KO
from tests import matmul_bsgs_grouped_oracle as BO
from tests.dirty_ws import on_dirty_workspace
from tests.test_gpu_chunk_seams import cap
from tests.test_gpu_ks_grouped import dev, operands, pair, plant, poisoned, qcol
from tests.test_gpu_rotate_many_grouped import g_many, key_set, prepare

pytestmark = pytest.mark.gpu
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case:
    """the operands of one call: plain keys for the oracle, their prepared device copies, diagonals, ciphertexts, bias"""

    def __init__(self, N, qs, k, alpha, level, n_baby, n_giant, n_in=1, batch=1, bias=False, seed=0, edge=False, planted=False, ctx=None):
        self.N, self.qs, self.k, self.alpha, self.level, self.batch = N, list(qs), k, alpha, level, batch
        self.Lk = len(qs)
        self.ctx, self.ref = (ctx, ref_cpu.RefCtx(N, qs)) if ctx is not None else pair(N, qs)
        self.bgs = [pow(5, i + 1, 2 * N) for i in range(n_baby)]
        self.ggs = [pow(5, (j + 1) * (n_baby + 1), 2 * N) for j in range(n_giant)]
        if n_giant >= 2:
            self.ggs[-1] = 2 * N - 1                       # every sign but one flips
        if n_baby >= 2:
            self.bgs[-1] = g_many(N)                       # many wraps
        gs = self.bgs + self.ggs
        if gs:
            n_keys = min(len(gs), 3)
            plain = [operands(N, qs, k, alpha, level, 2, 1, seed=seed + 17 * i, edge=edge)[0] for i in range(n_keys)]
            evks = [plain[r % n_keys] for r in range(len(gs))]
            made, devs = {}, []
            for r, g in enumerate(gs):                     # a key used with two elements is prepared once per element
                key = (r % n_keys, int(g))
                if key not in made:
                    made[key] = prepare(self.ctx, self.Lk, evks[r], g)
                devs.append(made[key])
        else:
            evks, devs = [], []
        self.bk, self.gk = evks[:n_baby], evks[n_baby:]
        self.bdev, self.gdev = devs[:n_baby], devs[n_baby:]
        self.nd = evks[0].shape[0] if evks else -(-level // alpha)
        rng = np.random.default_rng(seed + 1000 * n_baby + 100 * n_giant + n_in)
        ql = qs[:level]
        if edge:
            self.diags = [np.broadcast_to(qcol(ql) - np.uint64(1), (n_giant + 1, n_baby + 1, level, N)).copy() for _ in range(n_in)]
        else:
            self.diags = [H.rand_residues(rng, ql, (n_giant + 1, n_baby + 1), N) for _ in range(n_in)]
        self.cts = [operands(N, qs, k, alpha, level, 2, batch, seed=seed + 31 * m, edge=edge)[1] for m in range(n_in)]
        if planted:
            self.cts = [plant(c, qs, level, alpha) for c in self.cts]
        self.bias = None
        if bias:
            self.bias = (np.broadcast_to(qcol(ql) - np.uint64(1), (level, N)).copy() if edge else H.rand_residues(rng, ql, (), N))
        self.ddev = [dev(d) for d in self.diags]
        self.cdev = [dev(c) for c in self.cts]
        self.bdevbuf = None if self.bias is None else dev(self.bias)

    def call(self, out):
        self.ctx.matmul_bsgs_grouped(self.Lk, self.level, self.k, self.alpha, [d.ptr for d in self.bdev], self.bgs, [d.ptr for d in self.gdev],
                                     self.ggs, self.nd, [d.ptr for d in self.ddev], [c.ptr for c in self.cdev],
                                     None if self.bdevbuf is None else self.bdevbuf.ptr, out.ptr, self.batch)

    def run(self):
        out = poisoned(self.batch * 2 * self.level * self.N)
        self.call(out)
        got = out.to_numpy((self.batch, 2, self.level, self.N))
        assert (got < qcol(self.qs[:self.level])).all()
        return got

    def oracle(self):
        return BO.matmul_bsgs_blocks_grouped_ref(self.ref, self.level, self.k, self.alpha, self.bk, self.bgs, self.gk, self.ggs, self.diags, self.cts,
                                                 bias=self.bias)

    def chain(self):
        """the composition the header states, entry point by entry point on the device"""
        ctx, N, level, batch, Lk, k, alpha = self.ctx, self.N, self.level, self.batch, self.Lk, self.k, self.alpha
        sz, nb1 = 2 * level * N, len(self.bgs) + 1
        imgs = []
        for ct, dct in zip(self.cts, self.cdev):
            terms = [ct[None]]
            if self.bgs:
                rots = poisoned(len(self.bgs) * batch * sz)
                ctx.rotate_many_grouped(Lk, level, k, alpha, [d.ptr for d in self.bdev], self.nd, self.bgs, dct.ptr, rots.ptr, batch)
                terms.append(rots.to_numpy((len(self.bgs), batch, 2, level, N)))
            img = dev(np.concatenate(terms))                                       # [nb1][batch][2][level][N]
            ctx.nntt(img.ptr, img.ptr, nb1 * batch * 2, level)
            imgs.append(img)
        total = None
        for j in range(len(self.ggs) + 1):
            a, b, keep = [], [], []
            for m, img in enumerate(imgs):
                for i in range(nb1):
                    bd = tf.DeviceBuffer(batch * sz)
                    tf.native.check(tf.native.lib().tfhe_broadcast_poly(ctx.h, bd.ptr, self.ddev[m].ptr + (j * nb1 + i) * level * N * 8, level * N, batch * 2))
                    a.append(img.ptr + i * batch * sz * 8)
                    b.append(bd.ptr)
                    keep.append(bd)
            inner = poisoned(batch * sz)
            ctx.dot(None, a, b, inner.ptr, batch * 2, level)
            ctx.inntt(inner.ptr, inner.ptr, batch * 2, level)
            if j == 0:
                total = inner
                continue
            rot, plain = poisoned(batch * sz), dev(self.gk[j - 1])
            ctx.rotate_grouped(Lk, level, k, alpha, plain.ptr, self.nd, self.ggs[j - 1], inner.ptr, rot.ptr, batch)
            ctx.add(total.ptr, rot.ptr, total.ptr, batch * 2, level)
        if self.bias is not None:
            full = np.zeros((batch, 2, level, N), dtype=np.uint64)
            full[:, 0] = self.bias
            fb = dev(full)
            ctx.add(total.ptr, fb.ptr, total.ptr, batch * 2, level)
        return total.to_numpy((batch, 2, level, N))


def check(c, want=None, chain=True):
    got = c.run()
    want = c.oracle() if want is None else want
    assert np.array_equal(got, want), (c.N, c.k, c.alpha, c.level, c.batch, len(c.bgs), len(c.ggs), len(c.cts), int((got != want).sum()))
    if chain:
        assert np.array_equal(got, c.chain()), "the composition chain"
    return got


# ---- 1. against the oracle and against the composition chain --------------------------------------------------------------------

@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("n_in", [1, 3])
@pytest.mark.parametrize("n_giant", [0, 1, 2, 4])
@pytest.mark.parametrize("n_baby", [0, 1, 3])
def test_counts_of_steps_inputs_bias_and_batch(n_baby, n_giant, n_in, bias, batch):
    """N = 64, K = 2, digits of two limbs at level 5 (the last group ragged); four giant steps are five sums: a full tile of four and
    a ragged one; three inputs run the seeded accumulation"""
    N, k, alpha, level = 64, 2, 2, 5
    check(Case(N, H.chain(30, 8, N), k, alpha, level, n_baby, n_giant, n_in, batch, bias, seed=n_baby + n_giant))


# ---- 2. every number of special primes, one digit, two policies, region 0 ---------------------------------------------------------

@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_every_number_of_special_primes(k):
    N, alpha, level = 64, 2, 3
    check(Case(N, H.chain(30, level + 1 + k, N), k, alpha, level, 2, 2, 2, 2, True, seed=k))


def _mixed12(N):
    """60-bit first limb and special primes around 40-bit limbs, as the example's ring: the wide and the narrow kernels side by side"""
    return H.chain(60, 1, N) + H.chain(40, 3, N) + H.chain(60, 3, N)[1:]


@pytest.mark.parametrize("N,ring,k,alpha,level,batch,n_baby,n_giant,n_in", [
    pytest.param(256, lambda N: H.chain(61, 6, N), 2, 4, 4, 2, 2, 1, 2, id="256-61bit-one-digit-fold-path"),
    pytest.param(1 << 12, lambda N: H.chain(50, 7, N), 2, 2, 5, 2, 2, 1, 1, id="4096-5x50-k2-a2"),
    pytest.param(1 << 12, _mixed12, 2, 2, 4, 2, 2, 1, 1, id="4096-60+3x40-2x60-mixed-ring"),
    pytest.param(1 << 15, lambda N: H.chain(40, 5, N), 2, 2, 3, 2, 1, 1, 1, id="32768-3x40-k2-a2-region-0"),
])
def test_shapes(N, ring, k, alpha, level, batch, n_baby, n_giant, n_in):
    check(Case(N, ring(N), k, alpha, level, n_baby, n_giant, n_in, batch, True, seed=3), chain=N <= 1 << 12)


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,bits", [(64, 30), (1 << 12, 50)])
def test_without_giant_steps_it_is_the_inverse_transform_of_the_diagonal_product(N, bits):
    k, alpha, level, batch = 2, 2, 5, 2
    c = Case(N, H.chain(bits, 8, N), k, alpha, level, 3, 0, 1, batch, seed=5)
    got = c.run()
    out = poisoned(batch * 2 * level * N)
    c.ctx.matmul_diag_grouped(c.Lk, level, k, alpha, [d.ptr for d in c.bdev], c.nd, c.bgs, c.ddev[0].ptr, c.cdev[0].ptr, out.ptr, batch)
    c.ctx.inntt(out.ptr, out.ptr, batch * 2, level)
    assert np.array_equal(got, out.to_numpy((batch, 2, level, N)))


@pytest.mark.parametrize("special", [1, 0])
@pytest.mark.parametrize("N,bits", [(64, 30), (1 << 12, 50)])
def test_one_limb_per_digit_is_tfhe_matmul_bsgs_blocks_on_the_same_prepared_keys(N, bits, special):
    Lk = 4
    qs = H.chain(bits, Lk, N)
    level, batch = Lk - special, 2
    c = Case(N, qs, special, 1, level, 2, 2, 2, batch, True, seed=7)
    # (tfhe_matmul_bsgs_blocks reads `level` components: operands' spare one is the special prime's)
    c.bk, c.gk = [e[:level] for e in c.bk], [e[:level] for e in c.gk]
    c.bdev = [prepare(c.ctx, Lk, e, g) for e, g in zip(c.bk, c.bgs)]
    c.gdev = [prepare(c.ctx, Lk, e, g) for e, g in zip(c.gk, c.ggs)]
    c.nd = level
    got = c.run()
    out = poisoned(batch * 2 * level * N)
    c.ctx.matmul_bsgs_blocks(Lk, level, special, [d.ptr for d in c.bdev], c.bgs, [d.ptr for d in c.gdev], c.ggs, level, [d.ptr for d in c.ddev],
                             [x.ptr for x in c.cdev], c.bdevbuf.ptr, out.ptr, batch)
    assert np.array_equal(got, out.to_numpy((batch, 2, level, N))), (N, special)


# ---- 4. chunks and the workspace --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (1 << 12, lambda N: H.chain(50, 6, N), 2, 3, 4)])
def test_batch_five_under_every_chunk_cap(N, ring, k, alpha, level):
    c = Case(N, ring(N), k, alpha, level, 2, 2, 2, 5, True, seed=2)
    want = c.oracle()
    for n in (1, 2, 3, 4, 5, 0):
        with cap(c.ctx, n):
            check(c, want=want, chain=False)
    # an empty batch leaves `out` untouched
    out = poisoned(2 * level * N)
    c.batch = 0
    c.call(out)
    c.ctx.sync()
    assert (out.to_numpy() == POISON).all()


@pytest.mark.parametrize("N,ring,k,alpha,level", [(1 << 12, lambda N: H.chain(50, 6, N), 2, 2, 3), (1 << 15, lambda N: H.chain(40, 5, N), 2, 2, 3)])
def test_on_a_dirty_workspace(N, ring, k, alpha, level):
    qs = ring(N)
    ctx = tf.Context(N, qs)                                  # a context of its own: the block is this call's
    c = Case(N, qs, k, alpha, level, 1, 1, 2, 3, True, seed=4, ctx=ctx)
    want = c.oracle()
    out = tf.DeviceBuffer(c.batch * 2 * level * N)
    on_dirty_workspace(ctx, lambda: c.call(out), out, want, moduli=qcol(qs[:level]))
    with cap(ctx, 2):
        on_dirty_workspace(ctx, lambda: c.call(out), out, want, moduli=qcol(qs[:level]))


# ---- 5. edge words ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,ring,k,alpha,level", [(64, lambda N: H.chain(30, 8, N), 2, 2, 5), (256, lambda N: H.chain(61, 6, N), 2, 4, 4)])
def test_every_word_q_minus_1_and_the_planted_group_integers(N, ring, k, alpha, level):
    qs = ring(N)
    check(Case(N, qs, k, alpha, level, 2, 1, 2, 2, True, edge=True))
    check(Case(N, qs, k, alpha, level, 2, 1, 2, 2, True, edge=True, planted=True))
    check(Case(N, qs, k, alpha, level, 2, 1, 2, 2, True, seed=1, planted=True))


# ---- 6. limits and refusals ---------------------------------------------------------------------------------------------------------

def test_64_baby_steps_are_accepted_and_65_refused():
    N, k, alpha, level = 64, 2, 2, 5
    qs = H.chain(30, 8, N)
    c = Case(N, qs, k, alpha, level, 64, 1, 1, 1, seed=9)
    check(c, chain=False)
    out = poisoned(2 * level * N)
    dd = dev(H.rand_residues(np.random.default_rng(0), qs[:level], (2, 66), N))
    with pytest.raises(AssertionError, match="n_baby=65"):
        c.ctx.matmul_bsgs_grouped(c.Lk, level, k, alpha, [c.bdev[0].ptr] * 65, [5] * 65, [c.gdev[0].ptr], c.ggs, c.nd, [dd.ptr], [c.cdev[0].ptr], None,
                                  out.ptr, 1)
    with pytest.raises(AssertionError, match="n_giant=65"):
        c.ctx.matmul_bsgs_grouped(c.Lk, level, k, alpha, [c.bdev[0].ptr], [5], [c.gdev[0].ptr] * 65, [5] * 65, c.nd, [dd.ptr], [c.cdev[0].ptr], None,
                                  out.ptr, 1)
    c.ctx.sync()
    assert (out.to_numpy() == POISON).all()


def test_host_checks_in_the_headers_order_leave_the_output_untouched():
    N = 64
    qs = H.chain(30, 6, N)
    ctx, _ = pair(N, qs)
    words = 2 * 4 * N                                       # one ciphertext at level 4
    buf, other = poisoned(16 * words), poisoned(8 * words)
    p, o = buf.ptr, other.ptr

    def f(baby=(p, p), bgs=(3, 5), giant=(p,), ggs=(127,), Lk=6, level=4, k=2, group=2, nd=2, diags=(p,), cts=(p,), bias=None, out=o, batch=1):
        ctx.matmul_bsgs_grouped(Lk, level, k, group, list(baby), list(bgs), list(giant), list(ggs), nd, list(diags), list(cts), bias, out, batch)
    with pytest.raises(AssertionError, match="null argument"):
        f(out=None, Lk=0)
    with pytest.raises(AssertionError, match="null baby key 1"):
        f(baby=(p, None), Lk=0)
    with pytest.raises(AssertionError, match="null giant key 0"):
        f(giant=(None,), bgs=(4, 4))
    with pytest.raises(AssertionError, match="null ciphertext of input 1"):
        f(diags=(p, p), cts=(p, None), Lk=0)
    with pytest.raises(AssertionError, match="n_in=0"):
        f(diags=(), cts=(), Lk=0)
    with pytest.raises(AssertionError, match="key_limbs"):
        f(Lk=7, bgs=(4, 4))
    with pytest.raises(AssertionError, match="n_special"):
        f(k=5, group=0)
    with pytest.raises(AssertionError, match="group"):
        f(group=0, level=0)
    with pytest.raises(tf.UsageError, match="level"):
        f(level=5, nd=0)
    with pytest.raises(tf.UsageError, match="components"):
        f(nd=1, batch=-1)
    with pytest.raises(AssertionError, match="negative batch"):
        f(batch=-1, ggs=(4,))
    for g in (4, 2 * N, 2 * N + 1):
        with pytest.raises(AssertionError, match="odd and below 2N"):
            f(bgs=(3, g), out=p)                            # ahead of the overlap
        with pytest.raises(AssertionError, match="odd and below 2N"):
            f(ggs=(g,), out=p)
    with pytest.raises(tf.UsageError, match="level"):
        f(baby=(), bgs=(), giant=(), ggs=(), level=5)       # no key: the shape checks run once
    for out in (p, p + (words - 1) * 8, p + (2 * 3 * 4 * N - 1) * 8):     # the ciphertext's first and last word; the diagonals' last
        with pytest.raises(AssertionError, match="overlaps"):
            f(out=out)
    with pytest.raises(AssertionError, match="overlaps"):
        f(bias=o + (words - 1) * 8)                         # the last word of out is the first of the bias
    with pytest.raises(AssertionError, match="overlaps"):
        f(out=p, batch=0)                                   # ahead of the empty batch
    ctx.sync()
    assert (buf.to_numpy() == POISON).all() and (other.to_numpy() == POISON).all()


# ---- 7. the coefficient route, in a process of its own (the flag is read once per process) ------------------------------------------

CHILD = r"""
import numpy as np
from tests import helpers as H
from tests.test_gpu_matmul_bsgs_grouped import Case, check
from tests.test_gpu_ks_grouped import poisoned
N, k, alpha, level = 64, 2, 2, 5
c = Case(N, H.chain(30, 8, N), k, alpha, level, 3, 4, 3, 3, True, seed=11)
check(c)
d = Case(N, H.chain(30, 8, N), k, alpha, level, 3, 0, 1, 2, seed=12)
out = poisoned(2 * 2 * level * N)
d.ctx.matmul_diag_grouped(d.Lk, level, k, alpha, [x.ptr for x in d.bdev], d.nd, d.bgs, d.ddev[0].ptr, d.cdev[0].ptr, out.ptr, 2)
d.ctx.inntt(out.ptr, out.ptr, 4, level)
assert np.array_equal(d.run(), out.to_numpy((2, 2, level, N)))
assert np.array_equal(d.run(), d.oracle())
print("RESULT ok")
"""


def test_coefficient_route_gives_the_same_words():
    env = dict(os.environ, TFHE_MD_COEFF="1")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "RESULT ok" in r.stdout


# ---- 8. the mirror, end to end ------------------------------------------------------------------------------------------------------

def test_mirror_product_decrypts_within_the_per_limb_products_error():
    """GroupedRaised(CKKSParams, 2, 2) at N = 2^12: a 4 x 4 matrix in blocks of N / 8 slots by n1 = 2: one baby and one giant step.
    tf.matmul_bsgs_grouped decrypts to the plain product.  Tolerance: the margin of
    tests/test_gpu_rotate_many_grouped.py::test_mirror_product_decrypts_within_the_per_limb_products_error -- 4 x the error tf.matmul_bsgs
    makes on a ModulusRaised key set of the same ciphertext ring and scale, measured here, plus what one grouped key-switch step may add per
    rotation by the bound tests/test_gpu_ks_grouped.py derives,
        d N (max Q_g // 2 + 1) max|e| // P + 1 + k (1 + N max|s|)      coefficient units of the rotated ciphertext,
    with max|e|, max|s| <= 20, carried to the slots: a coefficient error of at most B moves a slot by at most N B / scale.  Baby
    rotation i enters inner sum j weighted by max |diagonal j, i| (a giant rotation permutes slots and keeps magnitudes), summed over the
    giant steps; a giant rotation acts on an inner sum at the squared scale, so its own step adds N B / scale^2 with weight 1."""
    N = 1 << 12
    qs = H.chain(40, 3, N) + H.chain(41, 2, N)
    scale = 2**40
    n, n1 = 4, 2
    B = N // 2 // n
    rng = np.random.default_rng(34)
    x = rng.normal(0, 1, N // 2)
    Wm = rng.normal(0, 1, (n, n))
    dv = np.array([np.repeat(np.array([Wm[i, (i - k) % n] for i in range(n)]), B) for k in range(n)])
    want = Wm @ x.reshape(n, B)
    D, baby_steps, giant_steps = tf.bsgs_diagonals(dv, n1, B)

    def product(params, matmul):
        kp = tf.keygen(rng, params)
        c = tf.encrypt(rng, kp, tf.ckks_encode(x.astype(complex), params.R_cipher(), scale), scale=scale)
        bk = [tf.keygen_galois(rng, kp.priv, steps=s) for s in baby_steps]
        gk = [tf.keygen_galois(rng, kp.priv, steps=s) for s in giant_steps]
        res = matmul(bk, gk, tf.ckks_encode(D.reshape(-1, N // 2).astype(complex), params.R_cipher(), scale), c)
        got = tf.ckks_decode(tf.decrypt(kp, res), res.scale).real.reshape(n, B)
        return float(np.abs(got - want).max()), bk, gk, c

    grouped = tf.GroupedRaised(tf.CKKSParams(tf.NegacyclicRing(N, qs), 0, 3.2), 2, 2)
    raised = tf.ModulusRaised(tf.CKKSParams(tf.NegacyclicRing(N, qs[:4]), 0, 3.2))
    assert grouped.R_cipher().moduli == raised.R_cipher().moduli == qs[:3]
    err_g, gbk, ggk, gc = product(grouped, tf.matmul_bsgs_grouped)
    err_m, mbk, mgk, mc = product(raised, tf.matmul_bsgs)
    level, k, alpha = 3, 2, 2
    groups = KO.groups(level, alpha)
    step = len(groups) * N * (max(math.prod(qs[i] for i in G) for G in groups) // 2 + 1) * 20 // math.prod(qs[-k:]) + 1 + k * (1 + N * 20)
    weight = sum(float(np.abs(D[j, i]).max()) for j in range(D.shape[0]) for i in range(1, D.shape[1]))
    bound = 4 * err_m + weight * N * step / scale + len(giant_steps) * N * step / scale**2
    print(f"max |error|: matmul_bsgs_grouped {err_g:.3e}, matmul_bsgs (ModulusRaised) {err_m:.3e}, bound {bound:.3e}")
    assert err_g <= bound, (err_g, err_m, bound)
    # the block form with one input and no bias is the same call
    dd = tf.ckks_encode(D.reshape(-1, N // 2).astype(complex), grouped.R_cipher(), scale)
    one, blocks = tf.matmul_bsgs_grouped(gbk, ggk, dd, gc), tf.matmul_bsgs_blocks_grouped(gbk, ggk, [dd], [gc])
    assert all(np.array_equal(a.coeffs_primal().to_numpy(), b.coeffs_primal().to_numpy()) for a, b in zip(one.cs, blocks.cs))
    # the per-limb calls keep refusing grouped keys, the new ones refuse per-limb keys
    for refused in (lambda: tf.matmul_bsgs(gbk, ggk, dd, gc), lambda: tf.matmul_bsgs_blocks(gbk, ggk, [dd], [gc])):
        with pytest.raises(tf.UsageError, match="grouped digits"):
            refused()
    md = tf.ckks_encode(D.reshape(-1, N // 2).astype(complex), raised.R_cipher(), scale)
    for refused in (lambda: tf.matmul_bsgs_grouped(mbk, mgk, md, mc), lambda: tf.matmul_bsgs_blocks_grouped(mbk, mgk, [md], [mc])):
        with pytest.raises(tf.UsageError, match="grouped digits"):
            refused()
