"""tfhe_rotate_sum_grouped / tfhe_matmul_bsgs_fold_grouped on the device, word for word, every word read back below its modulus and
`out` pre-filled with 0xA5..: at N <= 2^13 against tests/rotate_sum_grouped_oracle.py AND against the C-ABI chain the header states --
per fold step tfhe_rotate_many_grouped over the step's keys on F_t -> tfhe_add of every result onto F_t; for the product
tfhe_matmul_bsgs_grouped (bias = NULL) -> that fold -> tfhe_add of the bias --, at N >= 2^15 against the chain alone (its links are
oracle-checked in their own files).  Step shapes over every (n_special, group) class; the limits; modulus edges; the gather's team
split and the finish's two widths; levels below the key's; the 32-limb seam; the product on two rings; large N under two transform
variants; the identities with the per-limb entry points; chunk seams; a dirty workspace; the refusals; and the mirror.  The families
name no route: a process runs them on the default (the fold on the coefficient route: no new kernel), and section 10 runs them again
in fresh processes under TFHE_MDG_FOLD_EVAL=1, where every fold step goes through k_mdg_fold_gather and k_mdg_fold_finish."""
import os
import subprocess
import sys

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from tests import helpers as H
from tests import rotate_sum_grouped_oracle as FO
from tests.dirty_ws import on_dirty_workspace
from tests.test_gpu_chunk_seams import cap
from tests.test_gpu_ks_grouped import dev, operands, pair, poisoned, qcol
from tests.test_gpu_matmul_bsgs_grouped import Case
from tests.test_gpu_modulus_edges import edge
from tests.test_gpu_rotate_many_grouped import g_many, prepare

pytestmark = pytest.mark.gpu
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fold_elements(N, steps, first=1):
    """distinct odd elements for the fold keys, step by step; the last key of a step of two or more flips every sign but one, the first
    key of the last step wraps many times"""
    gs, e = [], first
    for t, size in enumerate(steps):
        st = []
        for u in range(size):
            st.append(pow(5, e, 2 * N))
            e += 1
        if size >= 2:
            st[-1] = 2 * N - 1
        if t + 1 == len(steps) and t > 0:
            st[0] = g_many(N)
        gs.append(st)
    return gs


class Fold:
    """the fold keys of one call: at most three distinct plain keys dealt round robin (the oracle's), prepared once per (key, element)"""

    def __init__(self, ctx, N, qs, k, alpha, level, steps, seed=0, edge_words=False, spare=1):
        self.steps = list(steps)
        self.gs = fold_elements(N, steps)
        flat = [g for st in self.gs for g in st]
        n_keys = min(len(flat), 3)
        plain = [operands(N, qs, k, alpha, level, 2, 1, seed=seed + 101 + 17 * i, edge=edge_words, spare=spare)[0] for i in range(n_keys)]
        made, self.plain, self.dev = {}, [], []
        r = 0
        for st in self.gs:
            ps, ds = [], []
            for g in st:
                key = (r % n_keys, int(g))
                if key not in made:
                    made[key] = prepare(ctx, len(qs), plain[r % n_keys], g)
                ps.append(plain[r % n_keys])
                ds.append(made[key])
                r += 1
            self.plain.append(ps)
            self.dev.append(ds)
        self.nd = plain[0].shape[0] if plain else -(-level // alpha) + spare

    def ptrs(self):
        return [[d.ptr for d in st] for st in self.dev]

    def chain(self, ctx, Lk, level, k, alpha, N, f, batch):
        """per step tfhe_rotate_many_grouped on F_t -> tfhe_add of every result onto F_t, in place in the device buffer `f`"""
        sz = batch * 2 * level * N
        for st, gs in zip(self.dev, self.gs):
            rots = poisoned(len(st) * sz)
            ctx.rotate_many_grouped(Lk, level, k, alpha, [d.ptr for d in st], self.nd, gs, f.ptr, rots.ptr, batch)
            for u in range(len(st)):
                ctx.add(f.ptr, rots.ptr + u * sz * 8, f.ptr, batch * 2, level)
        return f


class SumCase:
    """tfhe_rotate_sum_grouped on a uniform (or edge) ciphertext batch"""

    def __init__(self, N, qs, k, alpha, level, steps, batch=2, seed=0, edge_words=False, ctx=None, spare=1):
        self.N, self.qs, self.k, self.alpha, self.level, self.batch, self.Lk = N, list(qs), k, alpha, level, batch, len(qs)
        self.ctx, self.ref = pair(N, qs)
        if ctx is not None:
            self.ctx = ctx
        self.fold = Fold(self.ctx, N, qs, k, alpha, level, steps, seed, edge_words, spare)
        self.ct = operands(N, qs, k, alpha, level, 2, batch, seed=seed + 7, edge=edge_words)[1]
        self.dct = dev(self.ct)

    def call(self, out, ptr=None):
        self.ctx.rotate_sum_grouped(self.Lk, self.level, self.k, self.alpha, self.fold.ptrs(), self.fold.gs, self.fold.nd, self.dct.ptr,
                                    out.ptr if ptr is None else ptr, self.batch)

    def run(self, misaligned=False):
        words = self.batch * 2 * self.level * self.N
        out = poisoned(words + 1)
        self.call(out, out.ptr + 8 if misaligned else None)     # `out` 8 bytes off a 16-byte boundary: the last step's finish at V = 1
        got = out.to_numpy()
        assert got[0 if misaligned else words] == POISON
        got = got[1:] if misaligned else got[:words]
        got = got.reshape(self.batch, 2, self.level, self.N)
        assert (got < qcol(self.qs[:self.level])).all()
        return got

    def oracle(self):
        return FO.rotate_sum_grouped_ref(self.ref, self.level, self.k, self.alpha, self.fold.plain, self.fold.gs, self.ct)

    def chain(self):
        f = self.fold.chain(self.ctx, self.Lk, self.level, self.k, self.alpha, self.N, dev(self.ct), self.batch)
        return f.to_numpy((self.batch, 2, self.level, self.N))


def check_sum(c, oracle=True, misaligned=False):
    got = c.run(misaligned)
    want = c.chain()
    assert np.array_equal(got, want), ("the chain", c.N, c.k, c.alpha, c.level, c.batch, c.fold.steps, int((got != want).sum()))
    if oracle:
        assert np.array_equal(got, c.oracle()), ("the oracle", c.N, c.k, c.alpha, c.level, c.batch, c.fold.steps)
    return got


class ProductCase(Case):
    """tfhe_matmul_bsgs_fold_grouped: the operands of tests/test_gpu_matmul_bsgs_grouped.py plus fold steps"""

    def __init__(self, N, qs, k, alpha, level, n_baby, n_giant, n_in, steps, batch=2, bias=True, seed=0, ctx=None):
        super().__init__(N, qs, k, alpha, level, n_baby, n_giant, n_in, batch, bias, seed=seed, ctx=ctx)
        self.fold = Fold(self.ctx, N, qs, k, alpha, level, steps, seed)
        if not (self.bk or self.gk):
            self.nd = self.fold.nd

    def call(self, out):
        self.ctx.matmul_bsgs_fold_grouped(self.Lk, self.level, self.k, self.alpha, [d.ptr for d in self.bdev], self.bgs, [d.ptr for d in self.gdev],
                                          self.ggs, self.nd, [d.ptr for d in self.ddev], [c.ptr for c in self.cdev], self.fold.ptrs(), self.fold.gs,
                                          None if self.bdevbuf is None else self.bdevbuf.ptr, out.ptr, self.batch)

    def oracle(self):
        return FO.matmul_bsgs_fold_grouped_ref(self.ref, self.level, self.k, self.alpha, self.bk, self.bgs, self.gk, self.ggs, self.diags, self.cts,
                                               self.fold.plain, self.fold.gs, bias=self.bias)

    def chain(self):
        """tfhe_matmul_bsgs_grouped (bias = NULL) -> the fold's chain -> tfhe_add of the bias onto component 0"""
        level, N, batch = self.level, self.N, self.batch
        f = poisoned(batch * 2 * level * N)
        self.ctx.matmul_bsgs_grouped(self.Lk, level, self.k, self.alpha, [d.ptr for d in self.bdev], self.bgs, [d.ptr for d in self.gdev], self.ggs,
                                     self.nd, [d.ptr for d in self.ddev], [c.ptr for c in self.cdev], None, f.ptr, batch)
        self.fold.chain(self.ctx, self.Lk, level, self.k, self.alpha, N, f, batch)
        if self.bias is not None:
            full = np.zeros((batch, 2, level, N), dtype=np.uint64)
            full[:, 0] = self.bias
            fb = dev(full)
            self.ctx.add(f.ptr, fb.ptr, f.ptr, batch * 2, level)
        return f.to_numpy((batch, 2, level, N))


def check_product(c, oracle=True):
    got = c.run()
    want = c.chain()
    assert np.array_equal(got, want), ("the chain", c.N, c.k, c.alpha, c.level, c.fold.steps, int((got != want).sum()))
    if oracle:
        assert np.array_equal(got, c.oracle()), ("the oracle", c.N, c.k, c.alpha, c.level, c.fold.steps)
    return got


# ---- 1. step shapes over every class of (n_special, group) ------------------------------------------------------------------------

@pytest.mark.parametrize("k,alpha", [(0, 1), (1, 1), (1, 2), (2, 2), (3, 3), (4, 2)])
@pytest.mark.parametrize("steps", [(1,), (1, 1), (3,), (2, 1), (1, 3, 1)])
def test_step_shapes(steps, k, alpha):
    """N = 2^8 on three 40-bit limbs: one limb per digit without and with a special prime, a ragged last digit (group 2), one digit in
    all (group 3), every number of special primes 0 .. 4; `out` on and 8 bytes off a 16-byte boundary (on the evaluation route: the
    last step's finish at V = 2 and at V = 1 for every K)"""
    N, level = 256, 3
    c = SumCase(N, H.chain(40, level + k, N), k, alpha, level, steps, batch=2, seed=len(steps))
    got = check_sum(c)
    assert np.array_equal(c.run(misaligned=True), got)


# ---- 2. the limits ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [(64,), (1,) * 64])
def test_64_keys_in_one_step_and_64_steps_of_one(steps):
    N, k, alpha, level = 64, 2, 2, 3
    check_sum(SumCase(N, H.chain(30, level + k, N), k, alpha, level, steps, batch=1, seed=2))


# ---- 3. modulus edges --------------------------------------------------------------------------------------------------------------------

def _mixed_policy(N):
    return edge("fp-top", 1, N) + edge("u64-bottom", 1, N) + edge("top62", 1, N) + edge("fold62", 1, N) + edge("fp-top", 2, N)[1:]


@pytest.mark.parametrize("name,logn,ring", [
    ("top62", 10, lambda N: edge("top62", 5, N)), ("fold62", 10, lambda N: edge("fold62", 5, N)),
    ("fp-top", 12, lambda N: edge("fp-top", 5, N)), ("u64-bottom", 12, lambda N: edge("u64-bottom", 5, N)), ("mixed-policy", 12, _mixed_policy)])
def test_modulus_edges(name, logn, ring):
    """(n_special, group) = (2, 2) at level 3; uniform words and every word q - 1"""
    N = 1 << logn
    qs = ring(N)
    check_sum(SumCase(N, qs, 2, 2, 3, (2, 1), batch=1, seed=3))
    check_sum(SumCase(N, qs, 2, 2, 3, (2, 1), batch=1, edge_words=True))


# ---- 4. the gather's team split and the finish's two widths --------------------------------------------------------------------------------

@pytest.mark.parametrize("logn", [4, 8, 11, 13])
def test_gathers_team_split_and_both_widths_of_the_finish(logn):
    """two 50-bit limbs, K = 2; `out` on and 8 bytes off a 16-byte boundary.  On the evaluation route (section 10): rows shorter than
    one workgroup's block, one team per row pair and several workgroups per row in the gather, the last step's finish with 16-byte and
    with 8-byte loads and stores.  On the default route the same sizes go through the hoisted rotations' tail"""
    N, k, alpha, level = 1 << logn, 2, 2, 2
    c = SumCase(N, H.chain(50, level + k, N), k, alpha, level, (2, 1), batch=3 if logn <= 8 else 1, seed=logn)
    got = check_sum(c)
    assert np.array_equal(c.run(misaligned=True), got)


# ---- 5. below the key's level; the 32-limb seam ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [1, 2])
def test_levels_below_the_keys(level):
    """a key of four ciphertext limbs and two special primes, digits of two limbs: the ciphertext at levels 1 and 2 (a digit cut short)"""
    N, k, alpha = 256, 2, 2
    qs = H.chain(40, 6, N)
    c = SumCase(N, qs, k, alpha, level, (2, 1), batch=2, seed=level, spare=2 - (-(-level // alpha)) + 1)
    check_sum(c)


@pytest.mark.parametrize("nw,k", [(32, 2), (33, 3), (40, 4)])
def test_the_32_limb_seam(nw, k):
    """level + n_special = 32, 33 and 40 at N = 2^5: the limb masks' seam; on the evaluation route five (level 30) and six (level 36) blocks of limbs
    in the finish"""
    N, alpha = 32, 4
    level = nw - k
    check_sum(SumCase(N, H.chain(30, nw, N), k, alpha, level, (2, 1), batch=1, seed=nw))


# ---- 6. the product ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ring,k,alpha,level", [(lambda N: H.chain(30, 8, N), 2, 2, 5), (lambda N: H.chain(61, 1, N) + H.chain(40, 3, N) + H.chain(41, 3, N), 3, 3, 4)])
@pytest.mark.parametrize("steps", [(1, 1), (3,), ()])
def test_product_with_bias_and_fold_steps(steps, ring, k, alpha, level):
    N = 64
    check_product(ProductCase(N, ring(N), k, alpha, level, 2, 2, 2, steps, batch=2, bias=True, seed=len(steps)))


@pytest.mark.parametrize("ring,k,alpha,level", [(lambda N: H.chain(30, 8, N), 2, 2, 5), (lambda N: H.chain(61, 1, N) + H.chain(40, 3, N) + H.chain(41, 3, N), 3, 3, 4)])
def test_product_of_one_baby_step_no_giant_step_no_bias(ring, k, alpha, level):
    N = 64
    check_product(ProductCase(N, ring(N), k, alpha, level, 1, 0, 1, (1,), batch=2, bias=False, seed=5))


def test_product_without_fold_steps_is_tfhe_matmul_bsgs_grouped():
    N, k, alpha, level = 64, 2, 2, 5
    c = ProductCase(N, H.chain(30, 8, N), k, alpha, level, 2, 1, 2, (), batch=2, bias=True, seed=6)
    got = c.run()
    out = poisoned(c.batch * 2 * level * N)
    Case.call(c, out)
    assert np.array_equal(got, out.to_numpy((c.batch, 2, level, N)))


# ---- 7. large N --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [(2,), (1,)])
@pytest.mark.parametrize("logn", [15, 16])
def test_large_rings_under_both_transform_variants(logn, steps):
    """N = 2^15 and 2^16, batch 1, three 40-bit limbs and two special primes: region 0 in use; against the device chain"""
    N, k, alpha, level = 1 << logn, 2, 2, 3
    c = SumCase(N, H.chain(40, level + k, N), k, alpha, level, steps, batch=1, seed=logn)
    try:
        for variant in (0, 2):
            c.ctx.set_ntt_variant(variant)
            check_sum(c, oracle=False)
    finally:
        c.ctx.set_ntt_variant(0)


# ---- 8. identities ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("special", [1, 0])
@pytest.mark.parametrize("N,bits", [(64, 30), (1 << 12, 50)])
def test_one_limb_per_digit_is_the_per_limb_entry_points_on_the_same_prepared_keys(N, bits, special):
    Lk = 4
    qs = H.chain(bits, Lk, N)
    level, batch = Lk - special, 2
    c = ProductCase(N, qs, special, 1, level, 2, 1, 2, (2, 1), batch=batch, bias=True, seed=7)
    # (the per-limb entry points read `level` components: operands' spare one is dropped)
    c.bk, c.gk = [e[:level] for e in c.bk], [e[:level] for e in c.gk]
    c.bdev = [prepare(c.ctx, Lk, e, g) for e, g in zip(c.bk, c.bgs)]
    c.gdev = [prepare(c.ctx, Lk, e, g) for e, g in zip(c.gk, c.ggs)]
    c.fold.plain = [[e[:level] for e in st] for st in c.fold.plain]
    c.fold.dev = [[prepare(c.ctx, Lk, e, g) for e, g in zip(st, gs)] for st, gs in zip(c.fold.plain, c.fold.gs)]
    c.nd = c.fold.nd = level
    got = c.run()
    out = poisoned(batch * 2 * level * N)
    c.ctx.matmul_bsgs_fold(Lk, level, special, [d.ptr for d in c.bdev], c.bgs, [d.ptr for d in c.gdev], c.ggs, level, [d.ptr for d in c.ddev],
                           [x.ptr for x in c.cdev], c.fold.ptrs(), c.fold.gs, c.bdevbuf.ptr, out.ptr, batch)
    assert np.array_equal(got, out.to_numpy((batch, 2, level, N))), (N, special, "product")
    a, b = poisoned(batch * 2 * level * N), poisoned(batch * 2 * level * N)
    c.ctx.rotate_sum_grouped(Lk, level, special, 1, c.fold.ptrs(), c.fold.gs, level, c.cdev[0].ptr, a.ptr, batch)
    c.ctx.rotate_sum(Lk, level, special, c.fold.ptrs(), c.fold.gs, level, c.cdev[0].ptr, b.ptr, batch)
    assert np.array_equal(a.to_numpy(), b.to_numpy()), (N, special, "fold")


def test_without_a_fold_step_the_fold_is_a_copy():
    N, k, alpha, level = 64, 2, 2, 3
    c = SumCase(N, H.chain(30, 5, N), k, alpha, level, (), batch=3)
    assert np.array_equal(c.run(), c.ct)


# ---- 9. chunk seams, a dirty workspace --------------------------------------------------------------------------------------------------------

def test_chunk_cap_one_at_batch_three():
    N, k, alpha, level = 256, 2, 2, 3
    qs = H.chain(40, 5, N)
    s = SumCase(N, qs, k, alpha, level, (2, 1), batch=3, seed=8)
    p = ProductCase(N, qs, k, alpha, level, 1, 1, 2, (2, 1), batch=3, bias=True, seed=8)
    want_s, want_p = s.run(), p.run()
    assert np.array_equal(want_s, s.oracle()) and np.array_equal(want_p, p.oracle())
    for n in (1, 2):
        with cap(s.ctx, n):
            assert np.array_equal(s.run(), want_s), n
        with cap(p.ctx, n):
            assert np.array_equal(p.run(), want_p), n
    out = poisoned(2 * level * N)                              # an empty batch leaves `out` untouched
    s.batch = p.batch = 0
    s.call(out)
    p.call(out)
    s.ctx.sync()
    assert (out.to_numpy() == POISON).all()


@pytest.mark.parametrize("logn", [8, 15])
def test_on_a_dirty_workspace(logn):
    N, k, alpha, level = 1 << logn, 2, 2, 3
    qs = H.chain(40, 5, N)
    ctx = tf.Context(N, qs)                                    # a context of its own: the block is this call's
    s = SumCase(N, qs, k, alpha, level, (2, 1), batch=2, seed=9, ctx=ctx)
    p = ProductCase(N, qs, k, alpha, level, 1, 1, 1, (2,), batch=2, bias=True, seed=9, ctx=ctx)
    for c in (s, p):
        want = c.chain()
        if logn <= 13:
            assert np.array_equal(want, c.oracle())
        out = tf.DeviceBuffer(c.batch * 2 * level * N)
        on_dirty_workspace(ctx, lambda: c.call(out), out, want, moduli=qcol(qs[:level]))


# ---- 10. every family above on the route that is not the default, in processes of their own (the switches are read once per process) --------
# The tests above do not name a route: they run the one the process is on -- by default the fold on the coefficient route, which launches
# ksg_hoist_tile and k_bsgs_sum and NEITHER of the new kernels.  The tests below start this file again under TFHE_MDG_FOLD_EVAL=1
# (mdg_fold_eval, csrc/md_api.inc: every fold step with n_special >= 1 then goes through k_mdg_fold_gather and k_mdg_fold_finish<K, V>), so
# that each family's cases -- and what their docstrings say about the gather and the finish -- hold on the device for the new kernels:
# K = 1 .. 4, both widths V, up to six blocks of limbs, the team split at 2^4 .. 2^13, the edge rings, chunks shorter than the cap, a
# dirty workspace.  One more child runs a selection under TFHE_MD_COEFF=1, which puts the baby phase on the coefficient route as well.

SWITCHES = ("TFHE_MDG_FOLD_EVAL", "TFHE_MD_COEFF")


def _again(env_extra, select):
    """the tests of this file whose names match `select`, in a fresh process under `env_extra`; -> how many passed there"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
           f"({select}) and not fresh_process"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    tail = r.stdout.strip().splitlines()[-1]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail and "error" not in tail, tail
    return int(tail.split(" passed")[0].split()[-1])


EVAL = {"TFHE_MDG_FOLD_EVAL": "1"}


def test_fresh_process_evaluation_route_step_shapes_and_limits():
    """the 30 step shapes over (n_special, group) -- k_mdg_fold_finish<1 .. 4, V> at V = 2 and, for the last step, V = 1; (0, 1) has no
    evaluation route -- and the limits"""
    assert _again(EVAL, "step_shapes or 64_keys") == 32


def test_fresh_process_evaluation_route_sizes_widths_edges_and_seams():
    """the team split at N = 2^4 .. 2^13 with `out` on and off a 16-byte boundary (V = 2 and V = 1), the edge rings, the levels below the
    key's, 32 / 33 / 40 working limbs (five and six blocks of limbs in the finish, K = 2, 3, 4), N = 2^15 and 2^16 under both variants"""
    assert _again(EVAL, "modulus_edges or gathers_team_split or levels_below or 32_limb or large_rings") == 18


def test_fresh_process_evaluation_route_product_identities_chunks_and_dirty_workspace():
    """the product on two rings (K = 2 and 3), the identities with the per-limb entry points ((1, 1): K = 1), chunk caps 1 and 2 at batch 3
    (nb below the chunk sets the finish's rotation stride), a dirty workspace at 2^8 and 2^15"""
    assert _again(EVAL, "product or one_limb_per_digit or without_a_fold_step or chunk_cap or dirty_workspace") == 17


def test_fresh_process_md_coeff_gives_the_same_words():
    """TFHE_MD_COEFF=1: the baby phase and the fold both on the coefficient route"""
    assert _again({"TFHE_MD_COEFF": "1"}, "product or chunk_cap or gathers_team_split or large_rings") >= 10


# ---- 11. the refusals ------------------------------------------------------------------------------------------------------------------------

def test_host_checks_in_the_headers_order_leave_the_output_untouched():
    N = 64
    qs = H.chain(30, 6, N)
    ctx, _ = pair(N, qs)
    words = 2 * 4 * N                                       # one ciphertext at level 4
    buf, other = poisoned(16 * words), poisoned(8 * words)
    p, o = buf.ptr, other.ptr

    def f(fold=((p, p), (p,)), fgs=((9, 11), (13,)), Lk=6, level=4, k=2, group=2, nd=2, ct=p, out=o, batch=1):
        ctx.rotate_sum_grouped(Lk, level, k, group, [list(s) for s in fold], [list(s) for s in fgs], nd, ct, out, batch)

    def g(baby=(p, p), bgs=(3, 5), giant=(p,), ggs=(127,), fold=((p, p), (p,)), fgs=((9, 11), (13,)), Lk=6, level=4, k=2, group=2, nd=2, diags=(p,),
          cts=(p,), bias=None, out=o, batch=1):
        ctx.matmul_bsgs_fold_grouped(Lk, level, k, group, list(baby), list(bgs), list(giant), list(ggs), nd, list(diags), list(cts),
                                     [list(s) for s in fold], [list(s) for s in fgs], bias, out, batch)
    for call in (f, g):
        with pytest.raises(AssertionError, match="null argument"):
            call(out=None, Lk=0)
        with pytest.raises(AssertionError, match="fold group 1 has size 0"):
            call(fold=((p,), ()), fgs=((9,), ()), Lk=0)
        with pytest.raises(AssertionError, match="more than 64 fold keys"):
            call(fold=((p,) * 65,), fgs=((9,) * 65,), Lk=0)
        with pytest.raises(AssertionError, match="n_fold_groups=65"):
            call(fold=((p,),) * 65, fgs=((9,),) * 65, Lk=0)
        with pytest.raises(AssertionError, match="null fold key 1"):
            call(fold=((p, None), (p,)), Lk=0)
        with pytest.raises(AssertionError, match="key_limbs"):
            call(Lk=7, fgs=((4, 4), (4,)))
        with pytest.raises(AssertionError, match="n_special"):
            call(k=5, group=0)
        with pytest.raises(AssertionError, match="group"):
            call(group=0, level=0)
        with pytest.raises(tf.UsageError, match="level"):
            call(level=5, nd=0)
        with pytest.raises(tf.UsageError, match="components"):
            call(nd=1, batch=-1)
        with pytest.raises(AssertionError, match="negative batch"):
            call(batch=-1, fgs=((9, 11), (4,)))
        for e in (4, 2 * N, 2 * N + 1):
            with pytest.raises(AssertionError, match="odd and below 2N"):
                call(fgs=((9, 11), (e,)), out=p)             # ahead of the overlap
        for out in (p, p + (words - 1) * 8):                 # the ciphertext's first and last word
            with pytest.raises(AssertionError, match="overlaps"):
                call(out=out)
        with pytest.raises(AssertionError, match="overlaps"):
            call(out=p, batch=0)                             # ahead of the empty batch
    with pytest.raises(tf.UsageError, match="level"):
        f(fold=(), fgs=(), level=5)                          # no key: the shape checks run once
    with pytest.raises(AssertionError, match="null fold key 0"):
        g(fold=((None,),), fgs=((9,),), baby=(p, None))      # the fold's rules come before the product's
    with pytest.raises(AssertionError, match="null baby key 1"):
        g(baby=(p, None), Lk=0)
    with pytest.raises(AssertionError, match="n_in=0"):
        g(diags=(), cts=(), Lk=0)
    with pytest.raises(AssertionError, match="odd and below 2N"):
        g(bgs=(3, 4), fgs=((9, 11), (2 * N,)), out=p)
    with pytest.raises(AssertionError, match="overlaps"):
        g(out=p + (2 * 3 * 4 * N - 1) * 8)                   # the diagonals' last word
    with pytest.raises(AssertionError, match="overlaps"):
        g(bias=o + (words - 1) * 8)                          # the last word of out is the first of the bias
    ctx.sync()
    assert (buf.to_numpy() == POISON).all() and (other.to_numpy() == POISON).all()


# ---- 12. the mirror --------------------------------------------------------------------------------------------------------------------------

def test_mirror_functions_are_the_per_step_mirror_composition():
    """GroupedRaised(CKKSParams, 2, 2) at N = 2^10: tf.rotate_sum_grouped against tf.rotate_many_grouped and + step by step, word for
    word; tf.matmul_bsgs_fold_grouped against tf.matmul_bsgs_blocks_grouped -> tf.rotate_sum_grouped -> + bias, word for word; the
    per-limb mirror functions refuse the grouped keys and the grouped ones refuse per-limb keys"""
    N = 1 << 10
    qs = H.chain(40, 3, N) + H.chain(41, 2, N)
    scale = 2**30
    rng = np.random.default_rng(41)
    params = tf.GroupedRaised(tf.CKKSParams(tf.NegacyclicRing(N, qs), 0, 3.2), 2, 2)
    kp = tf.keygen(rng, params)
    x = rng.normal(0, 1, N // 2)
    c = tf.encrypt(rng, kp, tf.ckks_encode(x.astype(complex), params.R_cipher(), scale), scale=scale)
    W = rng.normal(0, 1, (2, 8))
    B = N // 2 // 8
    D, baby_steps, giant_steps, fold_steps = tf.rect_diagonals(W, 2, B, fold_radix=2)
    assert [len(s) for s in fold_steps] == [1, 1]
    bk = [tf.keygen_galois(rng, kp.priv, steps=s) for s in baby_steps]
    gk = [tf.keygen_galois(rng, kp.priv, steps=s) for s in giant_steps]
    fk = [[tf.keygen_galois(rng, kp.priv, steps=s) for s in st] for st in fold_steps]
    words = lambda ct: [e.coeffs_primal().to_numpy() for e in ct.cs]
    # the fold
    got = tf.rotate_sum_grouped(fk, c)
    f = c
    for st in fk:
        g = f
        for r in tf.rotate_many_grouped(st, f):
            g = g + r
        f = g
    assert all(np.array_equal(a, b) for a, b in zip(words(got), words(f)))
    assert got.scale == c.scale
    # the product
    dd = tf.ckks_encode(D.reshape(-1, N // 2).astype(complex), params.R_cipher(), scale)
    bias = tf.ckks_encode(np.repeat(np.resize(rng.normal(0, 1, 2), 8), B).astype(complex), params.R_cipher(), scale * scale)
    got = tf.matmul_bsgs_fold_grouped(bk, gk, [dd], [c], fk, bias)
    want = tf.rotate_sum_grouped(fk, tf.matmul_bsgs_blocks_grouped(bk, gk, [dd], [c])) + bias
    assert all(np.array_equal(a, b) for a, b in zip(words(got), words(want)))
    assert got.scale == want.scale
    nofold = tf.matmul_bsgs_fold_grouped(bk, gk, [dd], [c], [], bias)
    assert all(np.array_equal(a, b) for a, b in zip(words(nofold), words(tf.matmul_bsgs_blocks_grouped(bk, gk, [dd], [c], bias))))
    for refused in (lambda: tf.rotate_sum(fk, c), lambda: tf.matmul_bsgs_fold(bk, gk, [dd], [c], fk)):
        with pytest.raises(tf.UsageError, match="grouped digits"):
            refused()
