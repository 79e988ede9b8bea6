"""tfhe_bfv_mul / tfhe_bfv_mul_relin on the folded route (the plan's limb table carries the contraction's input constants; the
evaluation key is prepared once per call), bit for bit against the oracle and against the general kernels; and what must NOT have
changed next to it: the public tfhe_bfv_contract / tfhe_bfv_expand on the same plan and tfhe_mul_relin on the same context.

How often k_evk_to_f64 runs per call is not asserted here: the library's profiling hooks (tfhe_prof_read) count the launches made
through launch_prof only, and the key conversion is not one of them.  The count is read from the kernel trace of the benchmark
(profiles/LOG.md); what this file does check is that a call of two chunks -- a full one and a short one, which run on ONE
preparation -- gives the words of the same call in one chunk."""
import functools

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import ref_cpu
from tests import helpers as H

pytestmark = pytest.mark.gpu

T, BATCH = 65537, 3
SHAPES = [(4096, 2, 3), (16384, 8, 9)]


@functools.lru_cache(maxsize=None)
def case(N, ns, np_):
    """inputs and oracle results of one shape, computed once for every test of it"""
    ch = H.chain(50, ns + np_, N)
    qs = ch[:ns]
    rng = np.random.default_rng(N + ns)
    c1, c2 = H.rand_residues(rng, qs, (BATCH, 2), N), H.rand_residues(rng, qs, (BATCH, 2), N)
    evk = H.uniform_evk(rng, qs, ns, N)
    rs, rb = ref_cpu.RefCtx(N, qs), ref_cpu.RefCtx(N, ch)
    prod = ref_cpu.bfv_mul(rs, rb, T, c1, c2)
    relin = rs.keyswitch(ns, False, evk, prod)
    a = H.rand_residues(rng, qs, (2,), N)                  # stand-alone conversions
    y = H.rand_residues(rng, ch, (3,), N)
    plain = rs.keyswitch(ns, False, evk, rs.enc_mul(c1, c2))   # tfhe_mul_relin: the product of CKKS / BGV ciphertexts on ℛ
    for x in (c1, c2, evk, prod, relin, a, y, plain):
        x.setflags(write=False)
    return dict(ch=ch, qs=qs, c1=c1, c2=c2, evk=evk, prod=prod, relin=relin, a=a, y=y, expand=ref_cpu.switch(rs, rb, a),
                contract=ref_cpu.contract(rb, rs, T, y), plain=plain)


def dev(x):
    return tf.DeviceBuffer.from_numpy(x)


@pytest.mark.parametrize("N,ns,np_", SHAPES)
def test_mul_and_mul_relin_on_the_folded_route(N, ns, np_):
    K = case(N, ns, np_)
    ctx = tf.Context(N, K["ch"])
    d1, d2, dk = dev(K["c1"]), dev(K["c2"]), dev(K["evk"])
    o3, o2, om = tf.DeviceBuffer(BATCH * 3 * ns * N), tf.DeviceBuffer(BATCH * 2 * ns * N), tf.DeviceBuffer(BATCH * 2 * ns * N)

    def plain_relin():
        ctx.mul_relin(ns, ns, False, dk.ptr, ns, d1.ptr, d2.ptr, om.ptr, BATCH)
        return om.to_numpy((BATCH, 2, ns, N))

    before = plain_relin()                                   # on the context's own limb table, before any plan exists
    assert np.array_equal(before, K["plain"])
    plan = tf.BfvPlan(ctx, ctx, T, idx_s=list(range(ns)))
    got = {}
    for chunk in (2, 3):                                     # 2: a full chunk and a short one on one prepared key; 3: one chunk
        plan.set_chunk(chunk)
        plan.mul(d1.ptr, d2.ptr, o3.ptr, BATCH)
        got["mul", chunk] = o3.to_numpy((BATCH, 3, ns, N))
        plan.mul_relin(dk.ptr, ns, d1.ptr, d2.ptr, o2.ptr, BATCH)
        got["relin", chunk] = o2.to_numpy((BATCH, 2, ns, N))
    assert np.array_equal(got["mul", 2], K["prod"])
    assert np.array_equal(got["relin", 2], K["relin"])
    assert np.array_equal(got["mul", 3], got["mul", 2])
    assert np.array_equal(got["relin", 3], got["relin", 2])
    plan.set_variant(1)                                      # the general kernels: no fused core, no folded table
    plan.set_chunk(2)
    plan.mul(d1.ptr, d2.ptr, o3.ptr, BATCH)
    assert np.array_equal(o3.to_numpy((BATCH, 3, ns, N)), got["mul", 2])
    plan.mul_relin(dk.ptr, ns, d1.ptr, d2.ptr, o2.ptr, BATCH)
    assert np.array_equal(o2.to_numpy((BATCH, 2, ns, N)), got["relin", 2])
    plan.set_variant(0)
    # the public conversions take plain rows: the folded table must not reach them
    da, de = dev(K["a"]), tf.DeviceBuffer(2 * (ns + np_) * N)
    plan.expand(da.ptr, de.ptr, 2)
    assert np.array_equal(de.to_numpy((2, ns + np_, N)), K["expand"])
    dy, dc = dev(K["y"]), tf.DeviceBuffer(3 * ns * N)
    plan.contract(dy.ptr, dc.ptr, 3)
    assert np.array_equal(dc.to_numpy((3, ns, N)), K["contract"])
    # ... and the context's own table is what it was
    assert np.array_equal(plain_relin(), before)
    plan.mul_relin(dk.ptr, ns, d1.ptr, d2.ptr, o2.ptr, BATCH)   # once more after the others have used the context's workspace
    assert np.array_equal(o2.to_numpy((BATCH, 2, ns, N)), K["relin"])
    plan.close()
    assert np.array_equal(plain_relin(), before)
    ctx.close()


@pytest.mark.parametrize("N,ns,np_", SHAPES[:1])
def test_two_rings_in_two_contexts(N, ns, np_):
    """ℛ and ℛbig in contexts of their own: the key is prepared in ℛ's workspace, the folded table copies ℛbig's"""
    K = case(N, ns, np_)
    small, big = tf.Context(N, K["qs"]), tf.Context(N, K["ch"])
    plan = tf.BfvPlan(small, big, T)
    plan.set_chunk(2)
    d1, d2, dk, o2 = dev(K["c1"]), dev(K["c2"]), dev(K["evk"]), tf.DeviceBuffer(BATCH * 2 * ns * N)
    plan.mul_relin(dk.ptr, ns, d1.ptr, d2.ptr, o2.ptr, BATCH)
    assert np.array_equal(o2.to_numpy((BATCH, 2, ns, N)), K["relin"])
    plan.close()
    small.close()
    big.close()
