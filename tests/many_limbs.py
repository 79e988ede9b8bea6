"""Rings of 17 to 40 limbs on both sides of the 32-limb routing-mask seam (toyfhe_hip.hip mask_all / mask_of), shared by
tests/test_many_limbs_cpu.py and tests/test_gpu_many_limbs.py.  Every modulus is distinct and = 1 mod 2N."""
import functools

from tests import helpers as H

MAX_LIMBS = 40     # conv_core.h TFHE_MAX_LIMBS
MASK_BITS = 32     # width of ntt_io_t::limb_mask and the key-switch kernels' limb masks


def _distinct(qs, N):
    assert len(set(qs)) == len(qs) and all(q % (2 * N) == 1 and q < H.Q_LIMIT for q in qs)
    return list(qs)


@functools.lru_cache(maxsize=None)
def _ring(name, N):
    if name == "U40":      # 40 x 40 bit: every limb fp64-size and narrow
        qs = H.chain(40, 40, N)
        assert all(q < H.FPS_QMAX for q in qs)
    elif name == "W40":    # 40 x 61 bit: the u64 policy only, none narrow
        qs = H.chain(61, 40, N)
        assert all(q >> H.FOLD_BITS for q in qs)
    elif name == "N34":    # 34 x 51 bit: at or above TFHE_FP_QMAX and below 2^52 -- narrow but not fp64-size
        qs = H.chain(51, 34, N)
        assert all(H.FP_QMAX <= q < (1 << H.FOLD_BITS) for q in qs)
    elif name in ("M34", "M33e"):   # 60-bit q0, 40-bit primes, 60-bit special prime last (infer.jl:97-112 stretched)
        q0, sp = H.chain(60, 2, N)
        qs = [q0] + H.chain(40, 32 if name == "M34" else 31, N) + [sp]
    else:
        raise KeyError(name)
    return tuple(_distinct(qs, N))


def ring(name, N):
    return list(_ring(name, N))


def mixed(n, N):
    """the mixed recipe at any limb count n >= 3: 60-bit q0, n - 2 primes of 40 bits, 60-bit special prime last"""
    q0, sp = H.chain(60, 2, N)
    return _distinct([q0] + H.chain(40, n - 2, N) + [sp], N)


def mixed40(N):
    """the "40 mixed" ring of tests/test_plain_codec_cpu.py: ten primes each of 30, 61, 40 and 50 bits"""
    return _distinct(H.chain(30, 10, N) + H.chain(61, 10, N) + H.chain(40, 10, N) + H.chain(50, 10, N), N)


def shuffled(n, k, seed):
    """k of the n limb positions in an order that is neither ascending nor descending"""
    import numpy as np
    idx = np.random.default_rng(seed).permutation(n)[:k].tolist()
    assert idx != sorted(idx) and idx != sorted(idx, reverse=True)
    return idx
