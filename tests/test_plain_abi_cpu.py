"""No-GPU checks of the plaintext-codec entry points (tfhe_plain_*, tfhe_bfv_noise_max): every argument check runs on the
host before any device use, so NULL / invalid arguments give TFHE_E_BADARG with or without a GPU, and the header, the
binding and the library agree on them."""
import ctypes as C

import numpy as np

from toyfhe_jl_amd import native

BADARG = native.E_BADARG
NAMES = ["tfhe_plain_plan_create", "tfhe_plain_plan_destroy", "tfhe_plain_encode", "tfhe_plain_decode", "tfhe_bfv_noise_max"]


def _err():
    return native.lib().tfhe_last_error().decode()


def test_entry_points_declared_bound_and_exported():
    lib = native.lib()
    for name in NAMES:
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert (native.PLAIN_BFV, native.PLAIN_BGV) == (0, 1)


def test_plan_create_validates_before_device_use():
    lib = native.lib()
    out = C.c_void_p(1234)
    idx = (C.c_int32 * 2)(0, 1)
    # limbs out of range, t outside [2, 2^62): rejected before the context is looked at
    for limbs in (0, -1, 41):
        assert lib.tfhe_plain_plan_create(None, idx, limbs, 65537, C.byref(out)) == BADARG
        assert "limbs" in _err()
    assert out.value is None                       # *out is cleared first
    for t in (0, 1, 2**62, 2**64 - 1):
        assert lib.tfhe_plain_plan_create(None, idx, 2, t, C.byref(out)) == BADARG
        assert "plaintext modulus" in _err()
    assert lib.tfhe_plain_plan_create(None, idx, 2, 65537, C.byref(out)) == BADARG
    assert "null" in _err()
    assert lib.tfhe_plain_plan_create(None, idx, 2, 65537, None) == BADARG
    assert lib.tfhe_plain_plan_destroy(None) == native.OK


def test_codec_calls_validate_before_device_use():
    lib = native.lib()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    for f in (lib.tfhe_plain_encode, lib.tfhe_plain_decode):
        assert f(None, native.PLAIN_BFV, p, p, -1) == BADARG
        assert "negative count" in _err()
        for scheme in (-1, 2, 7):
            assert f(None, scheme, p, p, 1) == BADARG
            assert "scheme" in _err()
        for a, b in ((None, p), (p, None), (None, None)):
            assert f(None, native.PLAIN_BGV, a, b, 1) == BADARG
            assert "null" in _err()
        assert f(None, native.PLAIN_BFV, p, p, 0) == BADARG    # a missing plan is an error even for an empty batch
    assert lib.tfhe_bfv_noise_max(None, p, p, -5) == BADARG
    assert "negative count" in _err()
    assert lib.tfhe_bfv_noise_max(None, None, p, 1) == BADARG
    assert lib.tfhe_bfv_noise_max(None, p, None, 1) == BADARG
    assert "null" in _err()
