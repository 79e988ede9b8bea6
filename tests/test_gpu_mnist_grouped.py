"""examples/encrypted_mnist.py --hoisted [--fused] --grouped 3,3 on the device: the restructured circuit at the example's default size
(N = 2^13, the reference's trained model) on a key ring that ends in three 60-bit special primes (their product above every digit modulus), keys with digits of three limbs --
the 63 Galois keys from keygen_galois_many, the square layers' products through tf.matmul_diag_grouped (fused) or
tf.rotate_many_grouped and the plaintext sum, at the levels below the key's that the circuit reaches, the squares through keyswitch on
3-element inputs -- against the run without the flag, same seed and model: the argmax of every image is equal; the logits differ in the
noise."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location("encrypted_mnist_example", os.path.join(ROOT, "examples", "encrypted_mnist.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def base():
    """the restructured circuit without the flag: (err, logit range, agreement with the plain model, logits [10][images])"""
    return _example().run(logn=13, seed=1, verbose=False, model="reference", hoisted=True, fused=True, return_logits=True)


@pytest.mark.parametrize("fused", [True, False])
def test_grouped_keys_give_the_argmax_of_the_run_without_the_flag(base, fused):
    got = _example().run(logn=13, seed=1, verbose=False, model="reference", hoisted=True, fused=fused, return_logits=True, grouped=(3, 3))
    print(f"--hoisted{' --fused' if fused else ''} --grouped 3,3: max |logit error| {got[0]:.3e} (without the flag {base[0]:.3e}), logit range {got[1]:.2f}, "
          f"argmax agreement with the plain model {got[2]}, max |logit difference to the run without the flag| {np.abs(got[3] - base[3]).max():.3e}")
    assert base[1] > 1.0 and base[2] == 1.0
    assert got[3].shape == base[3].shape and np.array_equal(got[3].argmax(0), base[3].argmax(0))


def test_flag_combinations_that_are_not_covered_say_so():
    ex = _example()
    for kw in (dict(), dict(hoisted=True, bsgs=8), dict(hoisted=True, mul_relin=True)):
        with pytest.raises(ValueError, match="grouped keys are covered for the hoisted circuit only"):
            ex.run(logn=13, seed=1, verbose=False, grouped=(3, 3), **kw)
    with pytest.raises(ValueError, match="below the largest digit modulus"):
        ex.run(logn=13, seed=1, verbose=False, hoisted=True, fused=True, grouped=(1, 3))
