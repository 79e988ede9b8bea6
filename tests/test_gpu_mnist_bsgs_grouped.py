"""examples/encrypted_mnist.py --bsgs 8 --blocks --grouped 3,3 on the device: the restructured circuit at the example's default size
(N = 2^13, the reference's trained model) on a key ring that ends in three 60-bit special primes, keys with digits of three limbs -- the
7 baby and 7 giant Galois keys from keygen_galois_many, the first dense layer through tf.matmul_bsgs_blocks_grouped and the last through
tf.matmul_bsgs_grouped (tfhe_matmul_bsgs_grouped), at the levels below the key's that the circuit reaches -- against the run without
--grouped, same seed and model: the argmax of every image is equal; the logits differ in the noise.  The two errors are printed side
by side; no threshold is taken from the code under test."""
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


def test_grouped_keys_give_the_argmax_of_the_run_without_the_flag():
    ex = _example()
    base = ex.run(logn=13, seed=1, verbose=False, model="reference", bsgs=8, blocks=True, return_logits=True)
    got = ex.run(logn=13, seed=1, verbose=False, model="reference", bsgs=8, blocks=True, return_logits=True, grouped=(3, 3))
    print(f"--bsgs 8 --blocks --grouped 3,3: max |logit error| {got[0]:.3e} (without --grouped {base[0]:.3e}), logit range {got[1]:.2f}, "
          f"argmax agreement with the plain model {got[2]}, max |logit difference to the run without --grouped| {np.abs(got[3] - base[3]).max():.3e}")
    assert base[1] > 1.0 and base[2] == 1.0
    assert got[3].shape == base[3].shape and np.array_equal(got[3].argmax(0), base[3].argmax(0))


def test_the_fold_on_grouped_keys_says_it_is_not_covered():
    ex = _example()
    with pytest.raises(ValueError, match="tfhe_matmul_bsgs_fold, which refuses keys with grouped digits"):
        ex.run(logn=13, seed=1, verbose=False, bsgs=8, rect=True, grouped=(3, 3))
    with pytest.raises(ValueError, match="grouped keys are covered for the hoisted circuit only"):
        ex.run(logn=13, seed=1, verbose=False, bsgs=8, hoisted=True, grouped=(3, 3))
