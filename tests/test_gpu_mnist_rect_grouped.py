"""examples/encrypted_mnist.py --bsgs 8 --rect --grouped 3,3 --fold-grouped on the device: the circuit at the example's default size
(N = 2^13, the reference's trained model) on a key ring that ends in three 60-bit special primes, keys with digits of three limbs, the
last layer -- 10 x 64, + bias -- as ONE tf.matmul_bsgs_fold_grouped call (tfhe_matmul_bsgs_fold_grouped) over 16 extended diagonals and
the fold, against the same run without `grouped` / `fold_grouped` (tfhe_matmul_bsgs_fold on per-limb keys), same seed and model: the
argmax of every image is equal; the logits differ in the noise.  The two errors and their difference are printed; no bound is fixed on
them beyond the argmax."""
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


def test_rectangular_last_layer_on_grouped_keys_gives_the_argmax_of_the_per_limb_run():
    ex = _example()
    base = ex.run(logn=13, seed=1, verbose=False, model="reference", bsgs=8, rect=True, return_logits=True)
    got = ex.run(logn=13, seed=1, verbose=False, model="reference", bsgs=8, rect=True, grouped=(3, 3), fold_grouped=True, return_logits=True)
    print(f"--bsgs 8 --rect --grouped 3,3 --fold-grouped: max |logit error| {got[0]:.3e} (without --grouped {base[0]:.3e}), difference of the two "
          f"{got[0] - base[0]:+.3e}, logit range {got[1]:.2f}, argmax agreement with the plain model {got[2]}, "
          f"max |logit difference to the run without --grouped| {np.abs(got[3] - base[3]).max():.3e}")
    assert got[3].shape == base[3].shape and np.array_equal(got[3].argmax(0), base[3].argmax(0))


def test_the_flag_needs_its_three_companions():
    ex = _example()
    for kw in (dict(bsgs=8, rect=True), dict(bsgs=8, grouped=(3, 3)), dict(rect=True, grouped=(3, 3), hoisted=True)):
        with pytest.raises(ValueError, match="fold_grouped|blocks and rect need bsgs"):
            ex.run(logn=13, seed=1, verbose=False, fold_grouped=True, **kw)
