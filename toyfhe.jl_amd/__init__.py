"""toyfhe.jl_amd -- MI355X-native engine for the power-of-two-cyclotomic RNS path of ToyFHE.jl.

The directory name contains a dot, so import it through the repo-root loader module:
``import toyfhe_jl_amd``.  Only what the hot path needs lives here: ``csrc/`` (HIP kernels + C ABI),
``native`` (ctypes binding) and the host-side mirror of the reference's ring/ciphertext interface.
"""
from . import native  # noqa: F401
from .native import BfvPlan, Comm, PlainPlan, Context, DeviceBuffer, Event, HipError, UsageError  # noqa: F401
from . import ring, she  # noqa: F401,E402
from .ring import NegacyclicRing, PlainElement, PlainRing, RingElement, nextprime, plaintext_space  # noqa: F401,E402
from . import wire  # noqa: F401,E402
from .she import (DeviceRng, BFVParams, BGVParams, CKKSParams, CipherText, GroupedRaised, ModulusRaised, apply_galois_element, bsgs_diagonals,  # noqa: F401,E402
                  ckks_decode, ckks_encode, decrypt, decrypt_array, enc_mul, encrypt, invariant_noise_budget, keygen, keygen_evalmult, keygen_galois, keygen_galois_many,
                  keyswitch, make_eval_key, matmul_bsgs, matmul_bsgs_blocks, matmul_bsgs_blocks_grouped, matmul_bsgs_fold, matmul_bsgs_fold_grouped, matmul_bsgs_grouped, matmul_diag, matmul_diag_grouped, modswitch, mul_relin, mul_relin_grouped,
                  rect_diagonals, rotate, rotate_many, rotate_many_grouped, rotate_sum, rotate_sum_grouped)
