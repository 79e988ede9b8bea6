#!/usr/bin/env python3
"""Encrypted CNN inference in the shape of the reference's examples/encrypted_mnist/infer.jl,
driven through the host mirror with every ring operation on the MI355X.

The reference evaluates its trained Flux model (examples/encrypted_mnist/mnist_conv.bson) on MNIST.  The weights are
exported from that file by tools/export_mnist_bson.py (a BSON reader, run in the build container) into
tests/golden/mnist_conv.npz and used here by default (`--model synthetic` draws a random model of the same architecture);
the MNIST images are not on disk, so the batch is synthetic (seeded; sparse stroke-like 28x28 images in [0, 1]).  The
homomorphic result is checked against the same arithmetic in float64 (infer.jl:55-88 `do_encrypted_inference`):

    conv 7x7 stride 3, 4 channels (49 ciphertexts x plaintext scalars)  ->  + bias  ->  rescale        infer.jl:127-131
    square + relinearise + rescale                                                                      :136-138
    dense 256 -> 64 as 4 diagonal-packed 64x64 products (63 rotations by 64 slots each)  + bias, rescale :142-165
    square + relinearise + rescale                                                                      :167-169
    dense 64 -> 10 (zero-padded to 64x64, 63 rotations) + bias                                          :171-179

Packing: N/2 slots = 64 windows x B images (B = N/128; the reference uses N = 2^13, B = 64), slot = window * B + image.

  python examples/encrypted_mnist.py [--logn 13] [--seed 0]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toyfhe_jl_amd as tf  # noqa: E402


def public_preprocess(batch):
    """infer.jl:57-64: I[i][j] = matrix [image k][window l] of pixel (i, j) of each 7x7 window (stride 3, 8x8 windows)"""
    B = batch.shape[0]
    I = np.empty((7, 7, B, 64))
    for a in range(8):
        for b in range(8):
            I[:, :, :, a + 8 * b] = batch[:, a * 3:a * 3 + 7, b * 3:b * 3 + 7].transpose(1, 2, 0)
    return I


def plain_matmul(W, x):
    """infer.jl:44-46 on plaintext: sum_k diag(circshift(W, (0, k-1))) .* circshift(x, (k-1, 0)) == W @ x"""
    n = x.shape[0]
    out = np.zeros_like(x)
    for k in range(n):
        d = np.array([W[i, (i - k) % n] for i in range(n)])
        out += d[:, None] * np.roll(x, k, axis=0)
    return out


def plain_model(model, batch):
    I = public_preprocess(batch)                                   # [7][7][B][64]
    conv = [sum(I[i, j] * model["conv_w"][i, j, ch] for i in range(7) for j in range(7)) + model["conv_b"][ch] for ch in range(4)]
    sq1 = [(c ** 2).T for c in conv]                               # [64 windows][B]
    fq1 = sum(plain_matmul(model["fq1_w"][:, 64 * i:64 * (i + 1)], sq1[i]) for i in range(4)) + model["fq1_b"][:, None]
    sq2 = fq1 ** 2
    W2 = np.vstack([model["fq2_w"], np.zeros((54, 64))])
    return (plain_matmul(W2, sq2) + np.concatenate([model["fq2_b"], np.zeros(54)])[:, None])[:10]


class BsgsKeys:
    """the two key sets of the baby-step/giant-step product: n1 - 1 keys for the steps B, 2B, .. and 64 / n1 - 1 for n1 B, 2 n1 B, .."""

    def __init__(self, n1, baby, giant):
        self.n1, self.baby, self.giant = n1, list(baby), list(giant)


def encrypted_matmul(gk, W, x, B, cache=None, fused=False):
    """infer.jl:140-149: diagonal method; `rotate` by B slots moves every window's value to the next window.
    gk = one Galois key (the reference's loop: 63 chained rotations by B slots) or a list of 63 keys for the steps B, 2B, ...,
    63B (hoisted: every rotation starts from x and they share one digit decomposition, tfhe_rotate_many -- fewer transforms
    and 63 times less rotation noise, at the price of 63 keys)."""
    n = 64
    K = x[0].count

    def diag(k):
        # the k-th generalised diagonal as a plaintext at x's scale; encoded once per (matrix, k) when a cache is given
        # (a deployed model encodes its weights once, not per inference)
        key = (id(W), k, x.ring().L, x.scale)
        if cache is not None and key in cache:
            return cache[key]
        v = np.repeat(np.array([W[i, (i - k) % n] for i in range(n)]), B)
        if cache is None:
            return v
        pt = tf.ckks_encode(np.repeat(v[None].astype(np.complex128), K, axis=0), x.ring(), x.scale)
        pt.coeffs_dual()
        cache[key] = pt
        return pt
    if isinstance(gk, BsgsKeys):
        # the whole product in one device call by baby and giant steps (tfhe_matmul_bsgs): n1 + 64 / n1 - 2 keys instead of 63; the
        # diagonals are pre-rotated on the host (bsgs_diagonals) and encoded once per (matrix, level, scale)
        # (on keys with grouped digits: tfhe_matmul_bsgs_grouped)
        return (tf.matmul_bsgs_grouped if _grouped(gk.baby + gk.giant) else tf.matmul_bsgs)(gk.baby, gk.giant, bsgs_encoded(gk, W, x, B, cache), x)
    if isinstance(gk, (list, tuple)) and cache is not None and fused:
        # the whole product in one device call (tfhe_matmul_diag): the diagonals are single plaintexts shared by the batch
        key = (id(W), "fused", x.ring().L, x.scale)
        if key not in cache:
            vs = np.stack([np.repeat(np.array([W[i, (i - k) % n] for i in range(n)]), B) for k in range(n)]).astype(np.complex128)
            enc = tf.ckks_encode(vs, x.ring(), x.scale)                       # the 64 diagonals as one stacked plaintext element
            enc.coeffs_dual()
            cache[key] = enc
        return (tf.matmul_diag_grouped if _grouped(gk) else tf.matmul_diag)(gk, cache[key], x)
    if isinstance(gk, (list, tuple)):
        rots = [x] + list((tf.rotate_many_grouped if _grouped(gk) else tf.rotate_many)(gk, x))
    else:
        rots = [x]
        for k in range(1, n):
            rots.append(tf.rotate(gk, rots[-1]))
    if cache is not None:      # plaintexts are ring elements already: the whole accumulation is one device pass per component
        return tf.CipherText.dot_plain(rots, [diag(k) for k in range(n)])
    result = rots[0].mul_plain(diag(0))
    for k in range(1, n):
        result = result + rots[k].mul_plain(diag(k))
    return result


def _grouped(gks):
    """whether a list of Galois keys has grouped digits (GroupedRaised): the hoisted rotations and the product have entry points of their own"""
    return isinstance(gks[0].key.params, tf.GroupedRaised)


def bsgs_encoded(gk, W, x, B, cache=None):
    """the pre-rotated diagonals of W for the baby/giant split of `gk` as one stacked plaintext at x's level and scale, encoded once
    per (matrix, split, level, scale) when a cache is given"""
    n = 64
    key = (id(W), "bsgs", gk.n1, x.ring().L, x.scale)
    if cache is not None and key in cache:
        return cache[key]
    vs = np.stack([np.repeat(np.array([W[i, (i - k) % n] for i in range(n)]), B) for k in range(n)])
    D = tf.bsgs_diagonals(vs, gk.n1, block=B)[0]
    enc = tf.ckks_encode(D.reshape(-1, D.shape[-1]).astype(np.complex128), x.ring(), x.scale)
    enc.coeffs_dual()
    if cache is not None:
        cache[key] = enc
    return enc


def encrypted_matmul_blocks(gk, Ws, xs, B, b, cache=None, name=None):
    """infer.jl:158-163 in one device call (tfhe_matmul_bsgs_blocks): sum_m Ws[m] @ xs[m] .+ b with the inner sums of all inputs added
    before the giant rotations -- len(gk.giant) giant key switches instead of len(xs) times as many; the bias, encoded at the result's
    scale (once per (layer, level, scale) with a cache, under add_bias's key), rides on the closing sum"""
    x = xs[0]
    scale2 = x.scale ** 2
    key = ("bias", name, x.ring().L, scale2)
    if cache is not None and key in cache:
        bias = cache[key]
    else:
        bias = tf.ckks_encode(np.asarray(b, dtype=np.complex128), x.ring(), scale2)
        if cache is not None:
            cache[key] = bias
    product = tf.matmul_bsgs_blocks_grouped if _grouped(gk.baby + gk.giant) else tf.matmul_bsgs_blocks
    return product(gk.baby, gk.giant, [bsgs_encoded(gk, W, x, B, cache) for W in Ws], xs, bias)


class RectKeys:
    """the key sets of a rectangular product by extended diagonals (tf.rect_diagonals): baby, giant, and one list of keys per fold step"""

    def __init__(self, n1, baby, giant, folds):
        self.n1, self.baby, self.giant, self.folds = n1, list(baby), list(giant), [list(g) for g in folds]


def encrypted_matmul_rect(gk, W, x, B, b, cache=None, name=None):
    """the last layer (infer.jl:169-173, a 10 x 64 matrix, .+ b) in one device call (tfhe_matmul_bsgs_fold): 16 extended diagonals and
    the fold of the four partial sums (tf.rect_diagonals' default: one step of three rotations) instead of the 64 diagonals of the
    matrix padded to 64 x 64.  Every row r of the result holds logit r mod 16; the
    bias, replicated the same way and encoded at the result's scale, is added after the fold."""
    scale2 = x.scale ** 2
    key = (id(W), "rect", gk.n1, x.ring().L, x.scale)
    if cache is not None and key in cache:
        enc, bias = cache[key]
    else:
        D = tf.rect_diagonals(W, gk.n1, block=B)[0]
        enc = tf.ckks_encode(D.reshape(-1, D.shape[-1]).astype(np.complex128), x.ring(), x.scale)
        enc.coeffs_dual()
        m = D.shape[0] * D.shape[1]                                 # the row count rounded up to a power of two
        bp = np.concatenate([np.asarray(b, dtype=np.float64), np.zeros(m - len(b))])
        bias = tf.ckks_encode(np.repeat(np.tile(bp, W.shape[1] // m), B).astype(np.complex128), x.ring(), scale2)
        if cache is not None:
            cache[key] = (enc, bias)
    # (on keys with grouped digits: tfhe_matmul_bsgs_fold_grouped)
    fold = tf.matmul_bsgs_fold_grouped if _grouped(gk.baby + gk.giant + [g for st in gk.folds for g in st]) else tf.matmul_bsgs_fold
    return fold(gk.baby, gk.giant, [enc], [x], gk.folds, bias)


def add_bias(ct, x, cache=None, name=None):
    """ct .+ bias (infer.jl: the `.+ b` of every layer).  With a cache the bias is encoded once per (layer, level, scale) like the
    weight plaintexts -- each encoding is a host-to-device copy the pass would otherwise wait on -- and added to the first
    component as CipherText.add_plain does."""
    if cache is None:
        return ct.add_plain(x)
    key = ("bias", name, ct.ring().L, ct.scale)
    if key not in cache:
        n2 = ct.ring().N // 2
        v = np.full(n2, x, dtype=np.complex128) if np.isscalar(x) else np.asarray(x, dtype=np.complex128)
        cache[key] = tf.ckks_encode(v, ct.ring(), ct.scale)
    return tf.CipherText(ct.params, (ct.cs[0] + cache[key],) + tuple(ct.cs[1:]), ct.scale)


GOLDEN_MODEL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "mnist_conv.npz")


def load_model(path=GOLDEN_MODEL):
    """the reference's trained weights; infer.jl:118-119 flips the Flux convolution kernel in both spatial dimensions"""
    d = np.load(path)
    m = {k: d[k].astype(np.float64) for k in d.files}
    m["conv_w"] = m["conv_w"][::-1, ::-1, :].copy()
    return m


def run(logn=13, seed=0, verbose=True, model="reference", batches=1, hoisted=False, repeat=1, fused=False, return_logits=False, stats=None,
        mul_relin=False, bsgs=0, blocks=False, rect=False, grouped=None, mul_relin_grouped=False, fold_grouped=False):
    """`grouped` = (K, G) (with `hoisted`, or with `bsgs` alone): the key ring ends in K 60-bit special primes instead of one and every key
    has grouped digits of G limbs (tf.GroupedRaised): the Galois keys shrink from 6 to ceil(6 / G) components.  With `hoisted` the square
    layers go through tf.matmul_diag_grouped (with `fused`) or tf.rotate_many_grouped and the plaintext sum; with `bsgs` (with or without
    `blocks`) through tf.matmul_bsgs_grouped / tf.matmul_bsgs_blocks_grouped (tfhe_matmul_bsgs_grouped).  The squares go through
    keyswitch (or `mul_relin_grouped`, below).  The fold (`rect`) on grouped keys is asked for by `fold_grouped`; mul_relin takes per-limb
    keys.
    `fold_grouped` (with `bsgs`, `rect` and `grouped`): the rectangular last layer as ONE tf.matmul_bsgs_fold_grouped call
    (tfhe_matmul_bsgs_fold_grouped) on the grouped keys.  Without it `rect` with `grouped` is refused, as before.
    `mul_relin_grouped` (with `hoisted` and `grouped`): the two square layers as one device call each (tf.mul_relin_grouped =
    tfhe_mul_relin_grouped, rescale=True) instead of modswitch(keyswitch(ek, c * c)); same logits, bit for bit.
    `rect` (with `bsgs`): the last layer -- 10 x 64, .+ b -- as ONE tfhe_matmul_bsgs_fold call over 16 extended diagonals and the fold
    of the four partial sums instead of the full product of the matrix padded to 64 x 64 (the key sets: the square product's baby and
    giant keys where the steps coincide, new keys for the rest).
    `blocks` (with `bsgs`): the first dense layer -- a 64 x 256 matrix over the four squares, .+ b -- as ONE tfhe_matmul_bsgs_blocks
    call instead of four tfhe_matmul_bsgs calls, three ciphertext additions and a plaintext addition.
    `bsgs` = n1 > 0: every matrix product as one tfhe_matmul_bsgs call with n1 - 1 baby and ceil(64 / n1) - 1 giant keys (a third
    circuit shape beside the chained loop and the 63 hoisted keys; the other layers as chosen by the remaining switches).
    `mul_relin`: the two square layers as one device call each (she.mul_relin = tfhe_mul_relin) instead of
    modswitch(keyswitch(ek, c * c)); same logits, bit for bit.
    `batches` = K ciphertext sets evaluated together (K * B images): every ring element carries a leading batch dimension
    of K, so each device call covers K ciphertexts (the batch the engine shards across GPUs)."""
    if (blocks or rect) and not bsgs:
        raise ValueError("blocks and rect need bsgs = n1 > 0")
    if fold_grouped and not (bsgs and rect and grouped is not None):
        raise ValueError("fold_grouped is the rectangular last layer on grouped keys: it needs bsgs = n1 > 0, rect and grouped = (K, G)")
    if grouped is not None and rect and not fold_grouped:
        raise ValueError("rect goes through tfhe_matmul_bsgs_fold, which refuses keys with grouped digits: grouped goes with bsgs and blocks only")
    if grouped is not None and (bool(hoisted) == bool(bsgs) or mul_relin):
        raise ValueError("grouped keys are covered for the hoisted circuit only (hoisted, with or without fused) or, instead of it, for the "
                         "baby-step/giant-step products (bsgs, with or without blocks): the chained rotation by one prepared key, the fold "
                         "(rect) and mul_relin have no grouped form")
    if mul_relin_grouped and (grouped is None or not hoisted):
        raise ValueError("mul_relin_grouped is the square layer on grouped keys: it needs hoisted and grouped = (K, G)")
    if mul_relin_grouped:
        square = lambda c: tf.mul_relin_grouped(ek, c, c, rescale=True)
    elif mul_relin:
        square = lambda c: tf.she.mul_relin(ek, c, c, rescale=True)
    else:
        square = lambda c: tf.modswitch(tf.keyswitch(ek, c * c))
    N = 1 << logn
    B = N // 128                                                   # images per ciphertext
    K = int(batches)
    rs = np.random.default_rng(seed)
    if model == "reference":
        model = load_model()
    else:
        model = {"conv_w": rs.normal(0, 0.15, (7, 7, 4)), "conv_b": rs.normal(0, 0.1, 4),
                 "fq1_w": rs.normal(0, 0.06, (64, 256)), "fq1_b": rs.normal(0, 0.1, 64),
                 "fq2_w": rs.normal(0, 0.1, (10, 64)), "fq2_b": rs.normal(0, 0.1, 10)}
    batch = (rs.random((K * B, 28, 28)) < 0.15) * rs.random((K * B, 28, 28))   # sparse strokes: MNIST-like pixel statistics
    want = plain_model(model, batch)

    # infer.jl:97-112: q0 (60 bit), five 40-bit primes, 60-bit special prime; ModulusRaised CKKS, sigma 3.2
    q0 = tf.nextprime(2**60 + 1, 1, 2 * N)
    ps = tf.nextprime(q0 + 2 * N, 1, 2 * N)
    qs = [tf.nextprime(2**40 + 1, 1, 2 * N)]
    for _ in range(4):
        qs.append(tf.nextprime(qs[-1] + 2 * N, 1, 2 * N))
    if grouped is None:
        ring = tf.NegacyclicRing(N, [q0] + qs + [ps])
        params = tf.ModulusRaised(tf.CKKSParams(ring, 0, 3.2))
    else:              # the same ciphertext ring under K 60-bit special primes (the reference's own first), G limbs per digit
        n_special, group = (int(v) for v in grouped)
        sp = [ps]
        for _ in range(n_special - 1):
            sp.append(tf.nextprime(sp[-1] + 2 * N, 1, 2 * N))
        ring = tf.NegacyclicRing(N, [q0] + qs + sp[:n_special])
        params = tf.GroupedRaised(tf.CKKSParams(ring, 0, 3.2), n_special, group)
        # the key-switch noise is the key's noise times Q_g / P: the special primes' product has to reach the largest digit modulus
        P, top = int(np.prod([int(p) for p in sp[:n_special]], dtype=object)), [q0] + qs
        Qg = max(int(np.prod([int(q) for q in top[i:i + group]], dtype=object)) for i in range(0, len(top), group))
        if P < Qg:
            raise ValueError(f"grouped = ({n_special}, {group}): {n_special} 60-bit special primes ({P.bit_length()} bits) are below the largest digit "
                             f"modulus ({Qg.bit_length()} bits); the rotations would drown the 2^40 scale in key-switch noise: more special primes or smaller digits")
    rng = tf.DeviceRng(seed + 1)                                   # all sampling on the GPU
    t0 = time.perf_counter()
    kp = tf.keygen(rng, params)
    ek = tf.keygen_evalmult(rng, kp.priv)
    if bsgs:
        _, bsteps, gsteps = tf.bsgs_diagonals(np.zeros((64, 1)), int(bsgs), block=B)
        keys = tf.keygen_galois_many(rng, kp.priv, steps=bsteps + gsteps)               # one device call for both key sets
        gk = BsgsKeys(int(bsgs), keys[:len(bsteps)], keys[len(bsteps):])
        if rect:   # the last layer's own steps: the square product's keys where it has them, new keys for the rest (the fold's)
            _, rb, rg, rf = tf.rect_diagonals(np.zeros((10, 64)), int(bsgs), block=B)
            have = dict(zip(bsteps + gsteps, keys))
            need = sorted({s for s in rb + rg + [s for g in rf for s in g]} - set(have))
            have.update(zip(need, tf.keygen_galois_many(rng, kp.priv, steps=need)))
            gk_rect = RectKeys(int(bsgs), [have[s] for s in rb], [have[s] for s in rg], [[have[s] for s in g] for g in rf])
    elif hoisted:
        gk = tf.keygen_galois_many(rng, kp.priv, steps=[k * B for k in range(1, 64)])   # one device call for the 63 keys
    else:
        gk = tf.keygen_galois(rng, kp.priv, steps=B)               # infer.jl:134 (steps = 64 there)
    scale = 2**40
    I = public_preprocess(batch)
    cring = params.R_cipher()
    def slots(m):                                                  # [K*B images][64 windows] -> [K][N/2], slot = window * B + image
        return m.reshape(K, B, 64).transpose(0, 2, 1).reshape(K, -1)
    C = [[tf.encrypt(rng, kp, tf.ckks_encode(slots(I[i, j]), cring, scale), scale=scale) for j in range(7)] for i in range(7)]
    t_setup = time.perf_counter() - t0

    fq1_blocks = [np.ascontiguousarray(model["fq1_w"][:, 64 * i:64 * (i + 1)]) for i in range(4)]   # stable ids for the cache
    W2 = np.vstack([model["fq2_w"], np.zeros((54, 64))])
    cache = {} if (repeat > 1 or fused) else None                 # pre-encoded weight plaintexts, filled by the first pass
    for rep in range(repeat):
      ev0, ev1 = tf.Event(), tf.Event()                             # device-side span of the pass next to the host's clock
      ev0.record(cring.ctx)
      t0 = time.perf_counter()
      conved = []
      if fused:        # the 4 x 49 scalar-weighted terms in one device pass per component over the 49 inputs (tfhe_lincomb_many)
          accs = tf.CipherText.lincomb_many([C[i][j] for i in range(7) for j in range(7)],
                                            [[float(model["conv_w"][i, j, ch]) for i in range(7) for j in range(7)] for ch in range(4)])
      for ch in range(4):
          if fused:
              acc = accs[ch]
          else:
              acc = None
              for i in range(7):
                  for j in range(7):
                      term = C[i][j].mul_plain(float(model["conv_w"][i, j, ch]))
                      acc = term if acc is None else acc + term
          conved.append(tf.modswitch(add_bias(acc, float(model["conv_b"][ch]), cache, ("conv", ch))))
      if fused:    # the four channels' squares, relinearisations and rescales as ONE batch of 4 K ciphertexts
          big = tf.CipherText.concat(conved)
          sq1 = square(big).split([K] * 4)
      else:
          sq1 = [square(c) for c in conved]
      if blocks:
          fq1 = tf.modswitch(encrypted_matmul_blocks(gk, fq1_blocks, list(sq1), B, np.repeat(model["fq1_b"], B), cache, "fq1"))
      else:
          fq1 = None
          for i in range(4):
              part = encrypted_matmul(gk, fq1_blocks[i], sq1[i], B, cache, fused)
              fq1 = part if fq1 is None else fq1 + part
          fq1 = tf.modswitch(add_bias(fq1, np.repeat(model["fq1_b"], B), cache, "fq1"))
      sq2 = square(fq1)
      if rect:
          res = encrypted_matmul_rect(gk_rect, model["fq2_w"], sq2, B, model["fq2_b"], cache, "fq2")
      else:
          res = add_bias(encrypted_matmul(gk, W2, sq2, B, cache, fused), np.repeat(np.concatenate([model["fq2_b"], np.zeros(54)]), B), cache, "fq2")
      ev1.record(res[0].ring.ctx)
      t_enq = time.perf_counter() - t0                                # every launch of the circuit is enqueued; the device may still be running
      dec = tf.ckks_decode(tf.decrypt(kp, res), res.scale).real       # [K][N/2]
      got = dec.reshape(K, 64, B)[:, :10].transpose(1, 0, 2).reshape(10, K * B)
      t_eval = time.perf_counter() - t0
    err = float(np.abs(got - want).max())
    if stats is not None:   # (tools/bench_configs.py)
        stats.update(images=K * B, eval_s=t_eval, setup_s=t_setup, images_per_s=K * B / t_eval, host_enqueue_s=t_enq,
                     device_span_s=ev0.elapsed_ms(ev1) * 1e-3)
    if verbose:
        print(f"N=2^{logn}, {K} x {B} images: setup {t_setup:.2f} s, encrypted evaluation {t_eval:.2f} s = {K * B / t_eval:.0f} images/s "
              f"(49 encrypted inputs, 5 x 63 {'hoisted ' if hoisted else ''}rotations, 5 relinearisations per ciphertext set"
              f"{'; pass ' + str(repeat) + ' with the weight plaintexts encoded by pass 1' if repeat > 1 else ''})")
        print(f"max |encrypted - plaintext| over the 10 x {K * B} logits: {err:.3e}   (logit range +-{np.abs(want).max():.2f})")
        print("argmax agreement:", float((got.argmax(0) == want.argmax(0)).mean()))
    if return_logits:
        return err, float(np.abs(want).max()), float((got.argmax(0) == want.argmax(0)).mean()), got
    return err, float(np.abs(want).max()), float((got.argmax(0) == want.argmax(0)).mean())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=13)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--model", default="reference", choices=["reference", "synthetic"])
    ap.add_argument("--batches", type=int, default=1, help="ciphertext sets evaluated together (images = batches * N/128)")
    ap.add_argument("--hoisted", action="store_true", help="63 Galois keys and tfhe_rotate_many instead of 63 chained rotations")
    ap.add_argument("--repeat", type=int, default=1, help="evaluate this many times; from the second pass on the weight plaintexts are cached")
    ap.add_argument("--fused", action="store_true",
                    help="with --hoisted: each matrix product as one tfhe_matmul_diag call and each convolution channel as one tfhe_lincomb per component")
    ap.add_argument("--mul-relin", action="store_true",
                    help="the two square layers through she.mul_relin (one tfhe_mul_relin call each) instead of modswitch(keyswitch(ek, c * c))")
    ap.add_argument("--bsgs", type=int, default=0, metavar="N1",
                    help="each matrix product as one tfhe_matmul_bsgs call: N1 - 1 baby and ceil(64 / N1) - 1 giant Galois keys instead of 63")
    ap.add_argument("--blocks", action="store_true",
                    help="with --bsgs N1: the first dense layer (64 x 256 over the four squares, + bias) as one tfhe_matmul_bsgs_blocks call")
    ap.add_argument("--grouped", default=None, metavar="K,G",
                    help="with --hoisted or with --bsgs N1 [--blocks]: K 60-bit special primes and G limbs per digit (GroupedRaised keys); the "
                         "products through tfhe_matmul_diag_grouped (--fused), tfhe_rotate_many_grouped or tfhe_matmul_bsgs_grouped (--bsgs)")
    ap.add_argument("--mul-relin-grouped", action="store_true",
                    help="with --hoisted --grouped K,G: the two square layers through tf.mul_relin_grouped (one tfhe_mul_relin_grouped call "
                         "each, the rescale on the key switch's tail) instead of modswitch(keyswitch(ek, c * c))")
    ap.add_argument("--rect", action="store_true",
                    help="with --bsgs N1: the last layer (10 x 64, + bias) as one tfhe_matmul_bsgs_fold call: 16 extended diagonals and a fold")
    ap.add_argument("--fold-grouped", action="store_true",
                    help="with --bsgs N1 --rect --grouped K,G: the rectangular last layer as one tfhe_matmul_bsgs_fold_grouped call on the grouped keys")
    a = ap.parse_args()
    if (a.blocks or a.rect) and not a.bsgs:
        ap.error("--blocks and --rect need --bsgs N1")
    grouped = tuple(int(v) for v in a.grouped.split(",")) if a.grouped else None
    if a.fold_grouped and not (a.bsgs and a.rect and grouped is not None):
        ap.error("--fold-grouped needs --bsgs N1 --rect --grouped K,G")
    if grouped is not None and a.rect and not a.fold_grouped:
        ap.error("--rect goes through tfhe_matmul_bsgs_fold, which refuses grouped keys: --grouped K,G goes with --bsgs N1 [--blocks] only")
    if grouped is not None and (len(grouped) != 2 or bool(a.hoisted) == bool(a.bsgs) or a.mul_relin):
        ap.error("--grouped K,G needs either --hoisted or --bsgs N1 [--blocks], and does not go with --mul-relin")
    if a.mul_relin_grouped and (grouped is None or not a.hoisted):
        ap.error("--mul-relin-grouped needs --hoisted --grouped K,G")
    run(a.logn, a.seed, model=a.model, batches=a.batches, hoisted=a.hoisted, repeat=a.repeat, fused=a.fused, mul_relin=a.mul_relin, bsgs=a.bsgs,
        blocks=a.blocks, rect=a.rect, grouped=grouped, mul_relin_grouped=a.mul_relin_grouped, fold_grouped=a.fold_grouped)
