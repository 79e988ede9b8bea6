"""Host-side mirror of ToyFHE's generic RLWE scheme and its BFV / BGV / CKKS / ModulusRaised parameter
wrappers, over device-resident ``RingElement``s (see ring.py).

Mirrors ``src/rlwe_she.jl`` (keys, CipherText, keygen/encrypt/decrypt, ``+ - *``, ``keyswitch``,
``rotate``), ``src/bfv.jl`` (π, π⁻¹, mul_expand / mul_contract), ``src/bgv.jl``, ``src/ckks.jl`` +
``src/ckksencoding.jl`` (encode / decode, ct ``modswitch``) and ``src/modulusraising.jl``.  The heavy
operations -- ring products, ``enc_mul`` for BFV, ``keyswitch``, ``rotate``, ``modswitch`` -- run as
single fused calls into libtoyfhe_hip.so; key generation, encryption and decryption are, as in the
reference, thin host-side callers of ring arithmetic.

Randomness cannot match Julia's (MersenneTwister + a forked Distributions); parity is defined on the
deterministic operations given inputs.  Samplers take a ``numpy.random.Generator``.
"""
from __future__ import annotations

import math
import os
from fractions import Fraction

import numpy as np

from . import native
from .native import PLAIN_BFV, PLAIN_BGV, BfvPlan, DeviceBuffer, PlainPlan, UsageError
from .ring import NegacyclicRing, RingElement, plaintext_space as _plaintext_space

DOT_MAX = 64   # operands / rotations one device pass of tfhe_dot, tfhe_lincomb[_many], tfhe_matmul_diag takes (TFHE_DOT_MAX, csrc/kernels.h)

# --------------------------------------------------------------------------------------------------
# samplers (poly.jl:7-23, crt.jl:146-148,277-279, bgv.jl:27-34)
# --------------------------------------------------------------------------------------------------


class DeviceRng:
    """Counter-based generator for the device samplers (tfhe_sample_uniform / tfhe_sample_gaussian): Philox4x32-10 keyed by
    the 64-bit `seed`.  Every draw of a polynomial takes a fresh value of the polynomial counter, which is its own counter
    word (separate from the coefficient index), so no two draws -- for rings of any degree -- ever share a counter; uniform
    and Gaussian draws additionally use different stream ids (0 / 1).  Passing a DeviceRng where the mirror takes an `rng`
    makes keygen / encrypt sample on the GPU (no host round trip).

    This is a reproducible statistical generator for tests and benchmarks, NOT a cryptographically secure one (64-bit key,
    Philox is not a CSPRNG): production keys must come from a CSPRNG on the host (`numpy.random.Generator` over
    `os.urandom`-seeded state is accepted wherever an `rng` is)."""

    def __init__(self, seed: int):
        self.seed, self.next_poly = int(seed) & (2**64 - 1), 0

    def take(self, n: int) -> int:
        first, self.next_poly = self.next_poly, self.next_poly + n
        return first


def _device_sample(rng: DeviceRng, ring: NegacyclicRing, batch, gaussian=None):
    if ring.idx != list(range(ring.L)):
        raise UsageError("device sampling: the ring must be a prefix of its context")
    n = 1 if batch is None else int(batch)
    out = DeviceBuffer(n * ring.L * ring.N)
    first = rng.take(n)
    if gaussian is None:
        ring.ctx.sample_uniform(ring.L, rng.seed, 0, first, out.ptr, n)
    else:
        sigma, mult = gaussian
        ring.ctx.sample_gaussian(ring.L, sigma, mult, rng.seed, 1, first, out.ptr, n)
    return RingElement(ring, out, None, batch)


def sample_uniform(rng, ring: NegacyclicRing, batch=None) -> RingElement:
    """RingSampler(ℛ, DiscreteUniform(coefftype)), poly.jl:7-23 / crt.jl:146-148,277-279: limb-wise independent."""
    if isinstance(rng, DeviceRng):
        return _device_sample(rng, ring, batch)
    shape = (ring.N,) if batch is None else (batch, ring.N)
    cols = [rng.integers(0, q, size=shape, dtype=np.uint64) for q in ring.moduli]
    return RingElement.from_host(ring, np.stack(cols, axis=len(shape) - 1))


def sample_noise(rng, ring: NegacyclicRing, sigma: float, batch=None, scale: int = 1) -> RingElement:
    """scale * round(N(0, sigma^2)) coefficients (𝒩 / 𝒢 of the schemes; rounded Gaussian as in test/bfv_crt.jl:34)."""
    if isinstance(rng, DeviceRng):
        return _device_sample(rng, ring, batch, gaussian=(sigma, scale))
    return lift_ints(ring, sample_normal_ints(rng, ring.N, sigma, batch), scale)


def sample_normal_ints(rng: np.random.Generator, N: int, sigma: float, batch=None):
    shape = (N,) if batch is None else (batch, N)
    return np.rint(rng.normal(0.0, sigma, size=shape)).astype(np.int64)


def lift_ints(ring: NegacyclicRing, ints: np.ndarray, scale: int = 1) -> RingElement:
    """small signed integers -> RNS residues (CRTEncoded(x::Integer), crt.jl:91-95)"""
    cols = [np.mod(ints.astype(object) * scale, q).astype(np.uint64) for q in ring.moduli]
    return RingElement.from_host(ring, np.stack(cols, axis=ints.ndim - 1))


# --------------------------------------------------------------------------------------------------
# scheme parameters
# --------------------------------------------------------------------------------------------------


class SHESchemeParams:
    relin_window = 0

    def R_cipher(self) -> NegacyclicRing:
        raise NotImplementedError

    def R_key(self) -> NegacyclicRing:      # ℛ_key, rlwe_she.jl:26
        return self.R_cipher()

    def noise(self, rng, ring, batch=None):  # 𝒩
        return sample_noise(rng, ring, self.sigma, batch)

    def secret_dist(self, rng, ring, batch=None):  # 𝒢
        return sample_noise(rng, ring, self.sigma, batch)

    def mul_expand(self, c):                 # rlwe_she.jl:39
        return None

    def encode(self, plaintext):             # π⁻¹
        raise NotImplementedError

    def decode(self, b):                     # π
        raise NotImplementedError


class BFVParams(SHESchemeParams):
    """BFVParams(ℛ, ℛbig, ℛplain, relin_window, σ, Δ), bfv.jl:5-19 (ℛplain given by its modulus t)."""

    scheme_name = "BFV"

    def __init__(self, ring: NegacyclicRing, ring_big: NegacyclicRing, t: int, relin_window: int = 0, sigma: float = 3.2):
        self.ring, self.ring_big, self.t, self.relin_window, self.sigma = ring, ring_big, int(t), relin_window, sigma
        self.delta = ring.modulus() // self.t            # test/bfv_crt.jl:35
        self._plan = None

    def R_cipher(self):
        return self.ring

    def plan(self) -> BfvPlan:
        if self._plan is None:
            self._plan = BfvPlan(self.ring.ctx, self.ring_big.ctx, self.t, self.ring.idx, self.ring_big.idx)
        return self._plan

    def mul_expand(self, c: RingElement) -> RingElement:
        """mul_expand for one component, bfv.jl:34: switch(ℛbig, c) (:202-226) -- the centred lift q -> Qbig, exact."""
        n = c.count
        out = DeviceBuffer(n * self.ring_big.L * self.ring_big.N)
        self.plan().expand(c.coeffs_primal().ptr, out.ptr, n)
        return RingElement(self.ring_big, out, None, c.batch)

    def mul_contract(self, e: RingElement) -> RingElement:
        """mul_contract for one component, bfv.jl:35-40: switch(ℛ, multround(e, t, q)) -- round-ties-away(t e / q), exact."""
        n = e.count
        out = DeviceBuffer(n * self.ring.L * self.ring.N)
        self.plan().contract(e.coeffs_primal().ptr, out.ptr, n)
        return RingElement(self.ring, out, None, e.batch)

    def plaintext_space(self):
        """ℛ_plain (bfv.jl:18, rlwe_she.jl:380-392): the psi = 0 host ring unless t is a prime with a 2N-th root."""
        return _plaintext_space(self.ring, self.t)

    def encode(self, plain) -> RingElement:
        """π⁻¹, bfv.jl:21-24: Δ * plaintext (a list of coefficients, or a list of such lists = a batch).  On the device
        (tfhe_plain_encode) whenever numpy holds the plaintext as int64 / uint64 without loss; Python big integers take the
        host path."""
        el = _device_encode(self, self.ring, PLAIN_BFV, plain)
        if el is not None:
            return el
        return self.ring(_map_plain(plain, lambda m: self.delta * (int(m) % self.t)))

    def _device_ring(self, b: RingElement) -> bool:
        # the device codec centres by the element's own Q; the reference centres by params.ring's (bfv.jl:26-29): the two agree
        # exactly when the element lives on params.ring's moduli (not so for ModulusRaised(BFV), whose ciphertext ring drops
        # the special prime -- that case stays on the host)
        return b.ring.N == self.ring.N and b.ring.moduli == self.ring.moduli

    def decode_array(self, b: RingElement) -> np.ndarray:
        """π as a uint64 array [N] / [batch][N] (tfhe_plain_decode when the element's ring is params.ring)."""
        if self._device_ring(b):
            a = _device_decode(self, b, PLAIN_BFV)
            if a is not None:
                return a
        return np.array(self._host_decode(b), dtype=np.uint64)

    def decode(self, b: RingElement):
        """π, bfv.jl:26-29: mod(SignedMod(divround(x, Δ)), t)."""
        if self._device_ring(b):
            a = _device_decode(self, b, PLAIN_BFV)
            if a is not None:
                return a.tolist()
        return self._host_decode(b)

    def _host_decode(self, b: RingElement):
        Q = self.ring.modulus()

        def one(x):
            v = x - Q if x > Q // 2 else x
            y = _div_ties_away(v, self.delta) % Q
            y = y - Q if y > Q // 2 else y
            return y % self.t
        return _map_plain(b.to_ints(), one)


class BGVParams(SHESchemeParams):
    """BGVParams(ℛ, ℛplain, σ), bgv.jl:5-34 (no relin_window field: keyswitch is unsupported, as upstream)."""

    scheme_name = "BGV"

    def __init__(self, ring: NegacyclicRing, t: int, sigma: float = 8 / math.sqrt(2 * math.pi)):
        self.ring, self.t, self.sigma = ring, int(t), sigma

    def R_cipher(self):
        return self.ring

    def noise(self, rng, ring, batch=None):  # ShiftedDiscreteNormal, bgv.jl:27-34
        return sample_noise(rng, ring, self.sigma, batch, self.t)

    def plaintext_space(self):
        """ℛ_plain (bgv.jl:18)."""
        return _plaintext_space(self.ring, self.t)

    def encode(self, plain):
        el = _device_encode(self, self.ring, PLAIN_BGV, plain)
        if el is not None:
            return el
        return self.ring(_map_plain(plain, lambda m: int(m) % self.t))

    # BGV's π centres by the element's own modulus, so the device codec of the element's ring (a plan per ring, cached here)
    # is exact for every ring with t < Q -- the ModulusRaised ciphertext ring included.
    def decode_array(self, b) -> np.ndarray:
        a = _device_decode(self, b, PLAIN_BGV)
        return a if a is not None else np.array(self._host_decode(b), dtype=np.uint64)

    def decode(self, b):
        a = _device_decode(self, b, PLAIN_BGV)
        return a.tolist() if a is not None else self._host_decode(b)

    def _host_decode(self, b):
        Q = b.ring.modulus()                 # the ciphertext's own level (a ModulusRaised / modswitched ring is a sub-basis)
        return _map_plain(b.to_ints(), lambda x: (x - Q if x > Q // 2 else x) % self.t)


class CKKSParams(SHESchemeParams):
    """CKKSParams(ℛ, relin_window, σ), ckks.jl:7-25."""

    scheme_name = "CKKS"

    def __init__(self, ring: NegacyclicRing, relin_window: int = 0, sigma: float = 8 / math.sqrt(2 * math.pi)):
        self.ring, self.relin_window, self.sigma = ring, relin_window, sigma

    def R_cipher(self):
        return self.ring

    def encode(self, plain):
        return plain  # π⁻¹(params, plaintext) = ℛ(plaintext), ckks.jl:21

    def decode(self, b):
        return b      # π(params, b) = b, ckks.jl:22


class ModulusRaised(SHESchemeParams):
    """ModulusRaised{P}, modulusraising.jl:12-21: the last CRT prime is a special prime reserved for keys."""

    def __init__(self, params: SHESchemeParams):
        self.params = params
        self.sigma = params.sigma
        self.relin_window = params.relin_window
        self.scheme_name = params.scheme_name + " (with special prime)"

    def R_cipher(self):
        return self.params.R_cipher().drop_last()

    def R_key(self):
        return self.params.R_key()

    def noise(self, rng, ring, batch=None):
        return self.params.noise(rng, ring, batch)

    def secret_dist(self, rng, ring, batch=None):
        return self.params.secret_dist(rng, ring, batch)

    def encode(self, plain):
        return self.params.encode(plain)

    def decode(self, b):
        return self.params.decode(b)

    def decode_array(self, b):
        return self.params.decode_array(b)


class GroupedRaised(SHESchemeParams):
    """Keys with grouped RNS digits and several special primes (the "hybrid" gadget; tfhe_keyswitch_grouped): the last `n_special`
    CRT primes of the key ring are reserved for keys, their product P pre-multiplies every key, and a digit of the key switch covers
    `group` limbs of the ciphertext ring.  ModulusRaised is the case (1, 1) on the per-limb routes; this class is deliberately not one
    of its subclasses: the fused routes test for ModulusRaised."""

    def __init__(self, params: SHESchemeParams, n_special: int, group: int):
        if params.relin_window != 0:
            raise UsageError("GroupedRaised takes RNS digits (relin_window = 0)")
        L = params.R_key().L
        if not 0 <= int(n_special) <= min(4, L - 1) or int(group) < 1:
            raise UsageError("GroupedRaised: n_special in [0, min(4, L - 1)] and group >= 1")
        self.params, self.n_special, self.group = params, int(n_special), int(group)
        self.sigma = params.sigma
        self.scheme_name = params.scheme_name + f" (with {self.n_special} special primes, {self.group} limbs per digit)"

    def R_cipher(self):
        ring = self.params.R_cipher()
        for _ in range(self.n_special):
            ring = ring.drop_last()
        return ring

    def R_key(self):
        return self.params.R_key()

    def noise(self, rng, ring, batch=None):
        return self.params.noise(rng, ring, batch)

    def secret_dist(self, rng, ring, batch=None):
        return self.params.secret_dist(rng, ring, batch)

    def encode(self, plain):
        return self.params.encode(plain)

    def decode(self, b):
        return self.params.decode(b)

    def decode_array(self, b):
        return self.params.decode_array(b)

    def digit_groups(self, level: int):
        """the limb ranges of the digits at `level`: groups of `group` limbs, the last one cut at the level"""
        return [range(g * self.group, min((g + 1) * self.group, level)) for g in range(-(-level // self.group))]


def _refuse_grouped(params, what: str):
    if isinstance(params, GroupedRaised):
        raise UsageError(f"{what} has no support for keys with grouped digits (GroupedRaised): keyswitch, rotate and modswitch take them")


def _refuse_grouped_keys(gks, what: str):
    for g in gks:     # (anything that is not a Galois key is the later checks' business)
        _refuse_grouped(getattr(getattr(g, "key", None), "params", None), what)


def _plain_plan(params, ring: NegacyclicRing):
    """the device codec of (ring, params.t), cached on the params object per ring; None when the device does not take it
    (t outside [2, 2^62) or not below the ring's modulus)"""
    cache = params.__dict__.setdefault("_plain_plans", {})
    key = (id(ring.ctx), tuple(ring.idx))
    if key not in cache:
        ok = 2 <= params.t < min(2**62, ring.modulus())
        cache[key] = PlainPlan(ring.ctx, params.t, ring.idx) if ok else None
    return cache[key]


def _device_decode(params, b: RingElement, scheme):
    """π on the device: uint64 [N] / [batch][N], or None when the plan cannot take this ring"""
    plan = _plain_plan(params, b.ring)
    if plan is None:
        return None
    n, N = b.count, b.ring.N
    out = DeviceBuffer(n * N)
    plan.decode(scheme, b.coeffs_primal().ptr, out.ptr, n)
    b.ring.ctx.sync()
    a = out.to_numpy((n, N))
    return a if b.batch is not None else a[0]


def _plain_array(plain, t: int, N: int):
    """the plaintext as uint64 [N] / [B][N] with negative values reduced mod t, or None when numpy cannot hold it as
    int64 / uint64 without loss (Python big integers, floats, ragged rows): those take the host path"""
    if isinstance(plain, np.ndarray):
        a = plain
    else:
        try:
            a = np.asarray(plain)
        except (ValueError, OverflowError, TypeError):
            return None
    if a.dtype.kind not in "iu" or a.ndim not in (1, 2) or a.shape[-1] != N or a.size == 0:
        return None
    if a.dtype.kind == "i":
        a = np.mod(a.astype(np.int64), np.int64(t))
    return np.ascontiguousarray(a, dtype=np.uint64)


def _device_encode(params, ring: NegacyclicRing, scheme, plain):
    """π⁻¹ on the device (tfhe_plain_encode) into `ring`, or None (host path)"""
    a = _plain_array(plain, params.t, ring.N)
    if a is None:
        return None
    plan = _plain_plan(params, ring)
    if plan is None:
        return None
    n = 1 if a.ndim == 1 else a.shape[0]
    src = DeviceBuffer.from_numpy(a)
    out = DeviceBuffer(n * ring.L * ring.N)
    plan.encode(scheme, src.ptr, out.ptr, n)               # (src is parked by the allocator until the kernel has read it)
    return RingElement(ring, out, None, None if a.ndim == 1 else n)


def _map_plain(plain, f):
    if len(plain) and hasattr(plain[0], "__len__"):
        return [[f(m) for m in row] for row in plain]
    return [f(m) for m in plain]


def _div_ties_away(x: int, y: int) -> int:
    """div(x, y, RoundNearestTiesAway), div_hacks.jl:120-135 (y > 0)."""
    q, r = divmod(abs(x), y)
    if 2 * r >= y:
        q += 1
    return q if x >= 0 else -q


# --------------------------------------------------------------------------------------------------
# keys and ciphertexts (rlwe_she.jl:67-149)
# --------------------------------------------------------------------------------------------------


class KeyComponent:
    def __init__(self, mask: RingElement, masked: RingElement):
        self.mask, self.masked = mask, masked


class PrivKey:
    def __init__(self, params, secret: RingElement):
        self.params, self.secret = params, secret


class PubKey:
    def __init__(self, params, key: KeyComponent):
        self.params, self.key = params, key


class KeyPair:
    def __init__(self, priv: PrivKey, pub: PubKey):
        self.priv, self.pub = priv, pub


class KeySwitchKey:
    """KeySwitchKey{P}(params, key::Vector{KeyComponent}), rlwe_she.jl:87-91.  ``packed()`` is the device
    layout the C ABI consumes: [n_digits][2 = mask, masked][Lk][N], NTT domain."""

    def __init__(self, params, key):
        self.params, self.key = params, list(key)
        self._packed = None

    def packed(self) -> DeviceBuffer:
        if self._packed is None:
            ring = self.key[0].mask.ring
            sz = ring.L * ring.N
            buf = DeviceBuffer(len(self.key) * 2 * sz)
            for i, kc in enumerate(self.key):
                for s, el in enumerate((kc.mask, kc.masked)):
                    native.check(native.lib().tfhe_memcpy_d2d(ring.ctx.h, buf.ptr + ((i * 2 + s) * sz) * 8,
                                                              el.coeffs_dual().ptr, sz * 8))   # once per key
            ring.ctx.sync()
            self._packed = buf
        return self._packed


class EvalMultKey:
    def __init__(self, key: KeySwitchKey):
        self.key = key


class GaloisKey:
    def __init__(self, galois_element: int, key: KeySwitchKey):
        self.galois_element, self.key = galois_element, key
        self._prepared = None

    def _prepare(self) -> DeviceBuffer:
        """the packed key with its NTT-domain rows permuted by g^-1 (tfhe_galois_key_prepare, which does not care what a digit is), once
        per key"""
        if self._prepared is None:
            ring = self.key.key[0].mask.ring
            src = self.key.packed()
            dst = DeviceBuffer(src.n)
            ring.ctx.galois_key_prepare(ring.L, len(self.key.key), self.galois_element, src.ptr, dst.ptr)
            self._prepared = dst
        return self._prepared

    def prepared(self) -> DeviceBuffer:
        """the prepared key of the per-limb hoisted rotations (rotate_many, matmul_*, the prepared-key rotation): they have no grouped
        form, so a key with grouped digits is refused here"""
        _refuse_grouped(self.key.params, "GaloisKey.prepared (hoisted rotations)")
        return self._prepare()

    def prepared_grouped(self) -> DeviceBuffer:
        """the prepared key of rotate_many_grouped and matmul_diag_grouped: a key with grouped digits (GroupedRaised) only"""
        if not isinstance(self.key.params, GroupedRaised):
            raise UsageError("GaloisKey.prepared_grouped takes a key with grouped digits (GroupedRaised); the others go through prepared()")
        return self._prepare()


# the forward transforms of many small ring elements in one launch (CipherText.dot_plain).  Above _BATCH_NTT_MAX_WORDS a single element's
# transform fills the chip by itself; a chunk stages at most _BATCH_NTT_CHUNK_WORDS (1 GiB) of coefficients, and as much of results.
_BATCH_NTT_MAX_WORDS = 0 if os.environ.get("TFHE_BATCH_NTT", "1") == "0" else 1 << 25   # TFHE_BATCH_NTT=0: one transform per element (comparisons)
_BATCH_NTT_CHUNK_WORDS = 1 << 27


def _stage_buffers(ctx, words):
    """the context's two staging buffers (coefficients in, evaluation-domain rows out), grown on demand and kept for the context's
    lifetime: everything that touches them is enqueued on the context's own stream, so a chunk may reuse them as soon as the previous
    chunk's calls are enqueued.  (r06: fresh multi-GiB buffers per call went through the recycling allocator -- past its soft threshold
    every first-time size is a device drain, `hipFree` of stale blocks and a `hipMalloc`: the reference-shaped MNIST pass ran 215 ms on its
    own and 520-680 ms behind the restructured case in one process.)"""
    st = getattr(ctx, "_ntt_stage", None)
    if st is None or st[0].n < words:
        ctx._ntt_stage = st = (DeviceBuffer(words), DeviceBuffer(words))
    return st


def release_staging(ctx):
    """give the staging buffers of `_stage_buffers` back (they are re-created on the next use)"""
    if getattr(ctx, "_ntt_stage", None) is not None:
        ctx._ntt_stage = None


class _PackedComponent:
    """component p of a key-switch result that is still one packed buffer [count][P][L][N] (_PackedResult): an operand of _dot_batched
    that is staged by the strided copy which would otherwise have split it off"""
    dual = None

    def __init__(self, owner, image, P, p):
        self.owner, self.image, self.P, self.p = owner, image, P, p

    def coeffs_dual(self):                                   # (the un-batched paths: the owner's ring element after all)
        return self.owner.cs[self.p].coeffs_dual()


def _component_source(c, p):
    """component p of ciphertext c as an operand of _dot_batched: the ring element, or -- for a result that has not been split --
    its place in the packed buffer"""
    if isinstance(c, _PackedResult) and c._cs is None:
        return _PackedComponent(c, c._packed_image[0], 2, p)
    return c.cs[p]


# TFHE_DOT_PLAIN_CALL=0: CipherText.dot_plain stages and transforms its operands itself (_dot_batched below: copies into the context's
# staging buffers, one tfhe_nntt, tfhe_dot) -- comparisons; the default is ONE tfhe_dot_plain call per component on view operands,
# with no staging copy and no staging buffer: the same words.
_DOT_PLAIN_CALL = os.environ.get("TFHE_DOT_PLAIN_CALL", "1") != "0"
# the largest log2 N at which dot_plain takes the call (TFHE_DOT_PLAIN_CALL_MAX_LOG2).  Above the fused sizes the call's composed form
# does the staging route's work below the ABI and measured level with it at N = 2^16, not faster (profiles/LOG.md), so the staging route stays
# there.
_DOT_PLAIN_CALL_MAX_LOG2 = int(os.environ.get("TFHE_DOT_PLAIN_CALL_MAX_LOG2", "14"))


def _dot_call(ring, n, cts, p, plains, dst):
    """dst = sum_k component p of cts[k] .* plains[k] in one tfhe_dot_plain call.  A ring element is a dense view (its cached
    transform, if there is one, as a transformed term); component p of a key-switch result that has not been split is a view into
    its packed buffer [n][2][L][N], which stays unsplit."""
    words = ring.L * ring.N
    views = []
    for c in cts:
        if isinstance(c, _PackedResult) and c._cs is None:
            views.append((c._packed_image[0].ptr + p * words * 8, 2 * words, False))
        else:
            e = c.cs[p]
            views.append((e.dual.ptr, words, True) if e.dual is not None else (e.coeffs_primal().ptr, words, False))
    ring.ctx.dot_plain(None, views, [(x.ptr, words) for x in plains], (dst.ptr, words), n, ring.L, ring.idx)


def _dot_batched(ring, n, elems, pb_ptrs, dst):
    """dst = sum_k elems[k] .* plain_k for ring elements of ONE ring and batch size, the plaintexts given by their evaluation-domain
    pointers.  Elements whose transform is cached are used where they lie.  When two or more are still in the coefficient domain
    and small against the chip (r06: a batch of 16 ciphertext components at N = 2^16 is 16 rows of a 60-bit limb -- 64 of the 256
    workgroup slots -- per call; the reference-shaped matrix product of infer.jl:140-149 asks for 2 x 63 such transforms, one per
    rotated ciphertext) the sum runs chunk by chunk: a chunk's operands are copied side by side into the context's staging buffer,
    transformed in ONE call, and accumulated onto dst (tfhe_dot with dst as its running sum: residues are canonical, so the partial
    sums are the same words as one pass over all terms).  The transforms are the same per row: bit for bit `coeffs_dual()`.
    Nothing is cached on the elements."""
    words = n * ring.L * ring.N
    todo = sum(1 for e in elems if e.dual is None)
    if todo < 2 or words > _BATCH_NTT_MAX_WORDS:
        ring.ctx.dot(None, [e.coeffs_dual().ptr for e in elems], pb_ptrs, dst.ptr, n, ring.L, ring.idx)
        return
    per = max(2, _BATCH_NTT_CHUNK_WORDS // words)
    lib = native.lib()
    acc = None
    for a in range(0, len(elems), per):
        part = elems[a:a + per]
        stage = [e for e in part if e.dual is None]
        ptrs = [e.dual.ptr if e.dual is not None else None for e in part]
        if len(stage) == 1:                                  # (a lone straggler of the last chunk: its own transform)
            i = ptrs.index(None)
            ptrs[i] = stage[0].coeffs_dual().ptr
        elif stage:
            src, dual = _stage_buffers(ring.ctx, len(stage) * words)
            for k, e in enumerate(stage):
                if isinstance(e, _PackedComponent):          # straight out of an unsplit key-switch result: the one strided copy
                    native.check(lib.tfhe_unpack_poly(ring.ctx.h, src.ptr + k * words * 8, e.image.ptr, e.P, e.p, ring.L * ring.N, n))
                else:
                    native.check(lib.tfhe_memcpy_d2d(ring.ctx.h, src.ptr + k * words * 8, e.coeffs_primal().ptr, words * 8))
            ring.ctx.nntt(src.ptr, dual.ptr, len(stage) * n, ring.L, ring.idx)
            k = 0
            for i, e in enumerate(part):
                if ptrs[i] is None:
                    ptrs[i] = dual.ptr + k * words * 8
                    k += 1
        ring.ctx.dot(acc, ptrs, pb_ptrs[a:a + per], dst.ptr, n, ring.L, ring.idx)
        acc = dst.ptr


class CipherText:
    """CipherText{Plain,P,T,N}(params, cs), rlwe_she.jl:131-149.  ``scale`` carries the CKKS FixedRational
    denominator (a type parameter upstream, ckksencoding.jl:3-15)."""

    def __init__(self, params, cs, scale=None):
        self.params, self._cs, self.scale = params, tuple(cs), scale
        # (packed [count][polys][L][N] image, the component buffers it was split into): a key switch / rotation returns its packed
        # result split into ring elements (strided copies); a chained caller (infer.jl:140-149: rotated = rotate(gk, rotated)) hands
        # the same elements straight back, and the next call takes the image instead of packing them again.  Ring elements never
        # change a device buffer in place (setindex! replaces it), so identity of the buffers is validity of the image.
        self._packed_image = None

    def _remember_packed(self, image, ctx):
        self._packed_image = (image, ctx, tuple(x.primal for x in self.cs))
        return self

    def _packed_for(self, prim, ctx, consume=False):
        """the packed image of exactly these coefficient buffers on this context, or None.  ``consume``: the image is handed
        over and forgotten (r06, ADVICE r05: a result ciphertext otherwise holds its packed buffer next to the unpacked
        components -- twice the device memory -- for as long as it lives; a chained caller uses it exactly once)"""
        pi = self._packed_image
        if pi is not None and pi[1] is ctx and len(pi[2]) == len(prim) and all(a is b for a, b in zip(pi[2], prim)):
            if consume:
                self._packed_image = None
            return pi[0]
        if consume:
            self._packed_image = None      # stale (a component was replaced): nothing can use it any more
        return None

    @property
    def cs(self):
        """the components (ring elements).  A deferred form (_ScalarSum) evaluates itself on the first access."""
        if self._cs is None:
            self._cs = tuple(self._evaluate())
        return self._cs

    @cs.setter
    def cs(self, v):
        self._cs = tuple(v)

    def _evaluate(self):
        raise AssertionError("a plain ciphertext always has its components")

    def __len__(self):
        return len(self.cs)

    def __getitem__(self, i):
        return self.cs[i]

    def ring(self):
        return self.cs[0].ring

    def _shape(self):
        """(polynomials per component, batch) without evaluating a deferred form"""
        return self.cs[0].count, self.cs[0].batch

    def __repr__(self):
        return f"{self.params.scheme_name} ciphertext (length {len(self)})"

    # homomorphic arithmetic, rlwe_she.jl:231-266
    def _addsub(self, o, sub):
        if self.params is not o.params:
            raise UsageError("Attempting to add ciphertexts with differing parameters")
        if isinstance(self, _ScalarSum) and isinstance(o, _ScalarSum):
            both = self._joined(o, sub)
            if both is not None:
                return both
        n = max(len(self), len(o))
        cs = []
        for i in range(n):
            if i >= len(self):
                cs.append(-o[i] if sub else o[i])
            elif i >= len(o):
                cs.append(self[i])
            else:
                cs.append(self[i] - o[i] if sub else self[i] + o[i])
        return CipherText(self.params, cs, self.scale)

    def __add__(self, o):
        if isinstance(o, RingElement):  # +(c, b::T), rlwe_she.jl:243-245
            return CipherText(self.params, (self.cs[0] + o,) + self.cs[1:], self.scale)
        return self._addsub(o, False)

    def __sub__(self, o):
        return self._addsub(o, True)

    def __mul__(self, o):
        if isinstance(o, CipherText):
            if (self.scale is None) != (o.scale is None):
                raise UsageError("multiplying a scaled (CKKS) ciphertext by an unscaled one")
            scale = None if self.scale is None else self.scale * o.scale  # ckksencoding.jl:133-135
            return CipherText(self.params, enc_mul(self, o), scale)
        if isinstance(o, int):
            return CipherText(self.params, [c * o for c in self.cs], self.scale)
        if isinstance(o, float):                     # ct * b::AbstractFloat, ckksencoding.jl:99-102
            return self.mul_plain(o)
        raise TypeError(type(o))

    __rmul__ = __mul__

    # ---- CKKS plaintext operands (ckksencoding.jl:99-124); the ciphertext carries its scale ----
    def _need_scale(self):
        if self.scale is None:
            raise UsageError("plaintext operands need a CKKS ciphertext (with a scale)")

    def mul_plain(self, x) -> "CipherText":
        """ct * float (:99-102) or vector .* ct (:104-109): the operand is brought to the ciphertext's scale, every
        component is multiplied by it; the result's scale is the square."""
        self._need_scale()
        if np.isscalar(x):
            fr = Fraction(float(x)) * Fraction(self.scale)
            fl = fr.numerator // fr.denominator
            rem = fr - fl
            scaled = fl + (1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2) else 0)   # FixedRational(b).x, ckks.jl:42
            if _LAZY_SCALAR_SUMS:
                return _ScalarSum.term(self, int(scaled))
            cs = [c * int(scaled) for c in self.cs]
        elif isinstance(x, RingElement):             # a plaintext the caller has encoded at this ciphertext's scale already
            if x.ring != self.ring():
                raise UsageError("pre-encoded plaintext belongs to another ring")
            cs = [c * x for c in self.cs]
        else:
            re = ckks_encode(np.asarray(x, dtype=np.complex128), self.ring(), self.scale)
            cs = [c * re for c in self.cs]
        return CipherText(self.params, cs, Fraction(self.scale) ** 2)

    @staticmethod
    def dot_plain(cts, plains) -> "CipherText":
        """sum_k cts[k] .* plains[k] for ciphertexts of one ring, length and scale and plaintexts already encoded at that scale
        (ring elements): the accumulation loop of the diagonal matrix product (infer.jl:140-149) as one device pass per
        component (tfhe_dot_plain: the operands' forward transforms run inside the call, unsplit key-switch results are read
        where they lie) instead of a ring multiplication and a ring addition per term; bit-identical to
        `sum(c.mul_plain(p) for c, p in zip(cts, plains))`."""
        cts, plains = list(cts), list(plains)
        if not cts or len(cts) != len(plains):
            raise AssertionError("dot_plain: as many ciphertexts as plaintexts, at least one")
        c0 = cts[0]
        c0._need_scale()
        ring = c0.ring()
        n, batch = c0._shape()
        for c in cts:
            if c.ring() != ring or len(c) != len(c0) or c.scale != c0.scale or c._shape()[0] != n:
                raise UsageError("dot_plain: ciphertexts of one ring, length, batch and scale")
        for p in plains:
            if not isinstance(p, RingElement) or p.ring != ring or p.count != n:
                raise UsageError("dot_plain: plaintexts must be ring elements of the ciphertexts' ring and batch")
        pb = [p.coeffs_dual() for p in plains]
        out = []
        for s_ in range(len(c0)):
            o = DeviceBuffer(n * ring.L * ring.N)
            if _DOT_PLAIN_CALL and ring.N <= (1 << _DOT_PLAIN_CALL_MAX_LOG2):
                _dot_call(ring, n, cts, s_, pb, o)
            else:
                _dot_batched(ring, n, [_component_source(c, s_) for c in cts], [x.ptr for x in pb], o)
            out.append(RingElement(ring, None, o, batch))
        return CipherText(c0.params, out, Fraction(c0.scale) ** 2)

    @staticmethod
    def _weight_residues(w: float, scale, moduli):
        """FixedRational(w).x at the ciphertext's scale, ckks.jl:42 (ties to even), as residues.  Integer arithmetic on the
        float's exact ratio (a layer has hundreds of weights: Fraction objects cost a millisecond per call)."""
        n, d = float(w).as_integer_ratio()
        sc = scale if isinstance(scale, Fraction) else Fraction(scale)
        num, den = n * sc.numerator, d * sc.denominator
        fl, rem = divmod(num, den)
        v = fl + (1 if 2 * rem > den or (2 * rem == den and fl % 2) else 0)
        return [v % q for q in moduli]

    @staticmethod
    def lincomb(cts, weights) -> "CipherText":
        """sum_k cts[k] * weights[k] for float weights (ct * float, ckksencoding.jl:99-102, and the + of rlwe_she.jl:231-245 per
        term): the scalar-weighted sums of a convolution over encrypted inputs (infer.jl:127-129) as ONE device pass per
        component (tfhe_lincomb); bit-identical to `sum(c.mul_plain(w) for c, w in zip(cts, weights))`."""
        return CipherText.lincomb_many(cts, [weights])[0]

    @staticmethod
    def lincomb_many(cts, weight_rows) -> "list[CipherText]":
        """[sum_k cts[k] * row[k] for row in weight_rows]: several weighted sums of the SAME ciphertexts -- the output channels of
        a convolution layer (infer.jl:127-131: every channel weighs the same 49 encrypted inputs) -- with one pass over the
        operands per component (tfhe_lincomb_many); each result bit-identical to `lincomb(cts, row)`."""
        cts = list(cts)
        rows = [[float(w) for w in row] for row in weight_rows]
        if not cts or not rows or any(len(r) != len(cts) for r in rows):
            raise AssertionError("lincomb: as many ciphertexts as weights, at least one")
        if len(cts) > DOT_MAX:      # a device pass takes DOT_MAX operands: longer sums as partial sums (the same residues: + is exact)
            parts = [CipherText.lincomb_many(cts[k:k + DOT_MAX], [r[k:k + DOT_MAX] for r in rows]) for k in range(0, len(cts), DOT_MAX)]
            outs = parts[0]
            for more in parts[1:]:
                outs = [a + b for a, b in zip(outs, more)]
            return outs
        c0 = cts[0]
        c0._need_scale()
        ring, n, batch = c0.ring(), c0[0].count, c0[0].batch
        for c in cts:
            if c.ring() != ring or len(c) != len(c0) or c.scale != c0.scale or c[0].count != n:
                raise UsageError("lincomb: ciphertexts of one ring, length, batch and scale")
        sc, mods = Fraction(c0.scale), list(ring.moduli)
        scal = [[CipherText._weight_residues(w, sc, mods) for w in row] for row in rows]
        primal = all(c.cs[0].primal is not None for c in cts)   # stay in the domain the operands are in
        comps = [[] for _ in rows]
        for s_ in range(len(c0)):
            ab = [(c.cs[s_].coeffs_primal() if primal else c.cs[s_].coeffs_dual()) for c in cts]
            outs = [DeviceBuffer(n * ring.L * ring.N) for _ in rows]
            if len(rows) == 1:
                ring.ctx.lincomb(scal[0], [x.ptr for x in ab], outs[0].ptr, n, ring.L, ring.idx)
            else:
                ring.ctx.lincomb_many(scal, [x.ptr for x in ab], [o.ptr for o in outs], n, ring.L, ring.idx)
            for k, o in enumerate(outs):
                comps[k].append(RingElement(ring, o, None, batch) if primal else RingElement(ring, None, o, batch))
        return [CipherText(c0.params, out, Fraction(c0.scale) ** 2) for out in comps]

    @staticmethod
    def concat(cts) -> "CipherText":
        """the batches of several ciphertexts (same parameters, length and scale) as one batched ciphertext: the independent
        ciphertexts of one circuit layer share every device call that follows"""
        cts = list(cts)
        c0 = cts[0]
        if any(len(c) != len(c0) or c.scale != c0.scale or c.ring() != c0.ring() for c in cts):
            raise UsageError("concat: ciphertexts of one ring, length and scale")
        return CipherText(c0.params, [RingElement.concat([c.cs[s_] for c in cts]) for s_ in range(len(c0))], c0.scale)

    def split(self, sizes) -> "list[CipherText]":
        """inverse of concat"""
        parts = [x.split(sizes) for x in self.cs]
        return [CipherText(self.params, [p[k] for p in parts], self.scale) for k in range(len(sizes))]

    def add_plain(self, x) -> "CipherText":
        """ct .+ float / ct .+ vector (:111-124): encoded at the ciphertext's scale and added to the first component."""
        self._need_scale()
        n2 = self.ring().N // 2
        v = np.full(n2, x, dtype=np.complex128) if np.isscalar(x) else np.asarray(x, dtype=np.complex128)
        re = ckks_encode(v, self.ring(), self.scale)
        return CipherText(self.params, (self.cs[0] + re,) + self.cs[1:], self.scale)


# ct * float + ct * float + ... (infer.jl:127-129: `sum(C[i,j] * w[i,j] for i, j)`, 49 terms per channel) term by term is a scalar
# multiplication and an addition per term and component -- two passes over a ciphertext each, 27 us apiece at the example's batch, 784
# launches per pass.  TFHE_LAZY_SUMS=0 keeps that.
_LAZY_SCALAR_SUMS = os.environ.get("TFHE_LAZY_SUMS", "1") != "0"
_LAZY_UNPACK = os.environ.get("TFHE_LAZY_UNPACK", "1") != "0"      # key-switch / rotation results stay packed until their components are asked for


class _ScalarSum(CipherText):
    """sum_k s_k x_k, s_k integers (FixedRational(w).x of `ct * float`, ckksencoding.jl:99-102), NOT YET EVALUATED: `mul_plain(float)`
    returns one term, `+` / `-` of two such sums joins their terms, and the first use of the components evaluates the whole sum in one
    device pass per component and DOT_MAX terms (tfhe_lincomb) -- the same residues as the term-by-term evaluation, every operation being
    exact modulo each q.  What is captured per term is the DEVICE BUFFERS of the operand's components at the time of the
    multiplication (ring elements never change a buffer in place: setindex! replaces it), so a later change of the operand does not
    reach the sum -- the value semantics of the eager form.  Errors of the eager form are raised where it would raise them
    (`_need_scale` in mul_plain, differing parameters in `+`); sums that do not fit together (ring, batch, length, scale, domain)
    are evaluated and added as ordinary ciphertexts."""

    def __init__(self, params, scale, ring, n, batch, domain, terms):
        self.params, self._cs, self.scale = params, None, scale
        self._packed_image = None
        self._ring, self._n, self._batch, self._domain, self._terms = ring, n, batch, domain, terms

    @staticmethod
    def term(c: CipherText, scalar: int) -> "_ScalarSum":
        cs = c.cs
        primal = all(x.primal is not None for x in cs)             # stay in the domain the operand is in
        bufs = tuple(x.coeffs_primal() if primal else x.coeffs_dual() for x in cs)
        return _ScalarSum(c.params, Fraction(c.scale) ** 2, cs[0].ring, cs[0].count, cs[0].batch, primal, [(bufs, scalar)])

    def _joined(self, o, sub):
        if self._cs is not None or o._cs is not None:               # one of them has been evaluated already: ordinary ciphertexts
            return None
        if (self._ring != o._ring or self._n != o._n or self._batch != o._batch or self._domain != o._domain or self.scale != o.scale
                or len(self._terms[0][0]) != len(o._terms[0][0])):
            return None
        more = [(b, -k) for b, k in o._terms] if sub else list(o._terms)
        return _ScalarSum(self.params, self.scale, self._ring, self._n, self._batch, self._domain, self._terms + more)

    def __len__(self):
        return len(self._terms[0][0]) if self._cs is None else len(self._cs)

    def ring(self):
        return self._ring

    def _shape(self):
        return self._n, self._batch

    def _evaluate(self):
        ring, n = self._ring, self._n
        mods = list(ring.moduli)
        out = []
        for s_ in range(len(self._terms[0][0])):
            acc = None
            for a in range(0, len(self._terms), DOT_MAX):           # a device pass takes DOT_MAX operands (+ is exact)
                part = self._terms[a:a + DOT_MAX]
                o = DeviceBuffer(n * ring.L * ring.N)
                ring.ctx.lincomb([[k % q for q in mods] for _, k in part], [b[s_].ptr for b, _ in part], o.ptr, n, ring.L, ring.idx)
                el = RingElement(ring, o, None, self._batch) if self._domain else RingElement(ring, None, o, self._batch)
                acc = el if acc is None else acc + el
            out.append(acc)
        self._terms = None                                          # the operands' buffers are no longer needed
        return out


class _PackedResult(CipherText):
    """The result of a key switch / rotation as the device call left it: ONE packed buffer [count][2][L][N] on the key ring's context,
    split into ring elements only when somebody asks for the components (r06).  The chained rotations of infer.jl:140-149 never do:
    rotation k + 1 takes the packed buffer as its input, and the accumulation (`CipherText.dot_plain`) stages its operands straight
    out of the packed buffers -- two strided copies and two buffers per rotation less than splitting every result.  Evaluated, it
    is an ordinary ciphertext that remembers its packed image (`_packed_image`, as before)."""

    def __init__(self, params, scale, image, ctx, ring, n, batch):
        self.params, self._cs, self.scale = params, None, scale
        self._packed_image = (image, ctx, None)
        self._ring, self._n, self._batch = ring, n, batch

    def _deferred_image(self, ctx):
        """the packed buffer if the components have not been asked for and it lives on `ctx`, else None (it stays with this ciphertext)"""
        pi = self._packed_image
        return pi[0] if self._cs is None and pi is not None and pi[1] is ctx else None

    def __len__(self):
        return 2

    def ring(self):
        return self._ring

    def _shape(self):
        return self._n, self._batch

    def _evaluate(self):
        image, ctx, _ = self._packed_image
        cs = _unpack(image, self._ring, self._n, 2, self._batch, primal=True, ctx=ctx)
        if self._ring.ctx is not ctx:
            self._ring.ctx.wait_for(ctx)                   # the components are elements of the ciphertext ring: its stream must see them written
        self._packed_image = (image, ctx, tuple(x.primal for x in cs))
        return cs


# --------------------------------------------------------------------------------------------------
# keygen / encrypt / decrypt (rlwe_she.jl:155-217, modulusraising.jl:23-26)
# --------------------------------------------------------------------------------------------------


def keygen(rng, params) -> KeyPair:
    """keygen(rng, params), rlwe_she.jl:155-166.  With the stock samplers the public key -(mask s + e) is ONE device call
    (tfhe_evalkey_gen without a gadget): the same words and the same generator state as the composition below."""
    ring = params.R_key()
    if _keygen_device_ok(rng, params, ring):
        return _keygen_device(rng, params, ring)
    return _keygen_composed(rng, params)


def _keygen_composed(rng, params) -> KeyPair:
    ring = params.R_key()
    mask = sample_uniform(rng, ring)
    secret = params.secret_dist(rng, ring)
    error = params.noise(rng, ring)
    masked = -(mask * secret + error)
    return KeyPair(PrivKey(params, secret), PubKey(params, KeyComponent(mask, masked)))


# TFHE_FUSED_ENCRYPT=0: encrypt / decrypt as the reference's term-by-term expressions on ring elements (comparisons); the default
# is one device call each (tfhe_encrypt / tfhe_decrypt_phase) -- the same residues, the same generator state afterwards.
_FUSED_ENCRYPT = os.environ.get("TFHE_FUSED_ENCRYPT", "1") != "0"


def _is_prefix(ring: NegacyclicRing) -> bool:
    return ring.idx == list(range(ring.L))


def _noise_multiplier(params):
    """the multiplier of 𝒩 when the scheme draws 𝒢 and 𝒩 through the stock samplers (1; t for BGV, bgv.jl:27-34), else None"""
    inner = params.params if isinstance(params, (ModulusRaised, GroupedRaised)) else params
    if type(inner) in (BFVParams, CKKSParams):
        return 1
    return inner.t if type(inner) is BGVParams else None


def _packed_pubkey(pub: PubKey, keyring: NegacyclicRing) -> DeviceBuffer:
    """[2][L_key][N] (mask, masked), NTT domain: the layout of one evaluation-key digit, packed once per key"""
    if getattr(pub, "_packed", None) is None:
        pub._packed = _pack([pub.key.mask.coeffs_dual(), pub.key.masked.coeffs_dual()], keyring, 1)
    return pub._packed


def _encrypt_device(rng, pub: PubKey, batch, enc: RingElement | None, scale):
    """encrypt_zero (+ the encoded message) as ONE device call, or None when this key / generator / message is not covered"""
    params = pub.params
    mult = _noise_multiplier(params)
    keyring, ring = params.R_key(), params.R_cipher()
    if not _FUSED_ENCRYPT or mult is None or not (isinstance(rng, (DeviceRng, np.random.Generator))):
        return None
    if not _is_prefix(keyring) or ring.ctx is not keyring.ctx or not _is_prefix(ring) or ring.L > keyring.L:
        return None
    if pub.key.mask.ring.ctx is not keyring.ctx or pub.key.mask.ring.idx != keyring.idx or pub.key.mask.batch is not None:
        return None
    if enc is not None and (enc.ring.ctx is not ring.ctx or enc.ring.idx != ring.idx or enc.batch != batch):
        return None
    n, N = (1 if batch is None else int(batch)), ring.N
    ctx = keyring.ctx
    pk = _packed_pubkey(pub, keyring)
    msg = None if enc is None else enc.coeffs_primal()
    out = DeviceBuffer(n * 2 * ring.L * N)
    if isinstance(rng, DeviceRng):
        # u, e1, e2: n counters each, in the order the three separate draws take them
        ctx.encrypt(keyring.L, ring.L, pk.ptr, out.ptr, n, msg=None if msg is None else msg.ptr, sigma_u=params.sigma, sigma_e=params.sigma,
                    mult_e=mult, seed=rng.seed, stream=1, first_poly=rng.take(3 * n))
    else:
        draws = [sample_normal_ints(rng, N, params.sigma, batch).reshape(n, N) for _ in range(3)]   # u, e1, e2 in today's order
        ints = np.stack(draws, axis=1)
        if np.abs(ints).max(initial=0) >= 2**31:
            raise AssertionError("encrypt: a noise draw does not fit 32 bits")
        rand = DeviceBuffer.from_numpy(np.ascontiguousarray(ints.astype(np.int32)).reshape(-1).view(np.uint64))
        ctx.encrypt(keyring.L, ring.L, pk.ptr, out.ptr, n, msg=None if msg is None else msg.ptr, rand=rand.ptr, mult_e=mult)
    # an ordinary ciphertext, as before: split into its components (one strided copy each), no packed image kept -- a fresh
    # ciphertext is read component by component (serialisation, c + plain) at least as often as it goes to a key switch
    return CipherText(params, _unpack(out, ring, n, 2, batch, primal=True, ctx=ctx), scale)


def encrypt_zero(rng, pub: PubKey, batch=None) -> CipherText:
    c = _encrypt_device(rng, pub, batch, None, None)
    if c is not None:
        return c
    return _encrypt_zero_composed(rng, pub, batch)


def _encrypt_zero_composed(rng, pub: PubKey, batch=None) -> CipherText:
    params = pub.params
    ring = params.R_key()
    u = params.secret_dist(rng, ring, batch)
    e1, e2 = params.noise(rng, ring, batch), params.noise(rng, ring, batch)
    mask, masked = pub.key.mask, pub.key.masked
    if batch is not None:  # broadcast the key over the batch
        mask, masked = _broadcast(mask, batch), _broadcast(masked, batch)
    c1 = masked * u + e1
    c2 = mask * u + e2
    cs = (c1, c2)
    if isinstance(params, ModulusRaised):  # modulusraising.jl:23-26: drop the special limb
        cs = tuple(c.modswitch_drop() for c in cs)
    if isinstance(params, GroupedRaised):  # the same for every special limb
        for _ in range(params.n_special):
            cs = tuple(c.modswitch_drop() for c in cs)
    return CipherText(params, cs)


def _broadcast(el: RingElement, batch: int) -> RingElement:
    el.coeffs_dual()                                       # keys are used as multiplicands: broadcast the NTT form
    return RingElement(el.ring, None, el.dual, None).broadcast_to(batch)


def encrypt(rng, key, plaintext, scale=None) -> CipherText:
    pub = key.pub if isinstance(key, KeyPair) else key
    enc = pub.params.encode(plaintext)
    c = _encrypt_device(rng, pub, enc.batch, enc, scale) if isinstance(enc, RingElement) else None
    if c is not None:
        return c
    c = _encrypt_zero_composed(rng, pub, enc.batch)
    c = c + enc  # rlwe_she.jl:190
    c.scale = scale
    return c


def _decryption_device(secret: RingElement, c: CipherText):
    """b = c_1 + s c_2 (+ s^2 c_3) as ONE device call (tfhe_decrypt_phase), or None when this ciphertext is not covered"""
    P = len(c)
    if not _FUSED_ENCRYPT or P not in (2, 3) or secret.batch is not None:
        return None
    ring, keyring = c.ring(), secret.ring
    if not _is_prefix(keyring) or ring.ctx is not keyring.ctx or not _is_prefix(ring) or ring.L > keyring.L:
        return None
    if not 1 << 12 <= ring.N <= 1 << 14:
        # outside the fused sizes the call's composed form measured SLOWER than the composition below (N = 2^16, reference ring:
        # 0.61-0.72 x through the mirror, 0.79-0.95 x as a raw call; profiles/LOG.md): the composition stays
        return None
    n, batch = c._shape()
    # decryption asks for the components, as before (an unsplit key-switch result is split here and keeps its packed image,
    # which is then the call's operand: no second copy)
    ntt_in = all(x.primal is None and x.dual is not None for x in c.cs)
    bufs = [x.coeffs_dual() if ntt_in else x.coeffs_primal() for x in c.cs]
    image = (None if ntt_in else c._packed_for(bufs, ring.ctx)) or _pack(bufs, ring, n)
    out = DeviceBuffer(n * ring.L * ring.N)
    ring.ctx.decrypt_phase(keyring.L, ring.L, secret.coeffs_dual().ptr, image.ptr, P, out.ptr, n, ntt_in=ntt_in)
    return RingElement(ring, out, None, batch)


def _decryption(key, c: CipherText):
    priv = key.priv if isinstance(key, KeyPair) else key
    b = _decryption_device(priv.secret, c)
    if b is not None:
        return priv, b
    secret = priv.secret
    while secret.ring.L != c[0].ring.L:  # rlwe_she.jl:202-204
        secret = secret.modswitch_drop()
    if c[0].batch is not None:
        secret = _broadcast(secret, c[0].batch)
    b, spow = c[0], secret
    for i in range(1, len(c)):
        b = b + spow * c[i]
        if i + 1 < len(c):
            spow = spow * secret
    return priv, b


def decrypt(key, c: CipherText):
    priv, b = _decryption(key, c)
    return priv.params.decode(b)


def decrypt_array(key, c: CipherText) -> np.ndarray:
    """decrypt(key, c) as a uint64 numpy array [N] (one ciphertext) or [batch][N] -- the same values; BFV / BGV only.  The
    plaintext codec runs on the device (tfhe_plain_decode) where decrypt's does."""
    priv, b = _decryption(key, c)
    dec = getattr(priv.params, "decode_array", None)
    if dec is None:
        raise NotImplementedError("decrypt_array: BFV / BGV parameters")
    return dec(b)


def invariant_noise_budget(key, c: CipherText):
    """invariant_noise_budget(pk::PrivKey{BFVParams}, c), bfv.jl:137-166:
    log2(q) - log2(t) - 1 - max_i log2(birem(b_i)) with b = c_1 + s c_2 + s^2 c_3 ... and birem(x) = min(x mod Δ, Δ - x mod Δ).
    One ciphertext -> a float; a batch -> a list of floats, one per ciphertext (the same formula).  The maximum of birem runs
    on the device (tfhe_bfv_noise_max) when b lives on params.ring's moduli, else on the host."""
    priv = key.priv if isinstance(key, KeyPair) else key
    params = priv.params
    if not isinstance(params, BFVParams):
        raise NotImplementedError("invariant_noise_budget: BFV ciphertexts")
    _, b = _decryption(priv, c)                            # (the secret and the ciphertext share params.ring: nothing is dropped)
    delta = params.delta
    plan = _plain_plan(params, b.ring) if params._device_ring(b) else None
    if plan is not None:
        n, nw = b.count, plan.delta_words
        out = DeviceBuffer(n * nw)
        plan.noise_max(b.coeffs_primal().ptr, out.ptr, n)
        b.ring.ctx.sync()
        words = out.to_numpy((n, nw))
        worsts = [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in words]
    else:
        def birem(x):
            r = x % delta
            return delta - r if r > delta // 2 else r
        ints = b.to_ints()
        worsts = [max(birem(x) for x in row) for row in (ints if b.batch is not None else [ints])]

    def budget(worst):
        return math.log2(params.ring.modulus()) - math.log2(params.t) - 1 - (math.log2(worst) if worst else 0.0)
    out_b = [budget(w) for w in worsts]
    return out_b if c[0].batch is not None else out_b[0]


def slot_encode(plain_ring: NegacyclicRing, slots) -> RingElement:
    """SlotEncoding -> RingElement (encoding.jl:35-52): the slots ARE the NTT-domain (dual) coefficients, natural order."""
    vals = [int(v) % plain_ring.moduli[0] for v in slots]
    res = np.array([vals], dtype=np.uint64)
    return RingElement.from_host(plain_ring, res, dual=True)


def slot_decode(el: RingElement):
    """SlotEncoding(r) (encoding.jl:35-43): coeffs_dual of a plaintext ring element."""
    return [int(v) for v in el.to_numpy("dual")[0]]


# --------------------------------------------------------------------------------------------------
# multiplication (rlwe_she.jl:247-266 + bfv.jl:34-40)
# --------------------------------------------------------------------------------------------------


def enc_mul(c1: CipherText, c2: CipherText):
    if c1.params is not c2.params:
        raise UsageError("Attempting to multiply ciphertexts with differing parameters")
    params = c1.params
    ring, batch = c1[0].ring, c1[0].batch
    n = c1[0].count
    sz = ring.L * ring.N
    if isinstance(params, BFVParams):
        if len(c1) != 2 or len(c2) != 2:
            # any component counts (rlwe_she.jl:247-262 as written: e.g. (c*c)*c without relinearisation): mul_expand per
            # component (bfv.jl:34), the convolution over ℛbig, mul_contract per output component (bfv.jl:35-40).  The
            # conversions order ℛ's and ℛbig's streams themselves (tfhe_bfv_expand / tfhe_bfv_contract).
            e1, e2 = [params.mul_expand(c) for c in c1.cs], [params.mul_expand(c) for c in c2.cs]
            cs = [None] * (len(e1) + len(e2) - 1)
            for i, x in enumerate(e1):
                for j, y in enumerate(e2):
                    p = x * y
                    cs[i + j] = p if cs[i + j] is None else cs[i + j] + p
            return tuple(params.mul_contract(c) for c in cs)
        a, b = _pack([c.coeffs_primal() for c in c1.cs], ring, n), _pack([c.coeffs_primal() for c in c2.cs], ring, n)
        out = DeviceBuffer(n * 3 * sz)
        params.plan().mul(a.ptr, b.ptr, out.ptr, n)
        return _unpack(out, ring, n, 3, batch, primal=True)
    if len(c1) == 2 and len(c2) == 2:  # mul_expand / mul_contract are the identity (rlwe_she.jl:39-40)
        a, b = _pack([c.coeffs_dual() for c in c1.cs], ring, n), _pack([c.coeffs_dual() for c in c2.cs], ring, n)
        out = DeviceBuffer(n * 3 * sz)
        ring.ctx.tensor(a.ptr, b.ptr, out.ptr, n, ring.L, ring.idx)
        return _unpack(out, ring, n, 3, batch, primal=False)
    cs = [None] * (len(c1) + len(c2) - 1)  # generic convolution of components
    for i in range(len(c1)):
        for j in range(len(c2)):
            p = c1[i] * c2[j]
            cs[i + j] = p if cs[i + j] is None else cs[i + j] + p
    return tuple(cs)


def _pack(bufs, ring, n, ctx=None) -> DeviceBuffer:
    """[poly](n, L, N) -> (n, polys, L, N): one strided device copy per component, on the stream of `ctx` (the context that
    will consume the packed batch)."""
    ctx = ctx or ring.ctx
    P, sz = len(bufs), ring.L * ring.N
    out = DeviceBuffer(n * P * sz)
    lib = native.lib()
    for p, b in enumerate(bufs):
        native.check(lib.tfhe_pack_poly(ctx.h, out.ptr, b.ptr, P, p, sz, n))
    return out


def _unpack(buf, ring, n, P, batch, primal=True, ctx=None):
    """(n, P, L, N) -> P ring elements of shape (n, L, N), on the stream of `ctx` (the context that produced `buf`)."""
    ctx = ctx or ring.ctx
    sz = ring.L * ring.N
    lib = native.lib()
    outs = []
    for p in range(P):
        o = DeviceBuffer(n * sz)
        native.check(lib.tfhe_unpack_poly(ctx.h, o.ptr, buf.ptr, P, p, sz, n))
        outs.append(RingElement(ring, o, None, batch) if primal else RingElement(ring, None, o, batch))
    # no host wait: `buf` may be released by the caller as soon as we return -- the allocator parks a released block until
    # the work submitted so far on every context stream has finished (tfhe_free, dev_alloc.h)
    return tuple(outs)


# --------------------------------------------------------------------------------------------------
# key switching (rlwe_she.jl:273-360, modulusraising.jl:28-49)
# --------------------------------------------------------------------------------------------------


# TFHE_FUSED_KEYGEN=0: keys as the reference's term-by-term expressions on ring elements (comparisons; kept as the _composed
# functions); the default is one device call (tfhe_evalkey_gen) -- the same residues, the same generator state afterwards.
_FUSED_KEYGEN = os.environ.get("TFHE_FUSED_KEYGEN", "1") != "0"
# The largest log2 N at which the mirror takes the call.  Above 2^14 the call runs its composed form (fill -> transform -> finish),
# which has NOT been timed against the composition yet (tools/bench_keygen.py, profiles/LOG.md); the last call of this shape,
# tfhe_decrypt_phase, measured slower than its composition at N = 2^16 (_decryption_device).  Until it is timed the composition
# stays there; TFHE_FUSED_KEYGEN_MAX_LOG2=17 routes every size through the call.
_FUSED_KEYGEN_MAX_LOG2 = int(os.environ.get("TFHE_FUSED_KEYGEN_MAX_LOG2", "14"))


def _keygen_device_ok(rng, params, ring: NegacyclicRing, secret: RingElement | None = None) -> bool:
    """the draws come from the stock samplers (uniform mask, rounded Gaussian noise) and the key ring is a prefix of its context"""
    if not _FUSED_KEYGEN or _noise_multiplier(params) is None or not isinstance(rng, (DeviceRng, np.random.Generator)):
        return False
    if not _is_prefix(ring) or ring.N > 1 << _FUSED_KEYGEN_MAX_LOG2:
        return False
    return secret is None or (secret.batch is None and secret.ring.ctx is ring.ctx and secret.ring.idx == ring.idx)


def _gadget_table(params, ring: NegacyclicRing):
    """gamma[i][j]: the residue mod q_j that multiplies `old` in digit i of make_eval_key (rlwe_she.jl:281-287); ModulusRaised
    pre-multiplies by the special prime P (modulusraising.jl:28-32), whose own row and column are therefore zero"""
    mods = list(ring.moduli)
    if isinstance(params, GroupedRaised):                 # row g: P at the limbs of group g of the key's own top level, zero elsewhere
        top = ring.L - params.n_special
        P = math.prod(mods[top:])
        return [[(P % q if j in G else 0) for j, q in enumerate(mods)] for G in params.digit_groups(top)]
    P = mods[-1] if isinstance(params, ModulusRaised) else 1
    if params.relin_window != 0:                          # base-2^w gadget: 2^(i w) mod Q, Q the key ring's modulus
        w, Q = params.relin_window, ring.modulus()
        nwin = -(-Q.bit_length() // w)                    # ndigits(Q, base = 2^w)
        return [[(P % q) * (pow(2, i * w, Q) % q) % q for q in mods] for i in range(nwin)]
    return [[(P % q if i == j else 0) for j, q in enumerate(mods)] for i in range(ring.L)]   # CRTResidual, crt.jl:64-77


def _host_draws(rng: np.random.Generator, ring: NegacyclicRing, sigma: float, n: int, between=None):
    """n (mask, noise) pairs in the order the composition draws them -- per pair the limbs' `integers`, then `normal` -- as device
    buffers: uint64 [n][L][N] and int32 [n][N].  `between()` runs after the mask of the first pair (keygen draws the secret there)."""
    L, N = ring.L, ring.N
    mask, noise = np.empty((n, L, N), dtype=np.uint64), np.empty((n, N), dtype=np.int64)
    for i in range(n):
        for l, q in enumerate(ring.moduli):
            mask[i, l] = rng.integers(0, q, size=(N,), dtype=np.uint64)
        if i == 0 and between is not None:
            between()
        noise[i] = sample_normal_ints(rng, N, sigma)
    if np.abs(noise).max(initial=0) >= 2**31:
        raise AssertionError("keygen: a noise draw does not fit 32 bits")
    return (DeviceBuffer.from_numpy(mask),
            DeviceBuffer.from_numpy(np.ascontiguousarray(noise.astype(np.int32)).reshape(-1).view(np.uint64)))


def _key_from_buffer(params, ring: NegacyclicRing, buf: DeviceBuffer, n_digits: int) -> KeySwitchKey:
    """the KeySwitchKey over the packed buffer tfhe_evalkey_gen wrote: its components are dual-domain views into it"""
    sz = ring.L * ring.N
    ksk = KeySwitchKey(params, [KeyComponent(RingElement(ring, None, _KeyView(buf, (2 * i) * sz, sz)),
                                             RingElement(ring, None, _KeyView(buf, (2 * i + 1) * sz, sz))) for i in range(n_digits)])
    ksk._packed = buf
    return ksk


def _keygen_device(rng, params, ring: NegacyclicRing) -> KeyPair:
    ctx, sz = ring.ctx, ring.L * ring.N
    buf = DeviceBuffer(2 * sz)
    mult = _noise_multiplier(params)
    if isinstance(rng, DeviceRng):
        first = rng.take(1)                               # the mask; the secret takes first + 1, the error first + 2
        secret = params.secret_dist(rng, ring)
        ctx.evalkey_gen(ring.L, secret.coeffs_dual().ptr, [buf.ptr], 1, sigma_e=params.sigma, mult_e=mult, seed=rng.seed,
                        stream_mask=0, stream_noise=1, mask_poly=first, noise_poly=rng.take(1), poly_stride=1)
    else:
        drawn = []
        mask, noise = _host_draws(rng, ring, params.sigma, 1, between=lambda: drawn.append(params.secret_dist(rng, ring)))
        secret = drawn[0]
        ctx.evalkey_gen(ring.L, secret.coeffs_dual().ptr, [buf.ptr], 1, mask_rand=mask.ptr, noise_rand=noise.ptr, mult_e=mult)
    pub = PubKey(params, KeyComponent(RingElement(ring, None, _KeyView(buf, 0, sz)), RingElement(ring, None, _KeyView(buf, sz, sz))))
    pub._packed = buf                                     # what tfhe_encrypt takes (_packed_pubkey)
    return KeyPair(PrivKey(params, secret), pub)


def _evalkeys_device(rng, params, ring: NegacyclicRing, secret: RingElement, n_keys: int, old=None, galois=None):
    """n_keys key-switching keys in one tfhe_evalkey_gen call (a numpy generator: one call per key, a key's draws being what is
    staged on the host at a time).  old: a device buffer [1][L][N] (NTT domain; n_keys == 1), else galois[k]: 0 / g."""
    ctx, L, sz = ring.ctx, ring.L, ring.L * ring.N
    gadget = _gadget_table(params, ring)
    nd, mult = len(gadget), _noise_multiplier(params)
    s = secret.coeffs_dual()
    bufs = [DeviceBuffer(nd * 2 * sz) for _ in range(n_keys)]
    if isinstance(rng, DeviceRng):
        first = rng.take(2 * n_keys * nd)                 # per component: the mask's counter, then the noise's
        ctx.evalkey_gen(L, s.ptr, [b.ptr for b in bufs], nd, gadget=gadget, old=None if old is None else old.ptr, galois_elements=galois,
                        sigma_e=params.sigma, mult_e=mult, seed=rng.seed, stream_mask=0, stream_noise=1, mask_poly=first,
                        noise_poly=first + 1, poly_stride=2)
    else:
        for k, b in enumerate(bufs):
            mask, noise = _host_draws(rng, ring, params.sigma, nd)
            ctx.evalkey_gen(L, s.ptr, [b.ptr], nd, gadget=gadget, old=None if old is None else old.ptr,
                            galois_elements=None if galois is None else [galois[k]], mask_rand=mask.ptr, noise_rand=noise.ptr, mult_e=mult)
    return [_key_from_buffer(params, ring, b, nd) for b in bufs]


def make_eval_key(rng, old: RingElement, new: PrivKey) -> KeySwitchKey:
    """make_eval_key(rng, old => new), rlwe_she.jl:273-298 with the RNS gadget (:287) or base-2^w digits (:281-283); ModulusRaised
    pre-multiplies ``old`` by the special prime (modulusraising.jl:28-32).  One device call (tfhe_evalkey_gen) when the draws
    come from the stock samplers."""
    ring = old.ring
    if _keygen_device_ok(rng, new.params, ring, new.secret) and old.batch is None:
        return _evalkeys_device(rng, new.params, ring, new.secret, 1, old=old.coeffs_dual())[0]
    return _make_eval_key_composed(rng, old, new)


def _make_eval_key_composed(rng, old: RingElement, new: PrivKey) -> KeySwitchKey:
    """the composition on ring elements: the gadget built on the host, per digit two draws, a product, a sum and a difference"""
    params = new.params
    ring = old.ring
    if isinstance(params, ModulusRaised):
        old = old * ring.moduli[-1]                       # P * old over the key ring Q P; the gadget below is the parent's
    key = []
    if isinstance(params, GroupedRaised):
        top = ring.L - params.n_special
        res = (old * math.prod(ring.moduli[top:])).to_numpy("primal")
        gadget = []
        for G in params.digit_groups(top):
            g = np.zeros_like(res)
            g[list(G)] = res[list(G)]
            gadget.append(RingElement.from_host(ring, g))
    elif params.relin_window != 0:                          # base-2^w gadget, rlwe_she.jl:281-283
        w = params.relin_window
        nwin = -(-ring.modulus().bit_length() // w)       # ndigits(Q, base = 2^w)
        gadget = [old * pow(2, i * w, ring.modulus()) for i in range(nwin)]
    else:
        res = old.to_numpy("primal")
        gadget = []
        for i in range(ring.L):
            g = np.zeros_like(res)
            g[i] = res[i]                                 # CRTResidual, crt.jl:64-77
            gadget.append(RingElement.from_host(ring, g))
    for g in gadget:
        mask = sample_uniform(rng, ring)
        e = params.noise(rng, ring)
        key.append(KeyComponent(mask, g - (mask * new.secret + e)))
    return KeySwitchKey(params, key)


def keygen_evalmult(rng, priv: PrivKey) -> EvalMultKey:
    ring = priv.secret.ring
    if _keygen_device_ok(rng, priv.params, ring, priv.secret):     # s^2 is formed inside the call
        return EvalMultKey(_evalkeys_device(rng, priv.params, ring, priv.secret, 1, galois=[0])[0])
    return _keygen_evalmult_composed(rng, priv)


def _keygen_evalmult_composed(rng, priv: PrivKey) -> EvalMultKey:
    return EvalMultKey(_make_eval_key_composed(rng, priv.secret * priv.secret, priv))  # rlwe_she.jl:299


def galois_element_for_steps(steps: int, N: int) -> int:
    return pow(3, 2 * N - steps, 2 * N) if steps > 0 else pow(3, -steps, 2 * N)  # rlwe_she.jl:304


def keygen_galois(rng, priv: PrivKey, galois_element=None, steps=None) -> GaloisKey:
    assert (galois_element is None) != (steps is None)  # rlwe_she.jl:301
    if galois_element is None:
        galois_element = galois_element_for_steps(steps, priv.secret.ring.N)
    return keygen_galois_many(rng, priv, galois_elements=[galois_element])[0]


def _keygen_galois_composed(rng, priv: PrivKey, galois_element=None, steps=None) -> GaloisKey:
    assert (galois_element is None) != (steps is None)  # rlwe_she.jl:301
    if galois_element is None:
        galois_element = galois_element_for_steps(steps, priv.secret.ring.N)
    return GaloisKey(galois_element, _make_eval_key_composed(rng, priv.secret.apply_galois_element(galois_element), priv))


def keygen_galois_many(rng, priv: PrivKey, galois_elements=None, steps=None) -> "list[GaloisKey]":
    """[keygen_galois(rng, priv, g) for g in galois_elements] (or one key per entry of `steps`), word for word and with the same
    generator state afterwards -- all keys in ONE device call (tfhe_evalkey_gen) when the draws come from a DeviceRng: the secret
    under x -> x^g is read through an index permutation inside the call, never formed.  With a numpy generator the draws are made
    on the host: one call and one upload PER KEY (a key's draws, n_digits (L + 1) rows, are what is staged at a time; 63 keys of
    the MNIST ring at once would be 6.5 GB)."""
    assert (galois_elements is None) != (steps is None)
    ring = priv.secret.ring
    gs = [int(g) for g in galois_elements] if steps is None else [galois_element_for_steps(int(st), ring.N) for st in steps]
    if not gs:
        return []
    if _keygen_device_ok(rng, priv.params, ring, priv.secret) and all(g % 2 == 1 and 0 < g < 2 * ring.N for g in gs):
        return [GaloisKey(g, k) for g, k in zip(gs, _evalkeys_device(rng, priv.params, ring, priv.secret, len(gs), galois=gs))]
    return [_keygen_galois_composed(rng, priv, galois_element=g) for g in gs]


def keyswitch(ek, c: CipherText, _galois=None, _gk=None) -> CipherText:
    """keyswitch(ek, c), rlwe_she.jl:315-349 -- one fused device call."""
    if isinstance(ek, (EvalMultKey, GaloisKey)):
        ek = ek.key
    if len(c) not in (2, 3):
        raise AssertionError("keyswitch needs a 2- or 3-element ciphertext")  # rlwe_she.jl:318
    params = ek.params
    keyring = ek.key[0].mask.ring
    if params.relin_window != 0:                          # base-2^w digits, rlwe_she.jl:330-338
        special = isinstance(params, ModulusRaised)       # digits of c[end] over Q_level, keys over [q_0..q_{l-1}, P] (modulusraising.jl:35-49)
        ring, n, batch = c[0].ring, c[0].count, c[0].batch
        level = ring.L
        if keyring.idx != list(range(keyring.L)) or ring.idx != list(range(level)) or level > keyring.L - (1 if special else 0):
            raise UsageError("window key switch: the ciphertext ring must be a prefix of the key ring")
        cs = c.cs if _galois is None else [x.apply_galois_element(_galois) for x in c.cs]
        prim = [x.coeffs_primal() for x in cs]            # may enqueue inverse transforms on the ciphertext ring's stream: BEFORE the hand-over
        if ring.ctx is not keyring.ctx:
            if ring.N != keyring.N or ring.moduli != keyring.moduli[:level] or ring.psi != keyring.psi[:level]:
                raise UsageError("ciphertext and key belong to different rings")
            keyring.ctx.wait_for(ring.ctx)
        ct = _pack(prim, ring, n, ctx=keyring.ctx)
        out = DeviceBuffer(n * 2 * level * ring.N)
        keyring.ctx.keyswitch_window(level, params.relin_window, ek.packed().ptr, len(ek.key), ct.ptr, len(c), out.ptr, n,
                                     key_limbs=keyring.L, special=special)
        res = _unpack(out, ring, n, 2, batch, primal=True, ctx=keyring.ctx)
        if ring.ctx is not keyring.ctx:
            ring.ctx.wait_for(keyring.ctx)
        return CipherText(c.params, res, c.scale)
    special = isinstance(params, ModulusRaised)
    grouped = isinstance(params, GroupedRaised)
    ring = c.ring()
    n, batch = c._shape()
    level = ring.L
    if keyring.idx != list(range(keyring.L)) or ring.idx != list(range(level)):
        raise UsageError("ciphertext ring is not a prefix of the key ring")
    if ring.ctx is not keyring.ctx and (ring.N != keyring.N or ring.moduli != keyring.moduli[:level] or ring.psi != keyring.psi[:level]):
        raise UsageError("ciphertext and key belong to different rings")
    sz = level * ring.N
    ct = c._deferred_image(keyring.ctx) if isinstance(c, _PackedResult) else None   # an unsplit result of this very context: in stream order already
    if ct is None:
        prim = [x.coeffs_primal() for x in c.cs]           # may enqueue inverse transforms on the ciphertext ring's stream ...
        if ring.ctx is not keyring.ctx:
            keyring.ctx.wait_for(ring.ctx)                 # ... so the hand-over to the key ring's stream comes after them
        ct = c._packed_for(prim, keyring.ctx, consume=True) or _pack(prim, ring, n, ctx=keyring.ctx)
    out = DeviceBuffer(n * 2 * sz)
    if grouped:
        if _galois is None:
            keyring.ctx.keyswitch_grouped(keyring.L, level, params.n_special, params.group, ek.packed().ptr, len(ek.key), ct.ptr, len(c), out.ptr, n)
        else:
            keyring.ctx.rotate_grouped(keyring.L, level, params.n_special, params.group, ek.packed().ptr, len(ek.key), _galois, ct.ptr, out.ptr, n)
    elif _galois is None:
        keyring.ctx.keyswitch(keyring.L, level, special, ek.packed().ptr, len(ek.key), ct.ptr, len(c), out.ptr, n)
    elif _gk is not None and ring.N >= (1 << 15) and n >= 8:
        # N >= 2^15, 8 ciphertexts or more: the rotation is finished in the key switch's tail on the key as
        # tfhe_galois_key_prepare leaves it -- prepared once per key (GaloisKey.prepared), not once per call (r06:
        # infer.jl:140-149 rotates by ONE key 63 times per matrix product)
        keyring.ctx.rotate(keyring.L, level, special, _gk.prepared().ptr, len(ek.key), _galois, ct.ptr, out.ptr, n, prepared=True)
    else:
        keyring.ctx.rotate(keyring.L, level, special, ek.packed().ptr, len(ek.key), _galois, ct.ptr, out.ptr, n)
    if not _LAZY_UNPACK:
        cs = _unpack(out, ring, n, 2, batch, primal=True, ctx=keyring.ctx)
        if ring.ctx is not keyring.ctx:
            ring.ctx.wait_for(keyring.ctx)                 # the results are elements of `ring`: its stream must see them written
        return CipherText(c.params, cs, c.scale)._remember_packed(out, keyring.ctx)
    if ring.ctx is not keyring.ctx:
        ring.ctx.wait_for(keyring.ctx)                     # the result belongs to `ring`: its stream must see it written
    return _PackedResult(c.params, c.scale, out, keyring.ctx, ring, n, batch)


def mul_relin(ek, c1: CipherText, c2: CipherText, rescale: bool = False) -> CipherText:
    """modswitch(keyswitch(ek, c1 * c2)) (rescale=True) or keyswitch(ek, c1 * c2) of CKKS / BGV ciphertexts -- the square layers of
    infer.jl:135-137, :165-167 -- in ONE device call (tfhe_mul_relin) on the packed operands: same components, same scale
    (scale_1 scale_2 [/ q_last], ckksencoding.jl:127-135).  An unsplit key-switch result is taken as it is; otherwise one pack
    per operand (`c1 is c2` squares from one).  The result stays packed until its components are asked for, as keyswitch's.
    BFV multiplies through its plan (BFVParams.plan().mul_relin); windowed keys (relin_window != 0) take the composed path."""
    if isinstance(ek, (EvalMultKey, GaloisKey)):
        ek = ek.key
    if c1.params is not c2.params:
        raise UsageError("Attempting to multiply ciphertexts with differing parameters")
    _refuse_grouped(ek.params, "mul_relin")
    return _mul_relin_packed(ek, c1, c2, rescale)


def mul_relin_grouped(ek, c1: CipherText, c2: CipherText, rescale: bool = False) -> CipherText:
    """mul_relin on a key with grouped digits (GroupedRaised; tfhe_mul_relin_grouped): modswitch(keyswitch(ek, c1 * c2)) (rescale=True)
    or keyswitch(ek, c1 * c2), word for word, in ONE device call on the packed operands -- with a special prime the rescale rides on
    the key switch's tail.  Usage checks, operand handling, scales and the packed result are mul_relin's."""
    if isinstance(ek, (EvalMultKey, GaloisKey)):
        ek = ek.key
    if c1.params is not c2.params:
        raise UsageError("Attempting to multiply ciphertexts with differing parameters")
    if not isinstance(ek.params, GroupedRaised):
        raise UsageError("mul_relin_grouped takes a key with grouped digits (GroupedRaised); the others go through mul_relin")
    return _mul_relin_packed(ek, c1, c2, rescale)


def _mul_relin_packed(ek, c1: CipherText, c2: CipherText, rescale: bool) -> CipherText:
    """what mul_relin and mul_relin_grouped share, after the checks of the key's kind: `ek` a KeySwitchKey"""
    inner = c1.params.params if isinstance(c1.params, (ModulusRaised, GroupedRaised)) else c1.params
    if isinstance(inner, BFVParams):
        raise UsageError("mul_relin serves the schemes without mul_expand / mul_contract (CKKS, BGV); "
                         "BFV multiplies and relinearises through its plan: BFVParams.plan().mul_relin")
    if (c1.scale is None) != (c2.scale is None):
        raise UsageError("multiplying a scaled (CKKS) ciphertext by an unscaled one")
    params = ek.params
    if params.relin_window != 0 or len(c1) != 2 or len(c2) != 2:
        r = keyswitch(ek, c1 * c2)
        return modswitch(r) if rescale else r
    special = isinstance(params, ModulusRaised)
    keyring = ek.key[0].mask.ring
    ring = c1.ring()
    n, batch = c1._shape()
    level = ring.L
    if c2.ring() is not ring and (c2.ring().ctx is not ring.ctx or c2.ring().idx != ring.idx):
        raise UsageError("the factors live in different rings")
    if c2._shape() != (n, batch):
        raise UsageError("the factors have different batch shapes")
    if rescale and level < 2:
        raise UsageError("modswitch needs at least two CRT moduli")
    if keyring.idx != list(range(keyring.L)) or ring.idx != list(range(level)):
        raise UsageError("ciphertext ring is not a prefix of the key ring")
    if ring.ctx is not keyring.ctx and (ring.N != keyring.N or ring.moduli != keyring.moduli[:level] or ring.psi != keyring.psi[:level]):
        raise UsageError("ciphertext and key belong to different rings")
    factors = [c1] if c1 is c2 else [c1, c2]
    images = [c._deferred_image(keyring.ctx) if isinstance(c, _PackedResult) else None for c in factors]
    # operands that exist only as NTT images go in as they are (ntt_in): no inverse transforms just to transform them back
    ntt_in = all(im is None for im in images) and all(x.primal is None and x.dual is not None for c in factors for x in c.cs)
    bufs = [None if im is not None else [x.coeffs_dual() if ntt_in else x.coeffs_primal() for x in c.cs] for c, im in zip(factors, images)]
    if ring.ctx is not keyring.ctx:
        keyring.ctx.wait_for(ring.ctx)                     # the transforms above ran on the ciphertext ring's stream
    for i, c in enumerate(factors):
        if images[i] is None:
            images[i] = (None if ntt_in else c._packed_for(bufs[i], keyring.ctx, consume=True)) or _pack(bufs[i], ring, n, ctx=keyring.ctx)
    a, b = images[0], images[-1]
    ring_out = ring.drop_last() if rescale else ring
    out = DeviceBuffer(n * 2 * ring_out.L * ring.N)
    if isinstance(params, GroupedRaised):
        keyring.ctx.mul_relin_grouped(keyring.L, level, params.n_special, params.group, ek.packed().ptr, len(ek.key), a.ptr, b.ptr, out.ptr, n,
                                      ntt_in=ntt_in, rescale=rescale)
    else:
        keyring.ctx.mul_relin(keyring.L, level, special, ek.packed().ptr, len(ek.key), a.ptr, b.ptr, out.ptr, n, ntt_in=ntt_in, rescale=rescale)
    scale = None if c1.scale is None else c1.scale * c2.scale   # ckksencoding.jl:133-135
    if rescale and scale is not None:
        scale = scale / ring.moduli[-1]                     # ckksencoding.jl:127-130
    if ring.ctx is not keyring.ctx:
        ring.ctx.wait_for(keyring.ctx)                     # the result belongs to the ciphertext ring: its stream must see it written
    res = _PackedResult(c1.params, scale, out, keyring.ctx, ring_out, n, batch)
    if not _LAZY_UNPACK:
        res.cs                                             # split now (the image is remembered, as keyswitch does)
    return res


def apply_galois_element(c: CipherText, g: int) -> CipherText:
    return CipherText(c.params, [x.apply_galois_element(g) for x in c.cs], c.scale)  # rlwe_she.jl:355-357


def rotate(gk: GaloisKey, c: CipherText) -> CipherText:
    """rotate(gk, c) = keyswitch(gk, apply_galois_element(c, g)), rlwe_she.jl:359 (fused on the device)."""
    if len(c) != 2:
        raise AssertionError("rotate takes a 2-element ciphertext")
    return keyswitch(gk.key, c, _galois=gk.galois_element, _gk=gk)


def rotate_many(gks, c: CipherText):
    """[rotate(gk, c) for gk in gks] from one digit decomposition of c (tfhe_rotate_many: the forward transforms of the RNS
    digits are shared by all rotations); each result is bit-identical to `rotate(gk, c)`.  RNS-digit keys (relin_window = 0)."""
    gks = list(gks)
    _refuse_grouped_keys(gks, "rotate_many")
    if len(c) != 2:
        raise AssertionError("rotate takes a 2-element ciphertext")
    if not gks:
        return []
    params = gks[0].key.params
    if any(g.key.params is not params for g in gks) or params.relin_window != 0:
        raise UsageError("hoisted rotations need Galois keys of one parameter set with RNS digits")
    keyring = gks[0].key.key[0].mask.ring
    ring, n, batch = c[0].ring, c[0].count, c[0].batch
    level, special = ring.L, isinstance(params, ModulusRaised)
    if keyring.idx != list(range(keyring.L)) or ring.idx != list(range(level)):
        raise UsageError("ciphertext ring is not a prefix of the key ring")
    prim = [x.coeffs_primal() for x in c.cs]               # before the hand-over (see keyswitch)
    if ring.ctx is not keyring.ctx:
        if ring.N != keyring.N or ring.moduli != keyring.moduli[:level] or ring.psi != keyring.psi[:level]:
            raise UsageError("ciphertext and key belong to different rings")
        keyring.ctx.wait_for(ring.ctx)
    sz = level * ring.N
    ct = _pack(prim, ring, n, ctx=keyring.ctx)
    out = DeviceBuffer(len(gks) * n * 2 * sz)
    keyring.ctx.rotate_many(keyring.L, level, special, [g.prepared().ptr for g in gks], len(gks[0].key.key),
                            [g.galois_element for g in gks], ct.ptr, out.ptr, n, prepared=True)
    res = []
    for r in range(len(gks)):
        view = _View(out, r * n * 2 * sz)
        res.append(CipherText(c.params, _unpack(view, ring, n, 2, batch, primal=True, ctx=keyring.ctx), c.scale))
    if ring.ctx is not keyring.ctx:
        ring.ctx.wait_for(keyring.ctx)                     # as in keyswitch: the results live on `ring`, written on the key ring's stream
    return res


def matmul_diag(gks, diags, c: CipherText) -> CipherText:
    """diags[0] .* c + sum_k diags[k] .* rotate(gks[k-1], c): the diagonal matrix-vector product of infer.jl:140-149 /
    test/ckks_matmul.jl:33-41 with every rotation starting from `c` (one Galois key per step), in ONE device call
    (tfhe_matmul_diag).  `diags`: len(gks) + 1 plaintext ring elements of c's ring encoded at c's scale (one polynomial each:
    the same diagonal multiplies every ciphertext of the batch), or ONE batched element holding them back to back (what
    ckks_encode returns for a [len(gks) + 1][N/2] array of slot vectors).  Bit-identical to
    `CipherText.dot_plain([c] + rotate_many(gks, c), diags)`; the result is in the NTT domain, at the squared scale."""
    gks = list(gks)
    _refuse_grouped_keys(gks, "matmul_diag")
    if len(c) != 2:
        raise AssertionError("rotate takes a 2-element ciphertext")
    c._need_scale()
    ring, n, batch = c[0].ring, c[0].count, c[0].batch
    level = ring.L
    if len(gks) > DOT_MAX:          # a device call takes DOT_MAX rotations: more of them as partial products (+ is exact); the
        dl = diags.split([1] * diags.count) if isinstance(diags, RingElement) else list(diags)   # later ones weigh c itself by 0
        if len(dl) != len(gks) + 1:
            raise AssertionError("matmul_diag: one diagonal for the ciphertext itself and one per rotation")
        out = matmul_diag(gks[:DOT_MAX], dl[:DOT_MAX + 1], c)
        for k in range(DOT_MAX, len(gks), DOT_MAX):
            out = out + matmul_diag(gks[k:k + DOT_MAX], [ring.zero()] + dl[k + 1:k + DOT_MAX + 1], c)
        return out
    stacked = isinstance(diags, RingElement)              # one batched element holding the len(gks) + 1 diagonals back to back
    if stacked:
        if diags.ring != ring or diags.count != len(gks) + 1:
            raise UsageError("matmul_diag: a stacked plaintext element must hold one diagonal per rotation plus one")
    else:
        diags = list(diags)
        if len(diags) != len(gks) + 1:
            raise AssertionError("matmul_diag: one diagonal for the ciphertext itself and one per rotation")
        for d in diags:
            if not isinstance(d, RingElement) or d.ring != ring or d.count != 1:
                raise UsageError("matmul_diag: the diagonals are single plaintext elements of the ciphertext's ring")
    if gks:
        params = gks[0].key.params
        if any(g.key.params is not params for g in gks) or params.relin_window != 0:
            raise UsageError("hoisted rotations need Galois keys of one parameter set with RNS digits")
        keyring = gks[0].key.key[0].mask.ring
        special = isinstance(params, ModulusRaised)
    else:
        keyring, special = ring, False
    if keyring.idx != list(range(keyring.L)) or ring.idx != list(range(level)):
        raise UsageError("ciphertext ring is not a prefix of the key ring")
    prim = [x.coeffs_primal() for x in c.cs]               # both before the hand-over (see keyswitch)
    duals = [diags.coeffs_dual()] if stacked else [d.coeffs_dual() for d in diags]
    if ring.ctx is not keyring.ctx:
        if ring.N != keyring.N or ring.moduli != keyring.moduli[:level] or ring.psi != keyring.psi[:level]:
            raise UsageError("ciphertext and key belong to different rings")
        keyring.ctx.wait_for(ring.ctx)
    sz = level * ring.N
    dg = duals[0] if stacked else _pack(duals, ring, 1, ctx=keyring.ctx)   # [R+1][level][N]
    ct = _pack(prim, ring, n, ctx=keyring.ctx)
    out = DeviceBuffer(n * 2 * sz)
    keyring.ctx.matmul_diag(keyring.L, level, special, [g.prepared().ptr for g in gks], len(gks[0].key.key) if gks else level,
                            [g.galois_element for g in gks], dg.ptr, ct.ptr, out.ptr, n)
    res = _unpack(out, ring, n, 2, batch, primal=False, ctx=keyring.ctx)
    if ring.ctx is not keyring.ctx:
        ring.ctx.wait_for(keyring.ctx)
    return CipherText(c.params, res, Fraction(c.scale) ** 2)


def _grouped_key_set(gks, c, what):
    """the argument rules of rotate_many / matmul_diag for keys with grouped digits: (params, keyring)"""
    if len(c) != 2:
        raise AssertionError("rotate takes a 2-element ciphertext")
    params = gks[0].key.params
    if not isinstance(params, GroupedRaised) or any(g.key.params is not params for g in gks):
        raise UsageError(f"{what} needs Galois keys of one parameter set with grouped digits (GroupedRaised)")
    keyring = gks[0].key.key[0].mask.ring
    ring = c[0].ring
    if keyring.idx != list(range(keyring.L)) or ring.idx != list(range(ring.L)):
        raise UsageError("ciphertext ring is not a prefix of the key ring")
    if ring.ctx is not keyring.ctx and (ring.N != keyring.N or ring.moduli != keyring.moduli[:ring.L] or ring.psi != keyring.psi[:ring.L]):
        raise UsageError("ciphertext and key belong to different rings")
    return params, keyring


def rotate_many_grouped(gks, c: CipherText):
    """[rotate(gk, c) for gk in gks] on keys with grouped digits, from one digit decomposition of c (tfhe_rotate_many_grouped): the
    digits are decomposed and transformed once, each rotation costs one key sum, one inverse transform and one tail.  Each result is
    bit-identical to `rotate(gk, c)`."""
    gks = list(gks)
    if not gks:
        if len(c) != 2:
            raise AssertionError("rotate takes a 2-element ciphertext")
        return []
    params, keyring = _grouped_key_set(gks, c, "rotate_many_grouped")
    ring, n, batch = c[0].ring, c[0].count, c[0].batch
    level = ring.L
    prim = [x.coeffs_primal() for x in c.cs]               # before the hand-over (see keyswitch)
    if ring.ctx is not keyring.ctx:
        keyring.ctx.wait_for(ring.ctx)
    sz = level * ring.N
    ct = _pack(prim, ring, n, ctx=keyring.ctx)
    out = DeviceBuffer(len(gks) * n * 2 * sz)
    keyring.ctx.rotate_many_grouped(keyring.L, level, params.n_special, params.group, [g.prepared_grouped().ptr for g in gks],
                                    len(gks[0].key.key), [g.galois_element for g in gks], ct.ptr, out.ptr, n)
    res = []
    for r in range(len(gks)):
        view = _View(out, r * n * 2 * sz)
        res.append(CipherText(c.params, _unpack(view, ring, n, 2, batch, primal=True, ctx=keyring.ctx), c.scale))
    if ring.ctx is not keyring.ctx:
        ring.ctx.wait_for(keyring.ctx)
    return res


def matmul_diag_grouped(gks, diags, c: CipherText) -> CipherText:
    """matmul_diag on keys with grouped digits (tfhe_matmul_diag_grouped): diags[0] .* c + sum_k diags[k] .* rotate(gks[k-1], c) in one
    device call, the rotations hoisted as in rotate_many_grouped.  `diags` as for matmul_diag; at least one key (the parameter set is
    read from it).  Bit-identical to `CipherText.dot_plain([c] + rotate_many_grouped(gks, c), diags)`; NTT domain, squared scale."""
    gks = list(gks)
    if not gks:
        raise UsageError("matmul_diag_grouped needs at least one Galois key (GroupedRaised); without rotations it is a plain product")
    params, keyring = _grouped_key_set(gks, c, "matmul_diag_grouped")
    c._need_scale()
    ring, n, batch = c[0].ring, c[0].count, c[0].batch
    level = ring.L
    if len(gks) > DOT_MAX:          # as matmul_diag: partial products of DOT_MAX rotations, the later ones weigh c itself by 0
        dl = diags.split([1] * diags.count) if isinstance(diags, RingElement) else list(diags)
        if len(dl) != len(gks) + 1:
            raise AssertionError("matmul_diag_grouped: one diagonal for the ciphertext itself and one per rotation")
        out = matmul_diag_grouped(gks[:DOT_MAX], dl[:DOT_MAX + 1], c)
        for k in range(DOT_MAX, len(gks), DOT_MAX):
            out = out + matmul_diag_grouped(gks[k:k + DOT_MAX], [ring.zero()] + dl[k + 1:k + DOT_MAX + 1], c)
        return out
    stacked = isinstance(diags, RingElement)
    if stacked:
        if diags.ring != ring or diags.count != len(gks) + 1:
            raise UsageError("matmul_diag_grouped: a stacked plaintext element must hold one diagonal per rotation plus one")
    else:
        diags = list(diags)
        if len(diags) != len(gks) + 1:
            raise AssertionError("matmul_diag_grouped: one diagonal for the ciphertext itself and one per rotation")
        for d in diags:
            if not isinstance(d, RingElement) or d.ring != ring or d.count != 1:
                raise UsageError("matmul_diag_grouped: the diagonals are single plaintext elements of the ciphertext's ring")
    prim = [x.coeffs_primal() for x in c.cs]               # both before the hand-over (see keyswitch)
    duals = [diags.coeffs_dual()] if stacked else [d.coeffs_dual() for d in diags]
    if ring.ctx is not keyring.ctx:
        keyring.ctx.wait_for(ring.ctx)
    sz = level * ring.N
    dg = duals[0] if stacked else _pack(duals, ring, 1, ctx=keyring.ctx)   # [R+1][level][N]
    ct = _pack(prim, ring, n, ctx=keyring.ctx)
    out = DeviceBuffer(n * 2 * sz)
    keyring.ctx.matmul_diag_grouped(keyring.L, level, params.n_special, params.group, [g.prepared_grouped().ptr for g in gks],
                                    len(gks[0].key.key), [g.galois_element for g in gks], dg.ptr, ct.ptr, out.ptr, n)
    res = _unpack(out, ring, n, 2, batch, primal=False, ctx=keyring.ctx)
    if ring.ctx is not keyring.ctx:
        ring.ctx.wait_for(keyring.ctx)
    return CipherText(c.params, res, Fraction(c.scale) ** 2)


def bsgs_diagonals(dv, n1: int, block: int = 1):
    """The baby-step/giant-step regrouping of a diagonal product.  `dv[k]`, k < n, are slot vectors: diagonal k multiplies the
    rotation of the input by k * block slots (rotation by s steps acts on the slots as np.roll(x, s)).  With k = j n1 + i,
        sum_k dv[k] * roll(x, k block) = sum_j roll( sum_i D[j][i] * roll(x, i block), j n1 block ),
        D[j][i] = np.roll(dv[j n1 + i], -j n1 block)        (rows with j n1 + i >= n are zero).
    Returns (D, baby_steps, giant_steps): D of shape [n2][n1'][slots] with n2 = ceil(n / n1) and n1' = min(n1, n), and the rotation
    steps the two key sets are made for (keygen_galois_many): [i block for 0 < i < n1'], [j n1 block for 0 < j < n2].  Encode
    D.reshape(n2 * n1', slots) for `matmul_bsgs`."""
    dv = np.asarray(dv)
    if dv.ndim != 2 or n1 < 1 or block < 1:
        raise AssertionError("bsgs_diagonals: dv is [n][slots], n1 >= 1, block >= 1")
    n = dv.shape[0]
    n1 = min(int(n1), n)
    n2 = -(-n // n1)
    D = np.zeros((n2, n1) + dv.shape[1:], dtype=dv.dtype)
    for k in range(n):
        j, i = divmod(k, n1)
        D[j, i] = np.roll(dv[k], -j * n1 * block, axis=-1)
    return D, [i * block for i in range(1, n1)], [j * n1 * block for j in range(1, n2)]


def matmul_bsgs(baby_gks, giant_gks, diags, c: CipherText) -> CipherText:
    """The diagonal product by baby and giant steps in ONE device call (tfhe_matmul_bsgs):
        inner_j = sum_i diags[j][i] .* NTT(r_i(c)),   r_0 = identity, r_i = rotate(baby_gks[i - 1], .)
        result  = inner_0 + sum_{j >= 1} rotate(giant_gks[j - 1], inner_j)
    `diags`: len(giant_gks) + 1 lists of len(baby_gks) + 1 plaintext elements of c's ring at c's scale (one polynomial each, shared
    by the batch), or ONE stacked element holding the (len(giant_gks) + 1)(len(baby_gks) + 1) diagonals back to back, giant step
    major (what ckks_encode returns for bsgs_diagonals(..)[0].reshape(-1, slots)).  Pre-rotating them is the caller's business
    (bsgs_diagonals).  Word for word rotate_many -> dot_plain per giant step -> rotate -> +; the result is in the coefficient
    domain, at the squared scale."""
    baby_gks, giant_gks = list(baby_gks), list(giant_gks)
    _refuse_grouped_keys(baby_gks + giant_gks, "matmul_bsgs")
    if len(c) != 2:
        raise AssertionError("rotate takes a 2-element ciphertext")
    c._need_scale()
    if len(baby_gks) > DOT_MAX or len(giant_gks) > DOT_MAX:
        raise UsageError(f"matmul_bsgs: at most {DOT_MAX} baby and {DOT_MAX} giant steps per call")
    ring, n, batch = c[0].ring, c[0].count, c[0].batch
    level = ring.L
    nb1, ng1 = len(baby_gks) + 1, len(giant_gks) + 1
    stacked = isinstance(diags, RingElement)
    if stacked:
        if diags.ring != ring or diags.count != ng1 * nb1:
            raise UsageError("matmul_bsgs: a stacked plaintext element must hold (giant steps + 1) x (baby steps + 1) diagonals")
    else:
        diags = [list(row) for row in diags]
        if len(diags) != ng1 or any(len(row) != nb1 for row in diags):
            raise AssertionError("matmul_bsgs: one row of diagonals per giant step plus one, one diagonal per baby step plus one in each")
        diags = [d for row in diags for d in row]
        for d in diags:
            if not isinstance(d, RingElement) or d.ring != ring or d.count != 1:
                raise UsageError("matmul_bsgs: the diagonals are single plaintext elements of the ciphertext's ring")
    gks = baby_gks + giant_gks
    if gks:
        params = gks[0].key.params
        if any(g.key.params is not params for g in gks) or params.relin_window != 0:
            raise UsageError("hoisted rotations need Galois keys of one parameter set with RNS digits")
        keyring = gks[0].key.key[0].mask.ring
        special = isinstance(params, ModulusRaised)
    else:
        keyring, special = ring, False
    if keyring.idx != list(range(keyring.L)) or ring.idx != list(range(level)):
        raise UsageError("ciphertext ring is not a prefix of the key ring")
    prim = [x.coeffs_primal() for x in c.cs]               # both before the hand-over (see keyswitch)
    duals = [diags.coeffs_dual()] if stacked else [d.coeffs_dual() for d in diags]
    if ring.ctx is not keyring.ctx:
        if ring.N != keyring.N or ring.moduli != keyring.moduli[:level] or ring.psi != keyring.psi[:level]:
            raise UsageError("ciphertext and key belong to different rings")
        keyring.ctx.wait_for(ring.ctx)
    sz = level * ring.N
    dg = duals[0] if stacked else _pack(duals, ring, 1, ctx=keyring.ctx)   # [ng1][nb1][level][N]
    ct = _pack(prim, ring, n, ctx=keyring.ctx)
    out = DeviceBuffer(n * 2 * sz)
    keyring.ctx.matmul_bsgs(keyring.L, level, special, [g.prepared().ptr for g in baby_gks], [g.galois_element for g in baby_gks],
                            [g.prepared().ptr for g in giant_gks], [g.galois_element for g in giant_gks],
                            len(gks[0].key.key) if gks else level, dg.ptr, ct.ptr, out.ptr, n)
    res = _unpack(out, ring, n, 2, batch, primal=True, ctx=keyring.ctx)
    if ring.ctx is not keyring.ctx:
        ring.ctx.wait_for(keyring.ctx)
    return CipherText(c.params, res, Fraction(c.scale) ** 2)


def matmul_bsgs_blocks(baby_gks, giant_gks, diags, cs, bias=None) -> CipherText:
    """The block-row product by baby and giant steps in ONE device call (tfhe_matmul_bsgs_blocks): the sum over the inputs cs[m] of
    matmul_bsgs(baby_gks, giant_gks, diags[m], cs[m]) as a circuit, but with the inner sums of all inputs added BEFORE the giant
    rotations (len(giant_gks) key switches instead of len(cs) times as many):
        inner_j = sum_m sum_i diags[m][j][i] .* NTT(r_i(cs[m])),   result = inner_0 + sum_{j >= 1} rotate(giant_gks[j - 1], inner_j) (+ bias)
    `diags`: one entry per input, each in either form `matmul_bsgs` takes; `cs`: two-element ciphertexts of one ring, level, scale and
    batch; `bias`: None, or a single plaintext element of that ring encoded at the RESULT's scale (c.scale ** 2), added to component
    0.  Word for word rotate_many per input -> ONE dot_plain per giant step over all terms -> rotate -> + (-> + bias); not the words
    of the per-input calls added up (the key switch's contraction rounds once per giant step here).  The result is in the
    coefficient domain, at the squared scale."""
    return _matmul_bsgs_blocks(baby_gks, giant_gks, diags, cs, bias, None)


def _fold_groups(fold_gk_groups):
    """the fold steps as a list of non-empty lists of Galois keys, 64 keys at the most"""
    groups = [list(grp) for grp in fold_gk_groups]
    if len(groups) > DOT_MAX or sum(len(grp) for grp in groups) > DOT_MAX:
        raise UsageError(f"rotate_sum: at most {DOT_MAX} fold steps and {DOT_MAX} fold keys per call")
    if any(not grp for grp in groups):
        raise UsageError("rotate_sum: a fold step without a key")
    return groups


def rotate_sum(gk_groups, c: CipherText) -> CipherText:
    """Rotate and sum in ONE device call (tfhe_rotate_sum): F_0 = c, F_{t+1} = F_t + sum_{gk in gk_groups[t]} rotate(gk, F_t), the result
    the last F.  `gk_groups`: a list of lists of Galois keys, one list per step.  With the keys of the steps s, 2 s, 4 s, ... one per
    group, the result holds in every slot the sum of the slots s apart ("sum of slots"; the fold that closes a product by extended
    diagonals, rect_diagonals).  Word for word rotate_many over a group's keys -> + per group; scale and domain are c's."""
    groups = _fold_groups(gk_groups)
    _refuse_grouped_keys([g for grp in groups for g in grp], "rotate_sum")
    if len(c) != 2:
        raise AssertionError("rotate takes a 2-element ciphertext")
    gks = [g for grp in groups for g in grp]
    if not gks:
        return c
    params = gks[0].key.params
    if any(g.key.params is not params for g in gks) or params.relin_window != 0:
        raise UsageError("hoisted rotations need Galois keys of one parameter set with RNS digits")
    keyring = gks[0].key.key[0].mask.ring
    ring, n, batch = c[0].ring, c[0].count, c[0].batch
    level, special = ring.L, isinstance(params, ModulusRaised)
    if keyring.idx != list(range(keyring.L)) or ring.idx != list(range(level)):
        raise UsageError("ciphertext ring is not a prefix of the key ring")
    prim = [x.coeffs_primal() for x in c.cs]               # before the hand-over (see keyswitch)
    if ring.ctx is not keyring.ctx:
        if ring.N != keyring.N or ring.moduli != keyring.moduli[:level] or ring.psi != keyring.psi[:level]:
            raise UsageError("ciphertext and key belong to different rings")
        keyring.ctx.wait_for(ring.ctx)
    ct = _pack(prim, ring, n, ctx=keyring.ctx)
    out = DeviceBuffer(n * 2 * level * ring.N)
    keyring.ctx.rotate_sum(keyring.L, level, special, [[g.prepared().ptr for g in grp] for grp in groups],
                           [[g.galois_element for g in grp] for grp in groups], len(gks[0].key.key), ct.ptr, out.ptr, n)
    res = _unpack(out, ring, n, 2, batch, primal=True, ctx=keyring.ctx)
    if ring.ctx is not keyring.ctx:
        ring.ctx.wait_for(keyring.ctx)
    return CipherText(c.params, res, c.scale)


def matmul_bsgs_fold(baby_gks, giant_gks, diags, cs, fold_gk_groups, bias=None) -> CipherText:
    """The product of a rectangular matrix in ONE device call (tfhe_matmul_bsgs_fold): matmul_bsgs_blocks(baby_gks, giant_gks, diags, cs)
    without a bias -> rotate_sum(fold_gk_groups, .) -> + bias, word for word.  With the extended diagonals and the fold steps of
    rect_diagonals it is W @ x for an m x n matrix, m | n, by m diagonals instead of the n of the matrix padded to n x n; every row r
    of the result holds (W @ x)[r mod m].  `bias` (at the RESULT's scale, c.scale ** 2) is added AFTER the fold, so it is the bias of
    the layer as it stands, replicated like the result.  Usage errors as matmul_bsgs_blocks; the result is in the coefficient domain,
    at the squared scale."""
    return _matmul_bsgs_blocks(baby_gks, giant_gks, diags, cs, bias, _fold_groups(fold_gk_groups))


def rect_diagonals(W, n1: int, block: int = 1, fold_radix: int = 4):
    """The diagonals and rotation steps of a RECTANGULAR matrix product, for matmul_bsgs_fold.  W is m0 x n; the input vector has n rows
    of `block` slots each (row r in slots r block .. r block + block - 1 of n block slots); rotation by s steps acts on the slots as
    np.roll(x, s), as for bsgs_diagonals.  Returns (D, baby_steps, giant_steps, fold_steps): D, baby_steps and giant_steps as
    bsgs_diagonals returns them, fold_steps a list of groups of slot steps, one group per fold step (keygen_galois_many makes the
    keys of a group).

    Wide (m0 <= n): W is padded with zero rows to m, the next power of two, and n / m must be a power of two.  The m EXTENDED
    diagonals dv[i][r block + c] = Wp[r mod m][(r - i) mod n] leave n / m partial sums m rows apart, which log2(n / m) fold steps add:
    radix 2 by one key per step, [[m block], [2 m block], ...]; radix 4 by three keys per step, [[s, 2 s, 3 s], [4 s, 8 s, 12 s], ...]
    with s = m block and one radix-2 group last when log2(n / m) is odd (half the steps, three times the keys and key sums per step).
    Radix 4 is the default: the fold steps depend on each other, and one step of three rotations measured faster than two steps of
    one at every size (profiles/LOG.md, matmul_rect), at the price of one more key per pair of steps.
    Afterwards row r holds (W @ x)[r mod m]: rows m0 <= r mod m < m read zero.  m = n is the square product: no fold step.

    Tall (m0 > n, n | m0): the n extended diagonals dv[i][r block + c] = W[r][(r - i) mod n] over m0 rows, no fold.  The INPUT must
    be periodic with period n block slots -- row r holding x[r mod n], which is what a wide product leaves behind."""
    W = np.asarray(W)
    if W.ndim != 2 or n1 < 1 or block < 1 or fold_radix not in (2, 4):
        raise AssertionError("rect_diagonals: W is [m0][n], n1 >= 1, block >= 1, fold_radix 2 or 4")
    m0, n = W.shape
    if m0 > n:
        if m0 % n:
            raise UsageError("rect_diagonals: a tall matrix needs its row count to be a multiple of its column count")
        r = np.arange(m0)
        dv = np.stack([np.repeat(W[r, (r - i) % n], block) for i in range(n)])
        return bsgs_diagonals(dv, n1, block) + ([],)
    m = 1 << max(0, int(m0 - 1).bit_length())
    if n % m or (n // m) & (n // m - 1):
        raise UsageError("rect_diagonals: the column count must be a power of two times the row count rounded up to a power of two")
    Wp = np.zeros((m, n), dtype=W.dtype)
    Wp[:m0] = W
    r = np.arange(n)
    dv = np.stack([np.repeat(Wp[r % m, (r - i) % n], block) for i in range(m)])
    folds, s, left = [], m * block, (n // m).bit_length() - 1
    while left:
        if fold_radix == 4 and left >= 2:
            folds.append([s, 2 * s, 3 * s]); s *= 4; left -= 2
        else:
            folds.append([s]); s *= 2; left -= 1
    return bsgs_diagonals(dv, n1, block) + (folds,)


def matmul_bsgs_grouped(baby_gks, giant_gks, diags, c: CipherText) -> CipherText:
    """matmul_bsgs on keys with grouped digits (tfhe_matmul_bsgs_grouped, one input): operands, diagonal handling (bsgs_diagonals), scale
    and result as for matmul_bsgs; at least one key (the parameter set is read from it).  Word for word rotate_many_grouped -> dot_plain
    per giant step -> rotate -> +."""
    return _matmul_bsgs_blocks(baby_gks, giant_gks, [diags], [c], None, None, grouped="matmul_bsgs_grouped")


def matmul_bsgs_blocks_grouped(baby_gks, giant_gks, diags, cs, bias=None) -> CipherText:
    """matmul_bsgs_blocks on keys with grouped digits (tfhe_matmul_bsgs_grouped): operands, usage errors, scale and result as for
    matmul_bsgs_blocks; the keys are Galois keys of ONE GroupedRaised parameter set, at least one of them."""
    return _matmul_bsgs_blocks(baby_gks, giant_gks, diags, cs, bias, None, grouped="matmul_bsgs_blocks_grouped")


def rotate_sum_grouped(gk_groups, c: CipherText) -> CipherText:
    """rotate_sum on keys with grouped digits (tfhe_rotate_sum_grouped): `gk_groups` a list of lists of Galois keys of ONE GroupedRaised
    parameter set, one list per fold step.  Word for word rotate_many_grouped over a step's keys -> + per step; scale and domain are c's."""
    groups = _fold_groups(gk_groups)
    if len(c) != 2:
        raise AssertionError("rotate takes a 2-element ciphertext")
    gks = [g for grp in groups for g in grp]
    if not gks:
        return c
    params, keyring = _grouped_key_set(gks, c, "rotate_sum_grouped")
    ring, n, batch = c[0].ring, c[0].count, c[0].batch
    level = ring.L
    prim = [x.coeffs_primal() for x in c.cs]               # before the hand-over (see keyswitch)
    if ring.ctx is not keyring.ctx:
        keyring.ctx.wait_for(ring.ctx)
    ct = _pack(prim, ring, n, ctx=keyring.ctx)
    out = DeviceBuffer(n * 2 * level * ring.N)
    keyring.ctx.rotate_sum_grouped(keyring.L, level, params.n_special, params.group, [[g.prepared_grouped().ptr for g in grp] for grp in groups],
                                   [[g.galois_element for g in grp] for grp in groups], len(gks[0].key.key), ct.ptr, out.ptr, n)
    res = _unpack(out, ring, n, 2, batch, primal=True, ctx=keyring.ctx)
    if ring.ctx is not keyring.ctx:
        ring.ctx.wait_for(keyring.ctx)
    return CipherText(c.params, res, c.scale)


def matmul_bsgs_fold_grouped(baby_gks, giant_gks, diags, cs, fold_gk_groups, bias=None) -> CipherText:
    """matmul_bsgs_fold on keys with grouped digits (tfhe_matmul_bsgs_fold_grouped): matmul_bsgs_blocks_grouped without a bias ->
    rotate_sum_grouped(fold_gk_groups, .) -> + bias, word for word.  Operands (rect_diagonals), usage errors, scale and result as for
    matmul_bsgs_fold; the keys are Galois keys of ONE GroupedRaised parameter set, at least one of them."""
    return _matmul_bsgs_blocks(baby_gks, giant_gks, diags, cs, bias, _fold_groups(fold_gk_groups), grouped="matmul_bsgs_fold_grouped")


def _matmul_bsgs_blocks(baby_gks, giant_gks, diags, cs, bias, fold_groups, grouped=None):
    """matmul_bsgs_blocks (fold_groups None) and matmul_bsgs_fold (a list of lists of Galois keys, possibly empty); grouped: the name of
    the caller that takes keys with grouped digits (matmul_bsgs_grouped / matmul_bsgs_blocks_grouped, which have no fold, and
    matmul_bsgs_fold_grouped)"""
    baby_gks, giant_gks, cs, diags = list(baby_gks), list(giant_gks), list(cs), list(diags)
    if grouped:
        fold_gks = [g for grp in fold_groups or [] for g in grp]
        if not baby_gks + giant_gks + fold_gks:
            raise UsageError(f"{grouped}: no Galois key at all (GroupedRaised) -- plain products, use .* and +")
        if not cs:
            raise UsageError("matmul_bsgs_blocks: one set of diagonals per input ciphertext, at least one input")
        gparams, gkeyring = _grouped_key_set(baby_gks + giant_gks + fold_gks, cs[0], grouped)
    else:
        _refuse_grouped_keys(baby_gks + giant_gks + [g for grp in fold_groups or [] for g in grp], "matmul_bsgs_blocks / matmul_bsgs_fold")
    if len(diags) != len(cs) or not cs:
        raise UsageError("matmul_bsgs_blocks: one set of diagonals per input ciphertext, at least one input")
    if len(cs) > DOT_MAX:
        raise UsageError(f"matmul_bsgs_blocks: at most {DOT_MAX} inputs per call")
    c = cs[0]
    for x in cs:
        if len(x) != 2:
            raise AssertionError("rotate takes a 2-element ciphertext")
        x._need_scale()
    if len(baby_gks) > DOT_MAX or len(giant_gks) > DOT_MAX:
        raise UsageError(f"matmul_bsgs: at most {DOT_MAX} baby and {DOT_MAX} giant steps per call")
    ring, n, batch = c[0].ring, c[0].count, c[0].batch
    for x in cs[1:]:
        if x[0].ring != ring or x[1].ring != ring or x.scale != c.scale or x[0].count != n or x[0].batch != batch or x.params is not c.params:
            raise UsageError("matmul_bsgs_blocks: the inputs are ciphertexts of one ring, level, scale and batch")
    level = ring.L
    nb1, ng1 = len(baby_gks) + 1, len(giant_gks) + 1
    forms = []                                             # per input: (stacked, element(s))
    for dm in diags:
        if isinstance(dm, RingElement):
            if dm.ring != ring or dm.count != ng1 * nb1:
                raise UsageError("matmul_bsgs: a stacked plaintext element must hold (giant steps + 1) x (baby steps + 1) diagonals")
            forms.append((True, dm))
        else:
            dm = [list(row) for row in dm]
            if len(dm) != ng1 or any(len(row) != nb1 for row in dm):
                raise AssertionError("matmul_bsgs: one row of diagonals per giant step plus one, one diagonal per baby step plus one in each")
            dm = [d for row in dm for d in row]
            for d in dm:
                if not isinstance(d, RingElement) or d.ring != ring or d.count != 1:
                    raise UsageError("matmul_bsgs: the diagonals are single plaintext elements of the ciphertext's ring")
            forms.append((False, dm))
    if bias is not None and (not isinstance(bias, RingElement) or bias.ring != ring or bias.count != 1):
        raise UsageError("matmul_bsgs_blocks: the bias is a single plaintext element of the ciphertexts' ring")
    gks = baby_gks + giant_gks + [g for grp in fold_groups or [] for g in grp]
    if grouped:
        keyring, special = gkeyring, False
    elif gks:
        params = gks[0].key.params
        if any(g.key.params is not params for g in gks) or params.relin_window != 0:
            raise UsageError("hoisted rotations need Galois keys of one parameter set with RNS digits")
        keyring = gks[0].key.key[0].mask.ring
        special = isinstance(params, ModulusRaised)
    else:
        keyring, special = ring, False
    if keyring.idx != list(range(keyring.L)) or ring.idx != list(range(level)):
        raise UsageError("ciphertext ring is not a prefix of the key ring")
    prims = [[e.coeffs_primal() for e in x.cs] for x in cs]   # all before the hand-over (see keyswitch)
    duals = [[d.coeffs_dual()] if stacked else [e.coeffs_dual() for e in d] for stacked, d in forms]
    bprim = None if bias is None else bias.coeffs_primal()
    if ring.ctx is not keyring.ctx:
        if ring.N != keyring.N or ring.moduli != keyring.moduli[:level] or ring.psi != keyring.psi[:level]:
            raise UsageError("ciphertext and key belong to different rings")
        keyring.ctx.wait_for(ring.ctx)
    sz = level * ring.N
    dgs = [du[0] if stacked else _pack(du, ring, 1, ctx=keyring.ctx) for (stacked, _), du in zip(forms, duals)]   # each [ng1][nb1][level][N]
    packed = {}                                            # (a ciphertext given twice is packed once: the call takes repeated pointers)
    cts = [packed[id(x)] if id(x) in packed else packed.setdefault(id(x), _pack(p, ring, n, ctx=keyring.ctx)) for x, p in zip(cs, prims)]
    out = DeviceBuffer(n * 2 * sz)
    if grouped:
        gkeys = (keyring.L, level, gparams.n_special, gparams.group, [g.prepared_grouped().ptr for g in baby_gks],
                 [g.galois_element for g in baby_gks], [g.prepared_grouped().ptr for g in giant_gks], [g.galois_element for g in giant_gks],
                 len(gks[0].key.key), [d.ptr for d in dgs], [t.ptr for t in cts])
        if fold_groups is None:
            keyring.ctx.matmul_bsgs_grouped(*gkeys, None if bprim is None else bprim.ptr, out.ptr, n)
        else:
            keyring.ctx.matmul_bsgs_fold_grouped(*gkeys, [[g.prepared_grouped().ptr for g in grp] for grp in fold_groups],
                                                 [[g.galois_element for g in grp] for grp in fold_groups],
                                                 None if bprim is None else bprim.ptr, out.ptr, n)
        res = _unpack(out, ring, n, 2, batch, primal=True, ctx=keyring.ctx)
        if ring.ctx is not keyring.ctx:
            ring.ctx.wait_for(keyring.ctx)
        return CipherText(c.params, res, Fraction(c.scale) ** 2)
    keys = (keyring.L, level, special, [g.prepared().ptr for g in baby_gks], [g.galois_element for g in baby_gks],
            [g.prepared().ptr for g in giant_gks], [g.galois_element for g in giant_gks], len(gks[0].key.key) if gks else level,
            [d.ptr for d in dgs], [t.ptr for t in cts])
    if fold_groups is None:
        keyring.ctx.matmul_bsgs_blocks(*keys, None if bprim is None else bprim.ptr, out.ptr, n)
    else:
        keyring.ctx.matmul_bsgs_fold(*keys, [[g.prepared().ptr for g in grp] for grp in fold_groups],
                                     [[g.galois_element for g in grp] for grp in fold_groups], None if bprim is None else bprim.ptr, out.ptr, n)
    res = _unpack(out, ring, n, 2, batch, primal=True, ctx=keyring.ctx)
    if ring.ctx is not keyring.ctx:
        ring.ctx.wait_for(keyring.ctx)
    return CipherText(c.params, res, Fraction(c.scale) ** 2)


class _View:
    """a window into a DeviceBuffer (keeps the parent alive)"""

    def __init__(self, parent, word_offset):
        self.parent, self.ptr = parent, parent.ptr + word_offset * 8


class _KeyView(_View):
    """`n_words` of a packed key buffer as a ring element's coefficient buffer (read-only: ring elements never write in place)"""

    def __init__(self, parent, word_offset, n_words):
        super().__init__(parent, word_offset)
        self.n = int(n_words)

    def to_numpy(self, shape=None) -> np.ndarray:
        out = np.empty(self.n, dtype=np.uint64)
        native.check(native.lib().tfhe_memcpy_d2h(out.ctypes.data, self.ptr, self.n * 8))
        return out.reshape(shape) if shape is not None else out


def modswitch(c: CipherText) -> CipherText:
    """modswitch(::CipherText{CKKSEncoding}), ckksencoding.jl:127-130: rescale every component by the
    last modulus; the scale is divided by it."""
    q_last = c[0].ring.moduli[-1]
    scale = None if c.scale is None else c.scale / q_last
    return CipherText(c.params, [x.modswitch() for x in c.cs], scale)


# --------------------------------------------------------------------------------------------------
# CKKS encoding (float; ckksencoding.jl:43-97, ckks.jl:35-59) -- host side, tolerance-level parity
# --------------------------------------------------------------------------------------------------


def scale_parts(scale):
    """scale = mant * 2^exp2 with a 64-bit integer mant: exact for 2^k and for integers below 2^64 (times 2^k),
    to 2^-63 relative otherwise (the boundary type of tfhe_ckks_encode / decode)."""
    fr = Fraction(scale)
    if fr <= 0:
        raise AssertionError("scale must be positive")
    num, den = fr.numerator, fr.denominator
    if den & (den - 1) == 0:                               # dyadic: strip common powers of two
        exp2 = -(den.bit_length() - 1)
        while num % 2 == 0:
            num //= 2; exp2 += 1
        if num < 2**64:
            return num, exp2
    e = (num.bit_length() - den.bit_length()) - 63         # approximate: 63-64 significant bits
    mant = int(round(fr / Fraction(2) ** e)) if e >= 0 else int(round(fr * Fraction(2) ** (-e)))
    if mant >= 2**64:
        mant //= 2; e += 1
    return mant, e


def ckks_encode(slots, ring: NegacyclicRing, scale) -> RingElement:
    """convert(RingElement, ::CKKSEncoding), ckksencoding.jl:72-97 -- on the device (tfhe_ckks_encode).
    slots: [N/2] complex, or [batch][N/2]."""
    z = np.ascontiguousarray(np.asarray(slots, dtype=np.complex128))
    batch = None if z.ndim == 1 else z.shape[0]
    z2 = z.reshape(-1, z.shape[-1])
    if 2 * z2.shape[1] != ring.N:
        raise AssertionError("CKKS plaintexts have N/2 slots")
    if ring.idx != list(range(ring.L)):
        raise UsageError("CKKS encoding: the ring must be a prefix of its context")
    mant, exp2 = scale_parts(scale)
    dz = DeviceBuffer.from_numpy(z2.view(np.uint64))
    out = DeviceBuffer(z2.shape[0] * ring.L * ring.N)
    ring.ctx.ckks_encode(ring.L, mant, exp2, dz.ptr, out.ptr, z2.shape[0])
    return RingElement(ring, out, None, batch)             # (dz is parked by the allocator until the kernels have read it)


def ckks_decode(el: RingElement, scale) -> np.ndarray:
    """CKKSEncoding{ScaleT}(plain), ckksencoding.jl:56-66 -- on the device (tfhe_ckks_decode)."""
    ring = el.ring
    if ring.idx != list(range(ring.L)):
        raise UsageError("CKKS decoding: the ring must be a prefix of its context")
    mant, exp2 = scale_parts(scale)
    n = el.count
    out = DeviceBuffer(n * ring.N)                         # N/2 complex doubles = N words per plaintext
    ring.ctx.ckks_decode(ring.L, mant, exp2, el.coeffs_primal().ptr, out.ptr, n)
    ring.ctx.sync()
    z = out.to_numpy().view(np.complex128).reshape(n, ring.N // 2)
    return z if el.batch is not None else z[0]


# --------------------------------------------------------------------------------------------------
# on-wire format (wire.py): device <-> bytes
# --------------------------------------------------------------------------------------------------

def dump_ciphertext(c: CipherText) -> bytes:
    """CipherText -> wire blob (coefficient domain, [count][polys][L][N])."""
    from . import wire
    ring = c[0].ring
    res = np.stack([x.to_numpy("primal").reshape(x.count, ring.L, ring.N) for x in c.cs], axis=1)
    scale = scale_parts(c.scale) if c.scale is not None else (0, 0)
    return wire.dump(res, ring.moduli, ring.psi, kind=wire.KIND_CIPHERTEXT, domain=0, scale=scale, unbatched=c[0].batch is None)


def load_ciphertext(blob: bytes, params) -> CipherText:
    """wire blob -> CipherText on the device; the ring (moduli, psi) must be the scheme's ciphertext ring at that level."""
    from . import wire
    d = wire.load(blob)
    if d["kind"] != wire.KIND_CIPHERTEXT or d["domain"] != 0:
        raise UsageError("not a coefficient-domain ciphertext blob")
    ring = params.R_cipher()
    L = len(d["moduli"])
    if L != ring.L:
        ring = ring.crtselect(range(L))
    if d["N"] != ring.N or d["moduli"] != list(ring.moduli) or d["psis"] != list(ring.psi):
        raise UsageError("blob ring does not match the parameters' ciphertext ring")
    res = d["residues"]
    batch = res.shape[0]
    cs = [RingElement.from_host(ring, res[0, p] if d["unbatched"] else res[:, p]) for p in range(d["polys"])]
    smant, sexp = d["scale"]
    scale = None if smant == 0 else Fraction(smant) * Fraction(2) ** sexp
    return CipherText(params, cs, scale)
