"""No-GPU checks of tfhe_matmul_bsgs_blocks (the block-row matrix product by baby and giant steps, several inputs in one device
call): the symbol is declared, exported, bound by ctypes and by the Julia shim with one signature; every argument check that does not
need the ring runs on the host before any device use, in the order the header states; the SEEDED accumulation bodies of the k_md_acc
kernels (csrc/lazy_sum.h), run on the CPU (tests/md_acc_emul/), chain three inputs into exact big-integer sums at 60-, 61- and
62-bit moduli; the gfx950 code objects of the seeded kernels use no scratch memory; and the mirror's usage errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import kernel_harness as KH
from tests import test_julia_shim_cpu as shim
from toyfhe_jl_amd import native, she

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ctx, key_limbs, level, special, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, n_digits, diags, cts, n_in, bias, out, batch)
BLOCKS = ("tfhe_matmul_bsgs_blocks",
          ["ptr", "int", "int", "int", "ptr", "ptr", "int", "ptr", "ptr", "int", "int", "ptr", "ptr", "int", "ptr", "ptr", "i64"])


def _err():
    return native.lib().tfhe_last_error().decode()


# ---- one signature everywhere --------------------------------------------------------------------------------------------

def test_symbol_declared_exported_and_bound_with_one_signature():
    name, classes = BLOCKS
    protos = shim.header_prototypes()
    assert name in protos, f"{name} is not declared in include/toyfhe_hip.h"
    assert protos[name] == ("int", classes)
    assert name in native.EXPORTED_SYMBOLS
    f = getattr(native.lib(), name)                      # AttributeError: not exported by the library
    assert f.restype is C.c_int and len(f.argtypes) == len(classes)
    for k, t in zip(classes, f.argtypes):
        if k == "ptr":
            assert t is C.c_void_p or hasattr(t, "contents"), t
        else:
            assert t is {"int": C.c_int, "i64": C.c_int64}[k], (k, t)
    assert f.argtypes[5]._type_ is C.c_uint64 and f.argtypes[8]._type_ is C.c_uint64     # the Galois elements are host u64 arrays
    assert f.argtypes[11]._type_ is C.c_void_p and f.argtypes[12]._type_ is C.c_void_p   # diags, cts: host arrays of device pointers
    assert callable(getattr(native.Context, "matmul_bsgs_blocks")) and callable(she.matmul_bsgs_blocks)
    import toyfhe_jl_amd as tf
    assert tf.matmul_bsgs_blocks is she.matmul_bsgs_blocks


def test_julia_shim_binds_the_same_signature():
    name, classes = BLOCKS
    calls = [c for c in shim.shim_ccalls() if c[0] == name]
    assert len(calls) == 1, f"the shim binds {name} exactly once"
    _, ret, argtypes, nargs = calls[0]
    assert ret == "int" and argtypes == classes and nargs == len(classes)
    src = open(shim.SHIM).read()
    body = src[src.index("function matmul_bsgs_blocks("):]
    body = body[:body.index("\nend")]
    assert "GC.@preserve" in body and re.search(r"\bon\(", body) and "prepared(" in body


def test_header_states_the_layouts_the_composition_and_the_checks():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    i = text.index("int tfhe_matmul_bsgs_blocks(")
    doc = text[text.rindex("/*", 0, i):i]
    for word in ("[n_giant + 1][n_baby + 1][level][N]", "[batch][2][level][N]", "[level][N]", "PREPARED", "HOST", "coefficient domain",
                 "NTT domain", "word for word", "tfhe_rotate_many", "tfhe_nntt", "tfhe_dot", "tfhe_inntt", "tfhe_rotate_prepared", "tfhe_add",
                 "tfhe_ctx_set_chunk", "same bits", "TFHE_E_BADARG", "batch == 0", "[0, 64]", "[1, 64]", "component 0",
                 "NOT the sum of n_in calls of tfhe_matmul_bsgs", "once per giant step", "more than once", "in this order"):
        assert word in doc, word
    # the stated order of the checks
    order = [doc.index(w) for w in ("null arrays", "null key", "diags[m] or cts[m] among", "outside [0, 64]", "outside [1, 64]",
                                    "even Galois element", "starting where", "then the context", "level / key-limb rules", "not below 2N",
                                    "overlapping any operand anywhere")]
    assert order == sorted(order), order


# ---- argument validation precedes device use -------------------------------------------------------------------------------

def test_argument_validation_precedes_device_use():
    """every status that does not need the ring, with no context and host pointers, in the header's order: each call breaks one rule
    and every LATER one too where it can (a null context always), and must report the earliest; a call that passes them all ends at
    "null context" without having touched a device"""
    f = native.lib().tfhe_matmul_bsgs_blocks
    bufs = [np.zeros(64, dtype=np.uint64) for _ in range(8)]
    pk, pk2, pd, pd2, pc, pc2, pb, po = (x.ctypes.data for x in bufs)

    def call(baby=(pk, pk2), bg=(3, 5), giant=(pk,), gg=(9,), n_baby=None, n_giant=None, diags=(pd, pd2), cts=(pc, pc2), n_in=None, bias=pb,
             out=po, batch=1, drop=None):
        # (every array is filled up to 65 valid entries behind the ones under test: a count out of range reads none that is not there)
        arr = lambda t, xs, fill: (t * 65)(*(list(xs) + [fill] * (65 - len(xs))))
        args = dict(baby=arr(C.c_void_p, baby, pk), bg=arr(C.c_uint64, bg, 3), giant=arr(C.c_void_p, giant, pk), gg=arr(C.c_uint64, gg, 3),
                    diags=arr(C.c_void_p, diags, pd), cts=arr(C.c_void_p, cts, pc))
        if drop:
            args[drop] = None
        return f(None, 3, 2, 1, args["baby"], args["bg"], len(baby) if n_baby is None else n_baby, args["giant"], args["gg"],
                 len(giant) if n_giant is None else n_giant, 2, args["diags"], args["cts"], len(cts) if n_in is None else n_in, bias, out, batch)
    # 1. nulls: the arrays (even with a count out of range, an even Galois element and out on an operand behind them) ...
    for drop in ("baby", "bg", "giant", "gg", "diags", "cts"):
        assert call(drop=drop, n_in=0, gg=(4,), out=pb) == native.E_BADARG and "null argument" in _err(), drop
    assert call(out=None) == native.E_BADARG and "null argument" in _err()
    # ... a null key, a null entry per input, each ahead of a count out of range
    assert call(baby=(pk, None), n_in=0) == native.E_BADARG and "null baby key 1" in _err()
    assert call(giant=(None,), n_baby=-1) == native.E_BADARG and "null giant key 0" in _err()
    assert call(diags=(pd, None), n_giant=65, n_baby=-1) == native.E_BADARG and "null diagonals of input 1" in _err()
    assert call(cts=(None, pc2), n_baby=65) == native.E_BADARG and "null ciphertext of input 0" in _err()
    # a null entry beyond its count is not read
    assert call(baby=(None,), n_baby=0, giant=(None,), n_giant=0, diags=(pd, None), cts=(pc, None), n_in=1) == native.E_BADARG \
        and "null context" in _err()
    # 2. the counts, ahead of an even Galois element
    for n in (-1, 65):
        assert call(n_baby=n, gg=(4,)) == native.E_BADARG and "n_baby" in _err(), n
        assert call(n_giant=n, bg=(3, 4)) == native.E_BADARG and "n_giant" in _err(), n
    for n in (0, -1, 65):
        assert call(n_in=n, gg=(4,)) == native.E_BADARG and "n_in" in _err(), n
    # 3. an even Galois element, ahead of out on an operand
    assert call(bg=(3, 4), out=pc) == native.E_BADARG and "galois element must be odd" in _err()
    assert call(gg=(0,), out=pb) == native.E_BADARG and "galois element must be odd" in _err()
    # 4. out starting where an operand starts: any input's ciphertext or diagonals, the bias
    for o in (pc, pc2, pd, pd2, pb):
        assert call(out=o) == native.E_BADARG and "out overlaps an operand" in _err()
    # 5. everything that needs no ring passed: the context is next; without a bias, with one input, with a ciphertext given twice,
    # and an empty batch needs one too
    assert call() == native.E_BADARG and "null context" in _err()
    assert call(bias=None) == native.E_BADARG and "null context" in _err()
    assert call(diags=(pd,), cts=(pc,)) == native.E_BADARG and "null context" in _err()
    assert call(cts=(pc, pc)) == native.E_BADARG and "null context" in _err()
    assert call(batch=0) == native.E_BADARG and "null context" in _err()
    with pytest.raises(AssertionError):
        native.check(call(n_in=0))


# ---- the seeded accumulation bodies on the CPU -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return KH.md_acc_emul(tmp_path_factory.mktemp("md_acc_emul"))


def _moduli():
    """(q, lazy-reduction chunk): the next primes above 2^59, 2^60 and 2^61 (60, 61 and 62 bits: chunks 4, 2 and 1), N = 64"""
    out = [(H.primes_above(1 << 59, 1, 64)[0], 4), (H.primes_above(1 << 60, 1, 64)[0], 2), (H.primes_above(1 << 61, 1, 64)[0], 1)]
    assert [q.bit_length() for q, _ in out] == [60, 61, 62]
    return out


@pytest.mark.parametrize("q,chunk", _moduli())
@pytest.mark.parametrize("edge", [False, True])
def test_seeded_accumulation_bodies_match_exact_sums(emul, q, chunk, edge):
    """three inputs of n_baby + 1 = 6 and 9 terms each chained through the seed (18 / 27 terms per sum, every input above the chunk),
    both forms, every output tile (1, 2, 4 giant steps per pass) at whole and ragged tile counts, with random words and with every
    word q - 1 (the seed q - 1 under `chunk` products of (q - 1)^2: the top of the Barrett window).  `inner` arrives full of q - 1:
    input 0 must not read it."""
    assert emul.md_acc_emul_chunk(q) == chunk
    n, nin = 64, 3
    rng = np.random.default_rng(q % 1000 + edge)
    pinv = int(rng.integers(1, 1 << 29)) % q or 1
    for nrot, ngiant1, tile in ((5, 1, 1), (5, 2, 2), (8, 3, 4), (5, 4, 4), (8, 5, 4), (5, 2, 4), (5, 3, 2), (8, 2, 1)):
        assert nrot + 1 > chunk
        x = H.words_mod(rng, q, (nin, 2, n), edge)
        diag = H.words_mod(rng, q, (nin, ngiant1, nrot + 1, n), edge)
        # the dense form: ROT rows as they are (component 0 of x)
        rot = H.words_mod(rng, q, (nin, nrot, n), edge)
        x0 = np.ascontiguousarray(x[:, 0])
        inner = np.full((ngiant1, n), q - 1, dtype=np.uint64)
        assert emul.md_acc_emul_dense(q, tile, n, nrot, ngiant1, nin, x0.ctypes.data, rot.ctypes.data, diag.ctypes.data, inner.ctypes.data) == 0
        for j in range(ngiant1):
            want = 0
            for m in range(nin):
                terms = [x0[m].astype(object)] + [rot[m][t].astype(object) for t in range(nrot)]
                want = want + sum(diag[m][j][i].astype(object) * terms[i] for i in range(nrot + 1))
            assert np.array_equal(inner[j].astype(object), want % q), ("dense", q, nrot, ngiant1, tile, j)
        # the gather form: rotated value V[pi_r k] - U[k] (U scaled by P^-1 in the term where uscale is set)
        gs = np.array([int(g) for g in rng.choice(np.arange(3, 2 * n, 2), nrot, replace=False)], dtype=np.uint64)
        v = H.words_mod(rng, q, (nin, nrot, n, 2), False)
        u = H.words_mod(rng, q, (nin, 2, nrot, n), edge)
        for uscale in (0, 1):
            i0, i1 = np.full((ngiant1, n), q - 1, dtype=np.uint64), np.full((ngiant1, n), q - 1, dtype=np.uint64)
            assert emul.md_acc_emul_gather(q, tile, uscale, pinv, n, nrot, ngiant1, nin, x.ctypes.data, v.ctypes.data, u.ctypes.data,
                                                gs.ctypes.data, diag.ctypes.data, i0.ctypes.data, i1.ctypes.data) == 0
            for s, got in ((0, i0), (1, i1)):
                want = [0] * ngiant1
                for m in range(nin):
                    terms = [x[m][s].astype(object)]
                    for t in range(nrot):
                        uu = u[m][s][t].astype(object) * (pinv if uscale else 1) % q
                        terms.append((v[m][t][H.galois_pos(n, int(gs[t])), s].astype(object) - uu) % q)
                    for j in range(ngiant1):
                        want[j] = want[j] + sum(diag[m][j][i].astype(object) * terms[i] for i in range(nrot + 1))
                for j in range(ngiant1):
                    assert np.array_equal(got[j].astype(object), want[j] % q), ("gather", q, nrot, ngiant1, tile, uscale, s, j)
    assert emul.md_acc_emul_dense(q, 3, n, 0, 1, 1, None, None, None, None) == -1


# ---- resources of the gfx950 code objects ------------------------------------------------------------------------------------

@KH.needs_hipcc
def test_seeded_accumulation_kernels_use_no_scratch(tmp_path):
    """compiler-reported scratch is 0 for every seeded instantiation tfhe_matmul_bsgs_blocks launches (k_md_acc<., 1, true> holds 16
    accumulators and their seeds next to the gathers of the next rotation: the tightest of them)"""
    kernels = KH.kernel_resources("md_acc_emul/resource_probe.hip", tmp_path, ["PROBE_SEED=1"])
    seeded = [k for k in kernels if re.match(r"_Z\d+k_md_acc(ILb[01]ELi[124]ELb1EE|_denseILi[124]ELb1EE)", k["name"])]   # <USCALE, NG, true> / <NG, true>
    assert len(seeded) == 9, [k["name"] for k in kernels]   # 6 x k_md_acc, 3 x k_md_acc_dense
    for k in seeded:
        print(f"{k['name']}: {k['vgprs']} VGPRs, {k['agprs']} AGPRs, scratch {k['scratch']}")
        assert k["scratch"] == 0, (k["name"], k["scratch"])


def test_dispatch_launches_exactly_the_probed_forms():
    """csrc/md_api.inc launches the seeded forms for the inputs after the first of a chunk and the unseeded ones for input 0"""
    src = open(os.path.join(ROOT, "toyfhe.jl_amd", "csrc", "md_api.inc")).read()
    run = src[src.index("static int matmul_bsgs_run("):src.index("int tfhe_matmul_bsgs(")]
    assert "m == 0 ? (scaled ? k_md_acc<false, NG> : k_md_acc<true, NG>)" in run
    assert "k_md_acc<false, NG, true> : k_md_acc<true, NG, true>" in run
    assert "m == 0 ? k_md_acc_dense<NG> : k_md_acc_dense<NG, true>" in run
    assert run.index("for (int64_t b0 = 0;") < run.index("for (int m = 0; m < n_in; m++)")    # input 0 of EVERY chunk is unseeded


# ---- the mirror's usage errors ---------------------------------------------------------------------------------------------

class _Ring:
    L = 2

    def __init__(self, name):
        self.name = name

    def __eq__(self, other):
        return isinstance(other, _Ring) and self.name == other.name

    def __ne__(self, other):
        return not self == other


class _Stub:
    """a two-element ciphertext as far as the checks ahead of any device use look at it"""

    class _El:
        def __init__(self, ring, count, batch):
            self.ring, self.count, self.batch = ring, count, batch

    def __init__(self, ring="R", scale=2**20, count=2, batch=2, n=2, params="P"):
        self.cs = [self._El(_Ring(ring), count, batch) for _ in range(n)]
        self.scale, self.params = scale, params

    def __len__(self):
        return len(self.cs)

    def __getitem__(self, i):
        return self.cs[i]

    def _need_scale(self):
        if self.scale is None:
            raise she.UsageError("no scale")


def test_mirror_usage_errors():
    """what she.matmul_bsgs_blocks refuses before it touches a device: differing list lengths, no input, more than 64 inputs,
    ciphertexts of differing rings / scales / batches, a three-element ciphertext, too many steps, diagonals of the wrong shape"""
    f = she.matmul_bsgs_blocks
    c = _Stub()
    with pytest.raises(she.UsageError, match="one set of diagonals per input"):
        f([], [], [[[None]]], [c, c])
    with pytest.raises(she.UsageError, match="one set of diagonals per input"):
        f([], [], [], [])
    with pytest.raises(she.UsageError, match="at most 64 inputs"):
        f([], [], [[[None]]] * 65, [c] * 65)
    with pytest.raises(AssertionError, match="2-element"):
        f([], [], [[[None]]] * 2, [c, _Stub(n=3)])
    for other in (_Stub(ring="S"), _Stub(scale=2**21), _Stub(count=3), _Stub(batch=3), _Stub(params="Q")):
        with pytest.raises(she.UsageError, match="one ring, level, scale and batch"):
            f([], [], [[[None]]] * 2, [c, other])
    with pytest.raises(she.UsageError, match="at most 64 baby and 64 giant"):
        f([None] * 65, [], [[[None]]], [c])
    with pytest.raises(AssertionError, match="one row of diagonals per giant step plus one"):
        f([], [], [[[None], [None]]], [c])                       # two rows for no giant step
    with pytest.raises(she.UsageError, match="single plaintext elements"):
        f([], [], [[[None]]], [c])                               # not a ring element
