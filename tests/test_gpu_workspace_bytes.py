"""The bytes every key-switch and product entry point takes of the context workspace, pinned.

Each case calls ONE entry point ONCE on a fresh context with random operands and compares Context.workspace()[1] with a literal: first
uncapped, then on a second fresh context under set_chunk(2).  The words are other modules' business (tests/test_gpu_dirty_workspace.py,
tests/test_gpu_chunk_seams.py and the grouped modules hold them to the oracle); what is pinned here is the layout's size -- region 0
(the transforms' scratch above N = 2^14, a nested key switch's span), the chunked rows and the fixed tails -- so that a change to how a
workspace is carved shows up as a number.  BYTES was printed by the commit before the workspaces were laid out through ws_layout.h
(a648a96) on an MI355X, and has to hold unchanged.

Rings are the smallest that select each route: KS_THREE at 2^10, KS_ROW with the key as doubles at 2^13, KS_SUB at 2^15 (50x3), 2^15 at
40x4, the fused product cores with their parking rows at 2^12 (tfhe_mul_relin only), and for the grouped-digit keys N = 64 and 2^15 with
two special primes, digits of two limbs and a ciphertext of three.  Batch 3 (chunks 2 + 1 under the cap); tfhe_rotate_prepared also at
batch 8, where the rotation rides on the tail's stores at 2^15."""
import functools

import numpy as np
import pytest

import toyfhe_jl_amd as tf
from oracle import spec
from tests import helpers as H
from tests.test_gpu_chunk_seams import ring_of

pytestmark = pytest.mark.gpu

BATCH, CAP, W = 3, 2, 20

PLAIN_RINGS = [(1 << 10, "40x4", 0), (1 << 10, "40x4", 1), (1 << 13, "50x4", 1), (1 << 15, "50x3", 0), (1 << 15, "50x3", 1),
               (1 << 15, "40x4", 0), (1 << 15, "40x4", 1)]
PLAIN_ENTRIES = ["keyswitch-2", "keyswitch-3", "rotate", "rotate_prepared", "rotate_prepared-b8", "rotate_many", "rotate_many_prepared",
                 "keyswitch_window", "matmul_diag", "matmul_bsgs", "matmul_bsgs_blocks", "rotate_sum", "matmul_bsgs_fold", "mul_relin-r0",
                 "mul_relin-r1"]
GROUPED_RINGS = [(64, 30, 6), (1 << 15, 40, 5)]      # N, bits, key limbs; k = 2 special primes, digits of 2 limbs, level 3
GROUPED_ENTRIES = ["keyswitch_grouped-2", "keyswitch_grouped-3", "rotate_grouped", "rotate_many_grouped", "matmul_diag_grouped",
                   "matmul_bsgs_grouped", "mul_relin_grouped-r0", "mul_relin_grouped-r1"]
K, GROUP, GLEVEL = 2, 2, 3

# id -> (bytes uncapped, bytes under set_chunk(2))
BYTES = {
    "1024-40x4-s0-keyswitch-2": (589824, 393216),
    "1024-40x4-s0-keyswitch-3": (589824, 393216),
    "1024-40x4-s0-rotate": (786432, 524288),
    "1024-40x4-s0-rotate_prepared": (983040, 655360),
    "1024-40x4-s0-rotate_prepared-b8": (2621440, 655360),
    "1024-40x4-s0-rotate_many": (1245184, 917504),
    "1024-40x4-s0-rotate_many_prepared": (983040, 655360),
    "1024-40x4-s0-keyswitch_window": (1081344, 720896),
    "1024-40x4-s0-matmul_diag": (1376256, 917504),
    "1024-40x4-s0-matmul_bsgs": (2949120, 1966080),
    "1024-40x4-s0-matmul_bsgs_blocks": (2949120, 1966080),
    "1024-40x4-s0-rotate_sum": (786432, 524288),
    "1024-40x4-s0-matmul_bsgs_fold": (3342336, 2228224),
    "1024-40x4-s0-mul_relin-r0": (1277952, 851968),
    "1024-40x4-s0-mul_relin-r1": (1474560, 983040),
    "1024-40x4-s1-keyswitch-2": (491520, 327680),
    "1024-40x4-s1-keyswitch-3": (491520, 327680),
    "1024-40x4-s1-rotate": (638976, 425984),
    "1024-40x4-s1-rotate_prepared": (835584, 557056),
    "1024-40x4-s1-rotate_prepared-b8": (2228224, 557056),
    "1024-40x4-s1-rotate_many": (1097728, 819200),
    "1024-40x4-s1-rotate_many_prepared": (835584, 557056),
    "1024-40x4-s1-keyswitch_window": (884736, 589824),
    "1024-40x4-s1-matmul_diag": (1228800, 819200),
    "1024-40x4-s1-matmul_bsgs": (2408448, 1605632),
    "1024-40x4-s1-matmul_bsgs_blocks": (2408448, 1605632),
    "1024-40x4-s1-rotate_sum": (638976, 425984),
    "1024-40x4-s1-matmul_bsgs_fold": (2703360, 1802240),
    "1024-40x4-s1-mul_relin-r0": (1007616, 671744),
    "1024-40x4-s1-mul_relin-r1": (1155072, 770048),
    "8192-50x4-s1-keyswitch-2": (4718592, 3670016),
    "8192-50x4-s1-keyswitch-3": (4718592, 3670016),
    "8192-50x4-s1-rotate": (5898240, 4456448),
    "8192-50x4-s1-rotate_prepared": (6684672, 4456448),
    "8192-50x4-s1-rotate_prepared-b8": (17825792, 4456448),
    "8192-50x4-s1-rotate_many": (5898240, 4456448),
    "8192-50x4-s1-rotate_many_prepared": (6684672, 4456448),
    "8192-50x4-s1-keyswitch_window": (7864320, 5242880),
    "8192-50x4-s1-matmul_diag": (9830400, 6553600),
    "8192-50x4-s1-matmul_bsgs": (19267584, 12845056),
    "8192-50x4-s1-matmul_bsgs_blocks": (19267584, 12845056),
    "8192-50x4-s1-rotate_sum": (5898240, 4456448),
    "8192-50x4-s1-matmul_bsgs_fold": (21626880, 14417920),
    "8192-50x4-s1-mul_relin-r0": (73596928, 71958528),
    "8192-50x4-s1-mul_relin-r1": (74776576, 72744960),
    "32768-50x3-s0-keyswitch-2": (14155776, 11010048),
    "32768-50x3-s0-keyswitch-3": (14155776, 11010048),
    "32768-50x3-s0-rotate": (18874368, 14155776),
    "32768-50x3-s0-rotate_prepared": (28311552, 18874368),
    "32768-50x3-s0-rotate_prepared-b8": (42467328, 14155776),
    "32768-50x3-s0-rotate_many": (33030144, 23592960),
    "32768-50x3-s0-rotate_many_prepared": (28311552, 18874368),
    "32768-50x3-s0-keyswitch_window": (42467328, 28311552),
    "32768-50x3-s0-matmul_diag": (40108032, 26738688),
    "32768-50x3-s0-matmul_bsgs": (73138176, 48758784),
    "32768-50x3-s0-matmul_bsgs_blocks": (73138176, 48758784),
    "32768-50x3-s0-rotate_sum": (18874368, 14155776),
    "32768-50x3-s0-matmul_bsgs_fold": (82575360, 55050240),
    "32768-50x3-s0-mul_relin-r0": (30670848, 22020096),
    "32768-50x3-s0-mul_relin-r1": (35389440, 25165824),
    "32768-50x3-s1-keyswitch-2": (12582912, 9437184),
    "32768-50x3-s1-keyswitch-3": (12582912, 9437184),
    "32768-50x3-s1-rotate": (15728640, 11534336),
    "32768-50x3-s1-rotate_prepared": (22020096, 14680064),
    "32768-50x3-s1-rotate_prepared-b8": (36700160, 11534336),
    "32768-50x3-s1-rotate_many": (26738688, 19398656),
    "32768-50x3-s1-rotate_many_prepared": (22020096, 14680064),
    "32768-50x3-s1-keyswitch_window": (33030144, 22020096),
    "32768-50x3-s1-matmul_diag": (36175872, 24117248),
    "32768-50x3-s1-matmul_bsgs": (55050240, 36700160),
    "32768-50x3-s1-matmul_bsgs_blocks": (55050240, 36700160),
    "32768-50x3-s1-rotate_sum": (15728640, 11534336),
    "32768-50x3-s1-matmul_bsgs_fold": (61341696, 40894464),
    "32768-50x3-s1-mul_relin-r0": (23592960, 16777216),
    "32768-50x3-s1-mul_relin-r1": (26738688, 18874368),
    "32768-40x4-s0-keyswitch-2": (20971520, 16777216),
    "32768-40x4-s0-keyswitch-3": (20971520, 16777216),
    "32768-40x4-s0-rotate": (27262976, 20971520),
    "32768-40x4-s0-rotate_prepared": (44040192, 29360128),
    "32768-40x4-s0-rotate_prepared-b8": (58720256, 20971520),
    "32768-40x4-s0-rotate_many": (52428800, 37748736),
    "32768-40x4-s0-rotate_many_prepared": (44040192, 29360128),
    "32768-40x4-s0-keyswitch_window": (62914560, 41943040),
    "32768-40x4-s0-matmul_diag": (56623104, 37748736),
    "32768-40x4-s0-matmul_bsgs": (106954752, 71303168),
    "32768-40x4-s0-matmul_bsgs_blocks": (106954752, 71303168),
    "32768-40x4-s0-rotate_sum": (27262976, 20971520),
    "32768-40x4-s0-matmul_bsgs_fold": (119537664, 79691776),
    "32768-40x4-s0-mul_relin-r0": (42991616, 31457280),
    "32768-40x4-s0-mul_relin-r1": (49283072, 35651584),
    "32768-40x4-s1-keyswitch-2": (18874368, 14680064),
    "32768-40x4-s1-keyswitch-3": (18874368, 14680064),
    "32768-40x4-s1-rotate": (23592960, 17825792),
    "32768-40x4-s1-rotate_prepared": (36175872, 24117248),
    "32768-40x4-s1-rotate_prepared-b8": (52428800, 17825792),
    "32768-40x4-s1-rotate_many": (44564480, 32505856),
    "32768-40x4-s1-rotate_many_prepared": (36175872, 24117248),
    "32768-40x4-s1-keyswitch_window": (50331648, 33554432),
    "32768-40x4-s1-matmul_diag": (51904512, 34603008),
    "32768-40x4-s1-matmul_bsgs": (86507520, 57671680),
    "32768-40x4-s1-matmul_bsgs_blocks": (86507520, 57671680),
    "32768-40x4-s1-rotate_sum": (23592960, 17825792),
    "32768-40x4-s1-matmul_bsgs_fold": (95944704, 63963136),
    "32768-40x4-s1-mul_relin-r0": (35389440, 25690112),
    "32768-40x4-s1-mul_relin-r1": (40108032, 28835840),
    "4096-50x4-s0-mul_relin-r0": (37093376, 35913728),
    "4096-50x4-s0-mul_relin-r1": (37879808, 36438016),
    "4096-50x4-s1-mul_relin-r0": (36405248, 35454976),
    "4096-50x4-s1-mul_relin-r1": (36995072, 35848192),
    "64-30x6-k2g2l3-keyswitch_grouped-2": (30720, 20480),
    "64-30x6-k2g2l3-keyswitch_grouped-3": (30720, 20480),
    "64-30x6-k2g2l3-rotate_grouped": (39936, 26624),
    "64-30x6-k2g2l3-rotate_many_grouped": (46080, 30720),
    "64-30x6-k2g2l3-matmul_diag_grouped": (86016, 57344),
    "64-30x6-k2g2l3-matmul_bsgs_grouped": (101376, 67584),
    "64-30x6-k2g2l3-mul_relin_grouped-r0": (62976, 41984),
    "64-30x6-k2g2l3-mul_relin_grouped-r1": (62976, 41984),
    "32768-40x5-k2g2l3-keyswitch_grouped-2": (23592960, 15728640),
    "32768-40x5-k2g2l3-keyswitch_grouped-3": (23592960, 15728640),
    "32768-40x5-k2g2l3-rotate_grouped": (28311552, 18874368),
    "32768-40x5-k2g2l3-rotate_many_grouped": (39321600, 26214400),
    "32768-40x5-k2g2l3-matmul_diag_grouped": (59768832, 39845888),
    "32768-40x5-k2g2l3-matmul_bsgs_grouped": (66060288, 44040192),
    "32768-40x5-k2g2l3-mul_relin_grouped-r0": (40108032, 26738688),
    "32768-40x5-k2g2l3-mul_relin_grouped-r1": (40108032, 26738688),
}


@functools.lru_cache(maxsize=None)
def _buf(seed, qs, prefix, N):
    return tf.DeviceBuffer.from_numpy(np.ascontiguousarray(H.rand_residues(np.random.default_rng(seed), list(qs), prefix, N), dtype=np.uint64))


def _galois(N, n):
    return [pow(3, s + 1, 2 * N) for s in range(n)]


def _products(ctx, qs, N, level, n_digits, entry, batch, out, head, grouped):
    """2 rotations for the diagonal product; 1 baby step, 2 giant steps, 2 inputs and fold groups (1, 1) for the others"""
    q, cq = tuple(qs), tuple(qs[:level])
    keys = [_buf(10 + r, q, (n_digits, 2), N).ptr for r in range(5)]
    gs = _galois(N, 5)
    cts = [_buf(20 + m, cq, (batch, 2), N).ptr for m in range(2)]
    diags = [_buf(30 + m, cq, (3, 2), N).ptr for m in range(2)]           # [n_giant + 1][n_baby + 1][level][N]
    bias = _buf(40, cq, (), N).ptr
    if entry == "matmul_diag":
        d = _buf(50, cq, (3,), N).ptr                                     # [n_rot + 1][level][N]
        f = ctx.matmul_diag_grouped if grouped else ctx.matmul_diag
        f(*head, keys[:2], n_digits, gs[:2], d, cts[0], out.ptr, batch)
    elif entry == "matmul_bsgs" and grouped:
        ctx.matmul_bsgs_grouped(*head, keys[:1], gs[:1], keys[1:3], gs[1:3], n_digits, diags, cts, bias, out.ptr, batch)
    elif entry == "matmul_bsgs":
        ctx.matmul_bsgs(*head, keys[:1], gs[:1], keys[1:3], gs[1:3], n_digits, diags[0], cts[0], out.ptr, batch)
    elif entry == "matmul_bsgs_blocks":
        ctx.matmul_bsgs_blocks(*head, keys[:1], gs[:1], keys[1:3], gs[1:3], n_digits, diags, cts, bias, out.ptr, batch)
    elif entry == "rotate_sum":
        ctx.rotate_sum(*head, [[keys[3]], [keys[4]]], [[gs[3]], [gs[4]]], n_digits, cts[0], out.ptr, batch)
    else:
        assert entry == "matmul_bsgs_fold"
        ctx.matmul_bsgs_fold(*head, keys[:1], gs[:1], keys[1:3], gs[1:3], n_digits, diags, cts, [[keys[3]], [keys[4]]], [[gs[3]], [gs[4]]], bias,
                             out.ptr, batch)


def plain_call(ctx, qs, special, entry):
    N, Lk = ctx.N, len(qs)
    level = Lk - 1 if special else Lk
    q, cq = tuple(qs), tuple(qs[:level])
    batch = 8 if entry.endswith("-b8") else BATCH
    out = tf.DeviceBuffer(2 * batch * 2 * level * N)                      # (two rotations' worth)
    key = _buf(10, q, (Lk, 2), N).ptr
    g = _galois(N, 2)
    if entry.startswith("keyswitch-"):
        polys = int(entry[-1])
        ctx.keyswitch(Lk, level, special, key, Lk, _buf(21, cq, (batch, polys), N).ptr, polys, out.ptr, batch)
    elif entry == "keyswitch_window":
        nkey = spec.ndigits(int(np.prod([int(x) for x in qs], dtype=object)), 2 ** W)
        ctx.keyswitch_window(level, W, _buf(12, q, (nkey, 2), N).ptr, nkey, _buf(21, cq, (batch, 3), N).ptr, 3, out.ptr, batch, key_limbs=Lk,
                             special=special)
    elif entry.startswith("rotate_many"):
        ctx.rotate_many(Lk, level, special, [key, _buf(11, q, (Lk, 2), N).ptr], Lk, g, _buf(20, cq, (batch, 2), N).ptr, out.ptr, batch,
                        prepared=entry.endswith("prepared"))
    elif entry.startswith("rotate"):
        ctx.rotate(Lk, level, special, key, Lk, g[0], _buf(20, cq, (batch, 2), N).ptr, out.ptr, batch, prepared="prepared" in entry)
    elif entry.startswith("mul_relin"):
        ctx.mul_relin(Lk, level, special, key, Lk, _buf(20, cq, (batch, 2), N).ptr, _buf(21, cq, (batch, 2), N).ptr, out.ptr, batch,
                      rescale=entry.endswith("r1"))
    else:
        _products(ctx, qs, N, level, Lk, entry, batch, out, (Lk, level, special), False)
    return out


def grouped_call(ctx, qs, entry):
    N, Lk, level = ctx.N, len(qs), GLEVEL
    q, cq = tuple(qs), tuple(qs[:level])
    nd = -(-(Lk - K) // GROUP)                                            # the digits of a key made for the whole ciphertext ring
    out = tf.DeviceBuffer(2 * BATCH * 2 * level * N)
    key = _buf(10, q, (nd, 2), N).ptr
    g = _galois(N, 2)
    if entry.startswith("keyswitch_grouped"):
        polys = int(entry[-1])
        ctx.keyswitch_grouped(Lk, level, K, GROUP, key, nd, _buf(21, cq, (BATCH, polys), N).ptr, polys, out.ptr, BATCH)
    elif entry == "rotate_grouped":
        ctx.rotate_grouped(Lk, level, K, GROUP, key, nd, g[0], _buf(20, cq, (BATCH, 2), N).ptr, out.ptr, BATCH)
    elif entry == "rotate_many_grouped":
        ctx.rotate_many_grouped(Lk, level, K, GROUP, [key, _buf(11, q, (nd, 2), N).ptr], nd, g, _buf(20, cq, (BATCH, 2), N).ptr, out.ptr, BATCH)
    elif entry.startswith("mul_relin_grouped"):
        ctx.mul_relin_grouped(Lk, level, K, GROUP, key, nd, _buf(20, cq, (BATCH, 2), N).ptr, _buf(21, cq, (BATCH, 2), N).ptr, out.ptr, BATCH,
                              rescale=entry.endswith("r1"))
    else:
        _products(ctx, qs, N, level, nd, entry[:-len("_grouped")], BATCH, out, (Lk, level, K, GROUP), True)
    return out


def pinned(ident, N, qs, call):
    got = []
    for chunk in (0, CAP):
        ctx = tf.Context(N, qs)                                           # fresh: the block is this call's, and only this call's
        assert ctx.workspace() == (0, 0)
        ctx.set_chunk(chunk)
        keep = call(ctx)
        ctx.sync()
        got.append(ctx.workspace()[1])
        del keep
    print(f'    "{ident}": ({got[0]}, {got[1]}),')
    assert tuple(got) == BYTES[ident], (ident, got, BYTES[ident])


@pytest.mark.parametrize("entry", PLAIN_ENTRIES)
@pytest.mark.parametrize("N,qspec,special", PLAIN_RINGS)
def test_plain_keys(N, qspec, special, entry):
    qs = ring_of(N, qspec)
    pinned(f"{N}-{qspec}-s{special}-{entry}", N, qs, lambda ctx: plain_call(ctx, qs, special, entry))


@pytest.mark.parametrize("rescale", [0, 1])
@pytest.mark.parametrize("special", [0, 1])
def test_mul_relin_fused_cores(special, rescale):
    """N = 2^12 on fp64-size moduli: the fused product cores, whose parking rows are the layout's fixed tail"""
    N = 1 << 12
    qs = ring_of(N, "50x4")
    pinned(f"{N}-50x4-s{special}-mul_relin-r{rescale}", N, qs, lambda ctx: plain_call(ctx, qs, special, f"mul_relin-r{rescale}"))


@pytest.mark.parametrize("entry", GROUPED_ENTRIES)
@pytest.mark.parametrize("N,bits,Lk", GROUPED_RINGS)
def test_grouped_keys(N, bits, Lk, entry):
    qs = H.chain(bits, Lk, N)
    pinned(f"{N}-{bits}x{Lk}-k{K}g{GROUP}l{GLEVEL}-{entry}", N, qs, lambda ctx: grouped_call(ctx, qs, entry))
