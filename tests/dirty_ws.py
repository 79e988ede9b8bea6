"""Run a call on a workspace that holds anything but what the call would like to find there.

A context keeps one long-lived scratch block (Context.workspace()), a BFV plan a second one (BfvPlan.workspace()); the entry points
carve their intermediates out of them and nothing ever clears them.  on_dirty_workspace fills the whole block between calls -- with
tfhe_memset on the owner's own stream, never inside a call -- and asks for the oracle's words every time:

    0x00   what a block fresh from the driver gives
    0xA5   words far above every modulus
    0xFF   all-ones words, which are NaN to the kernels of the fp64 policy

Shared by tests/test_gpu_dirty_workspace.py."""
import numpy as np

import toyfhe_jl_amd as tf

FILLS = (0x00, 0xA5, 0xFF)


def _stream_ctx(owner):
    """the context whose stream fills an owner's block: the context itself, or the small ring's of a BFV plan"""
    return owner if isinstance(owner, tf.Context) else owner.small


def memset(ctx, ptr, byte, nbytes):
    tf.native.check(tf.native.lib().tfhe_memset(ctx.h, ptr, byte, nbytes))


def fill(owner, byte):
    """set every byte of the owner's block as it is now; -> (ptr, bytes)"""
    ptr, nbytes = owner.workspace()
    if nbytes:
        ctx = _stream_ctx(owner)
        memset(ctx, ptr, byte, nbytes)
        ctx.sync()                                   # a plan's block is used from two streams: nothing of the fill is left in flight
    return ptr, nbytes


def on_dirty_workspace(owner, call, out, want, fills=FILLS, moduli=None, picks=None, also=(), compare=None):
    """owner: the Context or BfvPlan whose block `call` works in (`also`: further owners, filled alongside when they hold a block --
    the contexts under a BFV plan).  out / want: a DeviceBuffer and the oracle's words for it, or equally long lists of both; want was
    computed before any device call.  moduli: broadcastable against want (or a list, None entries allowed): every word read back is
    below it.  picks: rows of the leading axis that `want` covers (the oracle on a few ciphertexts of a large ring).  compare: for the
    floating-point codecs, whose words the oracle bounds but does not fix -- compare(k, words, want[k], byte) judges output k's flat
    words in place of the equality."""
    outs, wants = (list(out), list(want)) if isinstance(out, (list, tuple)) else ([out], [want])
    mods = list(moduli) if isinstance(moduli, (list, tuple)) else [moduli] * len(outs)
    assert len(outs) == len(wants) == len(mods)
    ctx = _stream_ctx(owner)
    call()                                           # sizes the workspace
    where = owner.workspace()
    assert where[0] and where[1] > 0, "the call left no workspace: the case does not belong here"
    for byte in fills:
        assert fill(owner, byte) == where
        held = [fill(o, byte) for o in also]
        poison = byte ^ 0x5A                         # 0x5A, 0xFF, 0xA5: never the fill
        for o in outs:
            memset(ctx, o.ptr, poison, o.n * 8)
        call()
        for k, (o, w, q) in enumerate(zip(outs, wants, mods)):
            if compare is not None:
                compare(k, o.to_numpy(), w, byte)
                continue
            got = o.to_numpy().reshape((-1,) + w.shape[1:])
            got = got if picks is None else got[picks]
            assert got.shape == w.shape, (hex(byte), k, got.shape, w.shape)
            assert np.array_equal(got, w), ("fill", hex(byte), "output", k, "words off", int((got != w).sum()))
            if q is not None:
                assert (got < q).all(), ("fill", hex(byte), "output", k)
        # had the block moved, the fill would have missed what the call used
        assert owner.workspace() == where, ("fill", hex(byte), "the workspace moved", where, owner.workspace())
        assert [o.workspace() for o in also] == held, ("fill", hex(byte), "a further workspace moved")
