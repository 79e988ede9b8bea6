"""A context outlives the plans made on it, whatever order their finalizers run in.

tfhe_bfv_plan_destroy and tfhe_plain_plan_destroy drain the streams of the plan's contexts, so they read the context: a context
destroyed first is read after it was freed.  The finalizers of a garbage cycle -- a script's globals at interpreter exit -- run in
any order; the binding therefore defers a context's destroy until the last plan on it has closed.  No device: the library is a
recorder."""
import toyfhe_jl_amd as tf


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            if name.endswith("_create"):
                a[-1]._obj.value = 1000 + len(self.calls)      # the handle, through byref
            if name.endswith("_destroy"):
                self.calls.append((name, a[0]))
            return 0
        return f


def fake(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(tf.native, "lib", lambda: rec)
    monkeypatch.setattr(tf.native, "check", lambda rc: None)
    return rec


def test_a_context_closed_first_is_destroyed_after_its_plans(monkeypatch):
    rec = fake(monkeypatch)
    small, big = tf.Context(64, [97, 193]), tf.Context(64, [97, 193, 257])
    bfv, plain = tf.BfvPlan(small, big, 17), tf.PlainPlan(small, 17)
    hs, hb, hp, hq = small.h, big.h, bfv.h, plain.h
    small.__del__()                                         # the order a garbage cycle may choose: contexts first
    big.__del__()
    assert rec.calls == [] and small.h == hs and big.h == hb
    bfv.__del__()
    assert rec.calls == [("tfhe_bfv_plan_destroy", hp), ("tfhe_ctx_destroy", hb)]      # small still has the codec on it
    plain.__del__()
    assert rec.calls[2:] == [("tfhe_plain_plan_destroy", hq), ("tfhe_ctx_destroy", hs)]
    for o in (small, big, bfv, plain):
        o.__del__()                                         # closing twice does nothing
    assert len(rec.calls) == 4


def test_one_context_for_both_rings_and_the_usual_order(monkeypatch):
    rec = fake(monkeypatch)
    ctx = tf.Context(64, [97, 193, 257])
    plan = tf.BfvPlan(ctx, ctx, 17, idx_s=[0, 1])
    hc, hp = ctx.h, plan.h
    plan.close()
    assert rec.calls == [("tfhe_bfv_plan_destroy", hp)] and ctx.h == hc
    ctx.close()
    assert rec.calls[1:] == [("tfhe_ctx_destroy", hc)] and ctx.h is None
