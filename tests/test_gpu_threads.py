"""The threading contract of include/toyfhe_hip.h on the device: different contexts and plans driven from different host threads,
tfhe_free and tfhe_ctx_destroy from any thread, and a freed block never handed out while a kernel enqueued before its tfhe_free can
still touch it, whatever stream the next user runs on (csrc/dev_alloc.h).  The allocator's tables themselves run on the CPU under
sanitizers in tests/test_alloc_model_cpu.py; here the real streams.

Every scenario is ONE fresh child process (tests/gpu_threads_child.py, which states what each scenario does) with a timeout, one child
at a time, at most 8 threads in it: a deadlock ends as a killed child and a failed test.  After a child that timed out or died on a
signal this module starts nothing further on the device.  All comparisons are bit-exact (the serial run of the same calls in the same
child, oracle.ref_cpu for item 0); all memory a scenario touches stays allocated throughout, so the worst outcome is wrong words.

Scenario 1 makes its serial run AFTER the threads, not before: before the barrier nothing may have called into the library, so that
contexts, tables and the first-use paths of launch.h and md_api.inc are first used by racing threads.

Scenario 4's second leg (a workspace borrower on B, so that alloc_ws's stream wait is what reuses X) is not at a small shape: a call
borrows only above TFHE_WS_KEEP_GIB, which is read as whole GiB (at least 1), so the tfhe_matmul_diag there has 512 ciphertexts of 5
limbs (a 1.4 GiB workspace; still about a second).  The same path at kilobytes is in the model (scenario_ws_wait, the threaded runs)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "gpu_threads_child.py")
TIMEOUT_S = 240
SMALL_SOFT = {"TFHE_ALLOC_SOFT_GIB": "0.0001"}     # ~100 KiB: one parked block is past it, so tfhe_malloc waits for it (dev_alloc.h alloc)
_stopped = []                                      # why nothing further is started on the device


def run_child(scenario, extra_env=None):
    if _stopped:
        pytest.fail("not started: " + _stopped[0])
    env = {k: v for k, v in os.environ.items() if k not in ("TFHE_ALLOC_CACHE", "TFHE_ALLOC_SOFT_GIB", "TFHE_WS_KEEP_GIB", "TFHE_LANES")}
    env.update(extra_env or {})
    try:
        out = subprocess.run([sys.executable, CHILD, scenario], capture_output=True, text=True, timeout=TIMEOUT_S, env=env)
    except subprocess.TimeoutExpired:
        _stopped.append("the child of scenario %r did not end within %d s" % (scenario, TIMEOUT_S))
        pytest.fail(_stopped[0])
    if out.returncode < 0 or out.returncode in (3, 134, 137, 139):
        _stopped.append("the child of scenario %r ended with status %d (a signal, or a thread that never finished)" % (scenario, out.returncode))
        pytest.fail(_stopped[0] + "\n" + out.stdout[-2000:] + out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    report = json.loads(lines[-1])
    print(scenario, report)
    assert "why" not in report, report["why"]
    return report, out.returncode


def test_four_rings_on_four_threads_first_use_at_once_and_error_text_per_thread():
    """scenarios 1 and 2: a 50-bit ring (fp64 policy, with tfhe_matmul_diag), a 60-bit ring (u64 policy), the mixed 60/40-bit ring at the
    size where its lanes fork, a BFV plan over two contexts -- one thread each, 8 steps without host synchronisation, freeing as they go;
    beside them a thread whose every call is refused on the host and whose tfhe_last_error is its own each time"""
    report, rc = run_child("rings")
    assert sorted(report["rings"]) == ["bfv", "fp50", "mixed", "u60"]
    for name, r in report["rings"].items():
        assert r["iterations"] == 8 and r["outputs"] == (2 if name == "fp50" else 1), (name, r)
        assert r["equal_serial"], (name, "a threaded step differs from the serial run")
        assert r["equal_oracle"], (name, "item 0 of the first step differs from the oracle")
    assert report["rejected_rounds"] >= 200
    assert report["ok"] and rc == 0


def test_frees_from_a_finaliser_thread_while_the_producer_keeps_enqueuing():
    """scenario 3"""
    report, rc = run_child("finaliser")
    assert report["equal_serial"] and report["equal_oracle"]
    assert report["live_after"] == report["live_before"]
    assert report["reuses"] > 0 and report["fills"] >= 50
    assert report["ok"] and rc == 0


def test_hand_out_waits_for_work_queued_on_another_stream():
    """scenario 4, first leg: X is read by the end of a long queue on A, freed, allocated again and overwritten through B"""
    report, rc = run_child("handout", SMALL_SOFT)
    assert report["same_address"] and report["reuses"] >= 1, ("reuse not reached", report)
    assert report["equal_oracle"], "Y is not the transform of X: the block came back while A's queue could still read it"
    assert report["ok"] and rc == 0


def test_workspace_borrower_takes_the_parked_block_behind_a_stream_wait():
    """scenario 4, second leg: the next user of X is the per-call workspace of a tfhe_matmul_diag on B (alloc_ws: B's stream is made to
    wait for X's release events, the host is not)"""
    report, rc = run_child("handout_ws", {"TFHE_WS_KEEP_GIB": "1"})
    assert report["reuses"] >= 1 and report["hip_mallocs"] == 0 and report["cached_after"] == report["workspace_bytes"], ("reuse not reached", report)
    assert report["a_pending_ms"] > 1.0, ("reuse not reached: A's queue had drained before the product's call returned", report)
    assert report["equal_oracle"], "Y is not the transform of X: the product's workspace was written while A's queue could still read it"
    assert report["product_equal_serial"] and report["product_equal_oracle"]
    assert report["ok"] and rc == 0


def test_destroy_drains_before_the_allocator_forgets_the_stream():
    """scenario 5: tfhe_ctx_destroy(A) on its own thread, tfhe_free(X) inside it (tfhe_ctx_destroy: synchronise, THEN unregister_stream)"""
    report, rc = run_child("destroy", SMALL_SOFT)
    assert report["overlap"], ("no overlap", report)
    assert report["same_address"] and report["reuses"] >= 1, ("reuse not reached", report)
    assert report["equal_oracle"], "Y is not the transform of X: the free inside the destroy recorded no event on A's stream"
    assert report["ok"] and rc == 0
