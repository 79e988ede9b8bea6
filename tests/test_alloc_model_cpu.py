"""The device allocator's threading contract on the CPU (no GPU, nothing loaded into Python).  tests/alloc_model/alloc_model.cpp
includes the real csrc/dev_alloc.h against a host model of the eleven HIP calls it makes (tests/alloc_model/hip/hip_runtime.h) and
drives it from four worker threads, a "device" thread and a thread that registers / unregisters a fifth stream, checking at every
hand-out that the work enqueued before the block's release can no longer touch it; scripted scenarios pin the single paths
(busy stream, back-pressure wait, alloc_ws stream wait, destroyed stream, foreign device, a hard event-query error at the front of
the parked queue, the destroy order).  The program is built three ways -- plain, ThreadSanitizer, AddressSanitizer + UBSan -- and run
as a stand-alone executable; it returns non-zero on any violation, and its two negative controls (an event query that always says
"complete"; a stream unregistered while busy) must be REPORTED by its checker for it to return zero.  The counters it prints are
held to minimums, so that a run cannot pass by doing nothing."""
import os
import re
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
SRC = os.path.join(TESTS, "alloc_model", "alloc_model.cpp")
INCLUDES = ("-I" + os.path.join(TESTS, "alloc_model"), "-I" + os.path.join(ROOT, "toyfhe.jl_amd", "csrc"))   # the model's hip/ first
BUILDS = {
    "plain": ("-O2",),
    "thread": ("-O1", "-g", "-fsanitize=thread", "-fno-omit-frame-pointer"),
    "address_undefined": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"),
}
SANITIZER_REPORT = re.compile(r"ThreadSanitizer|AddressSanitizer|LeakSanitizer|UndefinedBehaviorSanitizer|runtime error:")


def counters(out, run):
    line = [l for l in out.splitlines() if l.startswith("run %s:" % run)]
    assert len(line) == 1, out[-3000:]
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line[0])}


@pytest.mark.parametrize("build", list(BUILDS))
def test_allocator_model_holds_the_hand_out_invariant_on_threads(build, tmp_path):
    exe = str(tmp_path / ("alloc_model_" + build))
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-pthread", "-Wall", "-Wextra", *BUILDS[build], *INCLUDES, SRC, "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout[-4000:]
    env = {k: v for k, v in os.environ.items() if k not in ("TFHE_ALLOC_CACHE", "TFHE_ALLOC_SOFT_GIB", "TFHE_ALLOC_DEBUG")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    out = r.stdout
    print(out[-6000:])
    assert not SANITIZER_REPORT.search(out), out[-6000:]
    assert r.returncode == 0, out[-6000:]
    assert "scenarios: failed=0 violations=0" in out
    ample, small, lying = (counters(out, k) for k in ("ample", "small", "lying"))
    assert ample["violations"] == 0 and small["violations"] == 0
    assert ample["rehandouts"] >= 10000 and small["rehandouts"] >= 10000          # hand-outs of released blocks, each one checked
    assert small["waits"] > 0 and small["trims"] > 0                                # back-pressure and the deferred trim were reached
    assert ample["ws_wait_handouts"] + small["ws_wait_handouts"] >= 1               # alloc_ws took a parked block behind a stream wait
    assert lying["violations"] > 0                                                  # the checker sees a weakened completion test
