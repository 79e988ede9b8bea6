"""No-GPU checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/toyfhe_hip.h declares, and fails loudly (never silently falls back) without a device."""
import ctypes
import os
import re

import pytest

import toyfhe_jl_amd as tf
from toyfhe_jl_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "toyfhe_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tfhe_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_all_exported():
    lib = native.lib()
    decl = _declared_symbols()
    assert len(decl) >= 40
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in include/toyfhe_hip.h but not exported"
    assert sorted(native.EXPORTED_SYMBOLS) == decl


def test_product_does_not_touch_oracle():
    pkg = os.path.join(ROOT, "toyfhe.jl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".inc", ".cpp", ".jl")):
                src = open(os.path.join(dirpath, f), errors="replace").read()
                assert "from oracle" not in src and "import oracle" not in src and "ref_cpu" not in src, f
                assert "libemul" not in src, f


def test_kernels_are_launched_through_the_helper_only():
    """csrc/launch.h is the one place that launches a kernel and raises a kernel's dynamic-LDS limit (once per device and
    kernel, behind a mutex).  No other source launches by hand, sets the attribute itself, or keeps a function-local
    `static bool` that remembers an attribute was set: those flags were unsynchronised and process-wide."""
    csrc = os.path.join(ROOT, "toyfhe.jl_amd", "csrc")
    helper = open(os.path.join(csrc, "launch.h")).read()
    assert helper.count("hipLaunchKernelGGL(") == 1 and helper.count("hipFuncSetAttribute(") == 1
    assert "std::mutex" in helper
    seen = 0
    for f in sorted(os.listdir(csrc)):
        if f == "launch.h" or not f.endswith((".h", ".hip", ".inc", ".cpp")):
            continue
        seen += 1
        src = open(os.path.join(csrc, f), errors="replace").read()
        for banned in ("hipFuncSetAttribute", "hipLaunchKernelGGL", "hipLaunchKernel(", "hipModuleLaunchKernel", "<<<", "set_lds"):
            assert banned not in src, f"{f}: {banned} outside csrc/launch.h"
        # a mutable function-local or file-scope `static bool` is how the attribute flags were kept (`static const bool` switches
        # read from the environment and `static bool f(...)` functions are something else)
        flags = re.findall(r"^.*\bstatic\s+bool\s+\w+\s*(?:=|;).*$", src, flags=re.M)
        assert not flags, f"{f}: {flags}"
    assert seen >= 15


@pytest.mark.skipif(native.device_count() > 0, reason="only meaningful without a GPU")
def test_fails_loudly_without_device():
    with pytest.raises(tf.HipError):
        tf.Context(16, [1099511627873])
    with pytest.raises(tf.HipError):
        tf.DeviceBuffer(16)


def test_argument_validation_precedes_device_use():
    # these are rejected on the host before any HIP call, so they behave the same with or without a GPU
    with pytest.raises(AssertionError):
        tf.Context(12, [1099511627873])            # N not a power of two
    with pytest.raises(AssertionError):
        tf.Context(16, [1099511627873 + 2])        # not prime
    with pytest.raises(AssertionError):
        tf.Context(64, [97])                       # 2N does not divide q-1
    with pytest.raises(AssertionError):
        tf.Context(4, [97, 97])                    # repeated modulus
    lib = tf.native.lib()
    assert lib.tfhe_ctx_set_chunk(None, 8) == tf.native.E_BADARG and b"null context" in lib.tfhe_last_error()
    assert lib.tfhe_ctx_set_chunk(None, -1) == tf.native.E_BADARG and b"chunk cap" in lib.tfhe_last_error()   # the sign first


def test_workspace_accessors_reject_null_arguments():
    """tfhe_ctx_workspace / tfhe_bfv_plan_workspace only report state: a null owner or a null out pointer is TFHE_E_BADARG, on the
    host, and what the out pointers held is left alone."""
    lib = tf.native.lib()
    block = ctypes.create_string_buffer(8)                  # stands in for an owner; never dereferenced: an out pointer is null
    owner = ctypes.c_void_p(ctypes.addressof(block))
    for f in (lib.tfhe_ctx_workspace, lib.tfhe_bfv_plan_workspace):
        ptr, n = ctypes.c_void_p(1234), ctypes.c_size_t(5678)
        assert f(None, ctypes.byref(ptr), ctypes.byref(n)) == tf.native.E_BADARG and b"null" in lib.tfhe_last_error()
        assert f(owner, None, ctypes.byref(n)) == tf.native.E_BADARG and b"null" in lib.tfhe_last_error()
        assert f(owner, ctypes.byref(ptr), None) == tf.native.E_BADARG and b"null" in lib.tfhe_last_error()
        assert f(None, None, None) == tf.native.E_BADARG
        assert (ptr.value, n.value) == (1234, 5678)
