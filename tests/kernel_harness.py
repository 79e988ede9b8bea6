"""What the no-GPU tests of the kernel bodies share: the host build of an emulation source (tests/*_emul/*.cpp), the gfx950 probe
compile that reports a kernel's registers, scratch and static LDS (tests/*_emul/resource_probe.hip), and the dynamic LDS a fused row
kernel's launch asks for.  Test infrastructure only; resource figures only: nothing here looks at a kernel's instructions."""
import ctypes as C
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
LDS_LIMIT = 163840   # bytes of LDS a workgroup may use on gfx950 (160 KiB)
EMUL_FLAGS = ("-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


def build_emul(src, outdir, extra_flags=()):
    """tests/`src` compiled for the host into `outdir` ($CXX, else g++; EMUL_FLAGS, then `extra_flags`) and loaded"""
    so = os.path.join(str(outdir), "lib" + os.path.splitext(os.path.basename(src))[0] + ".so")
    cmd = [os.environ.get("CXX", "g++"), *EMUL_FLAGS, *extra_flags, "-o", so, os.path.join(TESTS, src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout[-4000:]
    return C.CDLL(so)


def md_acc_emul(outdir):
    """tests/md_acc_emul/md_acc_emul.cpp (the accumulation bodies of lazy_sum.h in the order of k_md_acc / k_md_acc_dense, nin inputs
    chained through the seed) built into `outdir` and bound: its three tests share the binding"""
    L = build_emul("md_acc_emul/md_acc_emul.cpp", outdir)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.md_acc_emul_chunk.argtypes, L.md_acc_emul_chunk.restype = [u64], C.c_uint
    L.md_acc_emul_dense.argtypes, L.md_acc_emul_dense.restype = [u64, C.c_int, u32, u32, u32, u32, vp, vp, vp, vp], C.c_int
    L.md_acc_emul_gather.argtypes, L.md_acc_emul_gather.restype = [u64, C.c_int, C.c_int, u64, u32, u32, u32, u32] + [vp] * 7, C.c_int
    return L


def kernel_resources(src, outdir, defines=()):
    """tests/`src` compiled for gfx950 with -D`defines`: one record per kernel of the code object, in the compiler's order --
    {"name": mangled name, "vgprs", "agprs", "scratch": bytes per lane, "static_lds": bytes per block}"""
    obj = os.path.join(str(outdir), "_".join(("probe", *(d.split("=")[-1] for d in defines))) + ".o")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value", "--cuda-device-only", "-c",
           os.path.join(TESTS, src), *("-D" + d for d in defines), "-o", obj, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    fields = (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
              ("static_lds", r"LDS Size \[bytes/block\]: (\d+)"))
    return [dict(name=b.split()[0], **{k: int(re.search(pattern, b).group(1)) for k, pattern in fields})
            for b in re.split(r"remark: [^\n]*Function Name: ", r.stdout)[1:]]


def probe_all(src, outdir, jobs):
    """kernel_resources(src, outdir, defines) for every `defines` of `jobs`, compiled side by side"""
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        return list(ex.map(lambda defines: kernel_resources(src, outdir, defines), jobs))


def lds_bytes(lib, lb):
    """the dynamic LDS bytes the launch of a fused row kernel asks for at N = 2^lb (launch_fused_rows: lds_words<LOGB, LOGT>() * 8),
    evaluated from ntt_core.h by `lib`, any emulation built on tests/row_emul.h"""
    lib.row_emul_lds_bytes.argtypes, lib.row_emul_lds_bytes.restype = [C.c_int], C.c_long
    n = lib.row_emul_lds_bytes(lb)
    assert n > (8 << lb), (lb, n)      # the row itself and some padding (-2: no fused row kernel at this size)
    return n
