"""csrc/ws_layout.h on the host (tests/ws_layout_emul): the one list of regions from which every key-switch and product entry point
takes the size of its workspace and its pointers, and the decision of the transform-scratch accessor.

The emulation's table -- N = 2, 16 (8 N no multiple of 256) and 2^15, chunks 1 and 512, with and without scratch rows, a nested user,
row regions (an empty one among them) and tails -- is read from the library and its answers are compared with the restatement below,
written from the layout's description and not from its code.  The same table runs once more as a stand-alone program built with
-fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import pytest

from tests.kernel_harness import EMUL_FLAGS, TESTS, build_emul

SRC = "ws_layout_emul/ws_layout_emul.cpp"
GROW, FITS, REFUSED = 0, 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = build_emul(SRC, tmp_path_factory.mktemp("ws_layout"))
    u64p = C.POINTER(C.c_uint64)
    L.ws_layout_emul_cases.restype = C.c_int
    L.ws_layout_emul_case.argtypes, L.ws_layout_emul_case.restype = [C.c_int, u64p], None
    L.ws_layout_emul.argtypes, L.ws_layout_emul.restype = [u64p, u64p], None
    L.ws_scratch_emul.argtypes, L.ws_scratch_emul.restype = [C.c_int, C.c_uint64, C.c_uint64], C.c_int
    L.ws_scope_emul.argtypes, L.ws_scope_emul.restype = [C.c_uint64] * 3, C.c_int
    return L


def cases(lib):
    for i in range(lib.ws_layout_emul_cases()):
        raw, out = (C.c_uint64 * 14)(), (C.c_uint64 * 9)()
        lib.ws_layout_emul_case(i, raw)
        lib.ws_layout_emul(raw, out)
        v = list(raw)
        k = dict(N=v[0], chunk=v[1], scratch=v[2], nested=(v[4], v[5]) if v[3] else None, rows=v[7:7 + v[6]], tails=v[12:12 + v[11]])
        yield k, dict(region0=out[0], per_ct=out[1], bytes=out[2], offsets=list(out)[3:3 + v[6] + v[11]])


def restated(k):
    """[ region 0 | chunk x rows x N words per row region | tails ]; region 0: the larger of the scratch rows (above N = 2^14) and the
    nested user's bytes, up to the next multiple of 256"""
    r0 = k["chunk"] * k["scratch"] * k["N"] * 8 if k["N"] > 2 ** 14 else 0
    if k["nested"]:
        r0 = max(r0, k["nested"][0] + k["chunk"] * k["nested"][1])
    r0 = -(-r0 // 256) * 256
    spans, at = [], r0
    for rows in k["rows"]:
        spans.append((at, at + k["chunk"] * rows * k["N"] * 8))
        at = spans[-1][1]
    for b in k["tails"]:
        spans.append((at, at + b))
        at = spans[-1][1]
    return r0, spans, at


def test_the_table_covers_the_sizes_and_chunks(lib):
    seen = [k for k, _ in cases(lib)]
    assert {k["N"] for k in seen} == {2, 16, 2 ** 15} and {k["chunk"] for k in seen} == {1, 512}
    assert any(k["nested"] and k["nested"][0] % 256 for k in seen) and any(not k["rows"] and not k["tails"] for k in seen)
    assert any(len(k["rows"]) == 4 and len(k["tails"]) == 2 for k in seen)


def test_regions_in_order_disjoint_and_the_size_is_the_last_end(lib):
    for k, got in cases(lib):
        r0, spans, end = restated(k)
        assert got["region0"] == r0 and r0 % 256 == 0, k
        assert got["per_ct"] == sum(k["rows"]) * k["N"] * 8, k
        assert got["offsets"] == [lo for lo, _ in spans], k
        assert got["bytes"] == end, k
        if spans:
            assert spans[0][0] == r0, k                                     # the first region starts where region 0 ends
        for (_, hi), (lo, _) in zip(spans, spans[1:]):                      # declaration order, back to back: pairwise disjoint
            assert lo == hi, k


def test_region0_is_empty_when_nothing_asks_for_it(lib):
    n = 0
    for k, got in cases(lib):
        if not k["nested"] and (k["N"] <= 2 ** 14 or not k["scratch"]):
            assert got["region0"] == 0 and (not got["offsets"] or got["offsets"][0] == 0), k
            n += 1
        else:
            assert got["region0"] > 0, k
    assert n > 0


def test_the_scratch_accessor_decides(lib):
    for k, got in cases(lib):
        r0 = got["region0"]
        assert lib.ws_scratch_emul(1, r0, r0) == FITS, k
        assert lib.ws_scratch_emul(1, r0, r0 + 1) == REFUSED, k             # one byte more than region 0 holds: never over the regions
        assert lib.ws_scratch_emul(0, r0, r0 + 1) == GROW and lib.ws_scratch_emul(0, 0, 1 << 40) == GROW, k
    assert lib.ws_scratch_emul(1, 0, 0) == FITS and lib.ws_scratch_emul(1, 0, 1) == REFUSED


def test_a_nested_scope_restores_the_outer_one(lib):
    # 512 bytes: refused in the nested user's 256, served from the outer 1024 after its return, grown when no layout is left in force
    assert lib.ws_scope_emul(1024, 256, 512) == REFUSED + 4 * FITS + 16 * GROW
    assert lib.ws_scope_emul(256, 1024, 512) == FITS + 4 * REFUSED + 16 * GROW


def test_the_table_under_the_sanitizers(tmp_path):
    """the stand-alone program: the table against the layout's invariants, address and undefined-behaviour sanitizers on"""
    exe = str(tmp_path / "ws_layout_emul_main")
    flags = [f for f in EMUL_FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [os.environ.get("CXX", "g++"), *flags, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DWS_LAYOUT_EMUL_MAIN",
           "-o", exe, os.path.join(TESTS, SRC)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and ", 0 bad" in r.stdout, r.stdout[-4000:]
