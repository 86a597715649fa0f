"""The decode GEMV instantiations compiled into the library are exactly the ones accounted for (no GPU needed).

woq_gemv.h holds five kernel templates.  Every function symbol of theirs in the built library's gfx950 code objects
must be in one of three literal sets, and every member of the sets must be compiled:

  TABLE      what tests/test_gemv_matrix_gpu.py runs by name: woq_gemv_kernel, woq_gemv_m1_kernel, woq_gemv_m1s_kernel;
  ELSEWHERE  woq_gemv_m1_routed_kernel and woq_gemv_m1_dual_kernel, held bit for bit to the M = 1 forward by
             tests/test_moe_gpu.py and tests/test_batch_gpu.py;
  UNREACHED  compiled, but no call reaches them with any knob -- each with the host line that keeps it out, and none of
             them reported by the reachability sweep of tests/test_gemv_matrix_cpu.py.

Symbol names only: the code objects are taken out of neural_amd/libneural_amd.so and their symbol tables listed
demangled.
"""
import collections
import itertools
import os
import re
import shutil
import subprocess

import pytest

from tests.test_gemv_matrix_cpu import swept
from tests.test_gemv_matrix_gpu import TABLE, gemv_name, tf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "neural_amd", "libneural_amd.so")
FAMILIES = ("woq_gemv_kernel", "woq_gemv_m1_kernel", "woq_gemv_m1s_kernel", "woq_gemv_m1_routed_kernel",
            "woq_gemv_m1_dual_kernel")
# a function symbol of the table: "<value> g     F .text <size> [.protected] void nad::woq_gemv_...<...>(...)"
SYMBOL = re.compile(r"\sF \.text\s+[0-9a-f]+\s+(?:\.\w+ )?(?:void )?nad::(woq_gemv_\w*kernel)<([^>]*)>\(")

SLICES = [(1, 1), (2, 1), (4, 2), (4, 4)]  # (KSN, SPW) of gemv_m1_launch4 / routed_launch2
# (BITS, GPT, ASYM, ST) of the M = 1 stream: int4 with the runtime scale type, int2 with each (NAD_INT2_ST), four groups
# per tile sym only
M1_FORMATS = [(4, g, a, -1) for g in (1, 2) for a in (False, True)] + \
             [(2, g, a, st) for g in (1, 2) for a in (False, True) for st in (0, 1, 2)] + \
             [(2, 4, False, st) for st in (0, 1, 2)]

# woq_gemv_m1_routed_kernel<BITS, GPT, ASYM, KSN, SPW, kRoutedNst = 2, ST> (launch_gemv_routed: fp32 rows) and the two
# woq_gemv_m1_dual_kernel of launch_gemv_dual (int2 Q, K + int4 V at groups of 64 and of 128)
ELSEWHERE = {f"woq_gemv_m1_routed_kernel<{b}, {g}, {tf(a)}, {ksn}, {spw}, 2, {st}>"
             for (b, g, a, st), (ksn, spw) in itertools.product(M1_FORMATS, SLICES)} | {
    "woq_gemv_m1_dual_kernel<2, 4, 1, 4, 2, 2, 0>", "woq_gemv_m1_dual_kernel<2, 2, 1, 4, 1, 2, 0>"}

UNREACHED = {
    # capi_forward.hip prepare_gemv: `if (gpt == 0 || (gpt >= 4 && w0.asym)) return 0;` -- four groups per tile with
    # zero points never reach launch_gemv, whose gemv_launch2 instantiates them for int4 and int2
    gemv_name(bits, hilo, 4, True, nst) for bits in (4, 2) for hilo in (0, 1, 2) for nst in (1, 3)} | {
    # capi_forward.hip nad_batch_create: `prepare_gemv(b->a, ..., Act{p[0].act, kActF32, w0->k, 1, w0->k}, ...)` -- a
    # batch problem's activations are fp32 (nad_batch_problem.act is const float*), so gemv_m1_launch5's BATCH arm is
    # never taken with fp16 (AT 1) or bf16 (AT 2) rows
    f"woq_gemv_m1_kernel<{b}, {g}, {at}, {tf(a)}, {ksn}, {spw}, true, 3, {st}>"
    for (b, g, a, st), at, (ksn, spw) in itertools.product(M1_FORMATS, (1, 2), SLICES)}

assert len(ELSEWHERE) == 78 and len(UNREACHED) == 12 + 152


def _objdump():
    root = os.environ.get("ROCM_PATH", "/opt/rocm")
    for p in (os.path.join(root, "llvm", "bin", "llvm-objdump"), shutil.which("llvm-objdump")):
        if p and os.path.exists(p):
            return p
    return None


def compiled(tmp_path):
    """the library's GEMV kernel function symbols as 'family<template arguments>', one entry per symbol"""
    objdump = _objdump()
    if objdump is None or not os.path.exists(LIB):
        pytest.skip("the built library or llvm-objdump not found")
    link = tmp_path / "lib.so"
    os.symlink(LIB, link)  # --offloading writes each bundle entry next to its input
    subprocess.run([objdump, "--offloading", str(link)], check=True, capture_output=True)
    found = []
    for co in sorted(tmp_path.glob("lib.so.*gfx950")):
        table = subprocess.run([objdump, "-t", "--demangle", str(co)], check=True, capture_output=True, text=True)
        for line in table.stdout.splitlines():
            m = SYMBOL.search(line)
            if m and m.group(1) in FAMILIES:
                found.append(f"{m.group(1)}<{', '.join(a.strip() for a in m.group(2).split(','))}>")
    return found


def test_the_three_sets_are_disjoint():
    assert not (TABLE & ELSEWHERE) and not (TABLE & UNREACHED) and not (ELSEWHERE & UNREACHED)


def test_compiled_gemv_kernels_are_all_accounted_for(tmp_path):
    found = collections.Counter(compiled(tmp_path))
    assert [n for n, c in found.items() if c > 1] == [], "an instantiation compiled twice"
    have = set(found)
    per = collections.Counter(n.split("<")[0] for n in have)
    print("decode GEMV instantiations in the library:", ", ".join(f"{f} {per[f]}" for f in FAMILIES), "-- total",
          len(have))
    print(f"table {len(TABLE)}, elsewhere {len(ELSEWHERE)}, unreached {len(UNREACHED)}")
    expected = TABLE | ELSEWHERE | UNREACHED
    assert sorted(have - expected) == [], "compiled but in none of the three sets"
    assert sorted(expected - have) == [], "in a set but not compiled"


def test_no_unreached_kernel_is_reported_by_the_sweep(knob):
    assert sorted(swept(knob) & UNREACHED) == []
