"""The woq_mid_kernel instantiations compiled into the library are exactly the reachable ones (no GPU needed).

woq_gemm_mid.hip derives its dispatch from the one shape rule the host plans with (mid_shape), so the set of kernels in
the built library must equal GEOMETRY of tests/test_mid_matrix_gpu.py -- the literal table the matrix test runs --
times sym / asym and fp32 / 16-bit scales: 240, no more and no fewer.  Symbol names only: the gfx950 code objects are
taken out of neural_amd/libneural_amd.so and their symbol tables listed demangled.
"""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_mid_matrix_gpu import ACTS, TUPLES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "neural_amd", "libneural_amd.so")
ACT_T = {"fp32": 0, "fp16": 1, "bf16": 2}  # kActF32 / kActF16 / kActBF16 (woq_kernels.h)
# a function symbol of the table: "<value> g     F .text <size> [.protected] void nad::mid::woq_mid_kernel<...>(...)"
SYMBOL = re.compile(r"\sF \.text\s+[0-9a-f]+\s+(?:\.\w+ )?(?:void )?"
                    r"nad::mid::woq_mid_kernel<([^>]*)>\(nad::GemmArgs\)\s*$")


def _objdump():
    root = os.environ.get("ROCM_PATH", "/opt/rocm")
    for p in (os.path.join(root, "llvm", "bin", "llvm-objdump"), shutil.which("llvm-objdump")):
        if p and os.path.exists(p):
            return p
    return None


def compiled(tmp_path):
    """{(BITS, GPT, ASYM, AT, RF, S, NW, SPW, SF32)} of the library's woq_mid_kernel function symbols"""
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
            if m:
                args = [a.strip() for a in m.group(1).split(",")]
                found.append(tuple(int(a == "true") if a in ("true", "false") else int(a) for a in args))
    assert len(found) == len(set(found)), "an instantiation compiled twice"
    return set(found)


def test_compiled_mid_kernels_are_the_reachable_ones(tmp_path):
    assert set(ACT_T) == set(ACTS)
    expected = {(bits, gpt, asym, ACT_T[act], rf, s, nw, spw, sf32) for bits, gpt, act, rf, s, nw, spw in TUPLES
                for asym in (0, 1) for sf32 in (0, 1)}
    assert len(expected) == 240
    have = compiled(tmp_path)
    print("woq_mid_kernel instantiations in the library:", len(have))
    assert sorted(have - expected) == [], "compiled but reached by no launch"
    assert sorted(expected - have) == [], "reachable but not compiled"
